"""The cases of tests/test_ff_numerics_cpu.py and tests/test_ff_numerics_gpu.py, built once: the MLP regressor (DropoutFF: `mlp_tile16.hip`,
`mlp_pipe.hip`, and `ff_bank.hip` in the banks) against a plain float64 evaluation at hostile inputs, and the oracle variants ("mutants")
that prove the cases can tell a subtly wrong kernel from a right one.  No kernel runs here and no kernel result enters a reference.

Reference : `ff_forward64(sd, x, mask)`: DropoutFF.forward (the reference's nn_models.py:340-354) in float64 on the float32 weights and the
            float32 inputs the kernel sees (with `normalize_input`: `hi.raw_and_normalised`'s, float64 z-score rounded once); leaky_relu
            slope float32(0.01) widened, the value the kernels multiply by.  Written from the model, not derived from `orc.ff_forward`.
Yardstick : `e_ref = max |orc.ff_forward - ff_forward64|` on the same case (the pinned float32 oracle's own rounding error).
Budget    : `max(1e-6, 4 e_ref)`, the project's rule (tests/test_hostile_inputs_gpu.py), over every row of the call.
Cases     : weights seed 3, inputs seed 21 (the hostile tests' seeds); the weight scale applies to every layer but `_output_layer`.
Routes    : ROUTES names every forward route with the shape that pins its edge as a function of the device's CU count; the CPU proofs
            evaluate them for PROOF_CUS compute units (the smallest device that has a pipeline), the GPU tests for the device at hand."""
import numpy as np

from oracle import ape_oracle as orc
from oracle import philox as ph
from tests import test_hostile_inputs_cpu as hi

SEED_W, SEED_X = hi.SEED_W, 21
FLOOR, FACTOR = 1e-6, 4.0
P_DROP = 0.2
SLOPE = np.float32(0.01)
PROOF_CUS = 16

# (I, H, n_hidden, O)
MODELS = {
    "pocket_like": (22, 256, 2, 14),   # tests/golden/ff.npz's deployed-like model
    "small": (20, 128, 1, 12),
    "least": (1, 128, 0, 1),           # the smallest legal model
    "most": (64, 256, 7, 32),          # APE_MAX_INPUT / APE_MAX_FF_LAYERS - 1 / APE_MAX_OUTPUT, KX = 64
    "i33": (33, 256, 1, 17),           # KX = 64 with 31 padded columns, O just past 16
    "pipe_most": (32, 256, 2, 16),     # the pipeline's own limits
    "pipe_least": (1, 256, 2, 1),
}
CASES = ("benign", "w4", "w16", "z1e3", "sat30", "zeros")
CASE_WSCALE = {"benign": 1.0, "w4": 4.0, "w16": 16.0, "z1e3": 1.0, "sat30": 4.0, "zeros": 1.0}


def budget(e_ref):
    return max(FLOOR, FACTOR * e_ref)


def padded_input(I):
    return 32 * ((I + 31) // 32)


def n_hidden_of(sd):
    return sum(1 for k in sd if k.startswith("_hidden_layers.") and k.endswith("weight"))


def state_dict(model, case):
    I, H, n_hidden, O = MODELS[model]
    sd = orc.make_ff_state_dict(I, H, n_hidden, O, SEED_W)
    s = np.float32(CASE_WSCALE[case])
    return {k: v if k.startswith("_output_layer.") else (v * s).astype(np.float32) for k, v in sd.items()}


def case_z(case, B, T, I, seed=SEED_X):
    """float64 z-scores [B,T,I].  `zeros`: standard-normal rows with every fifth batch entry exact +0.0 (0, 5, ..) and every fifth exact
    -0.0 (2, 7, ..): a zero row's input-layer products are all (signed) zeros, its pre-activation is the bias alone"""
    z = hi.case_z(case, B, T, I, seed)
    if case == "zeros":
        z[0::5] = 0.0
        z[2::5] = -0.0
    return z


# ---------------- the reference ----------------------------------------------------------------------------------------------------------
def ff_forward64(sd, x, mask=None):
    """x float32 [rows, I] (the values the input layer sees), mask [rows, H] of 0 or 1/(1-p) or None -> float64 [rows, O]"""
    w = lambda k: sd[k].astype(np.float64)
    slope = np.float64(SLOPE)
    a = np.asarray(x).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = a @ w("_input_layer.weight").T + w("_input_layer.bias")
        a = np.where(a > 0, a, slope * a)
        for k in range(n_hidden_of(sd)):
            a = a @ w(f"_hidden_layers.{k}.weight").T + w(f"_hidden_layers.{k}.bias")
            a = np.where(a > 0, a, slope * a)
        if mask is not None:
            a = a * np.asarray(mask).astype(np.float64)
        return a @ w("_output_layer.weight").T + w("_output_layer.bias")


# ---------------- the routes ---------------------------------------------------------------------------------------------------------------
def wide_rows(n_cus):
    """W: the row count from which the tile kernel takes its 32-row form and AUTO the pipeline"""
    return 64 * n_cus


def pipe_pairs(n_cus):
    return (n_cus // 16) * 8


TILE, SLOTS = 32, 4
_W = wide_rows
_ring = lambda tiles_per_pair, extra: (lambda c: TILE * pipe_pairs(c) * tiles_per_pair + extra)
# route id: (model, set_kernel, N(n_cus) rows of the call, mode, last_kernel() must equal, needs a pipeline)
#   mode: "rows" x [N,I] | "all" x [N,3,I] every step | "last" x [N,3,I] last_step_only | "zscore" raw features, normalize_input |
#         "mc" monte_carlo_predictions(N, one row): the kernel's own Philox mask | "masks" an injected mask
ROUTES = {
    "tile-1/pocket_like": ("pocket_like", "tile16", lambda c: 37, "rows", "ape_mlp_tile16", False),
    "tile-1/small": ("small", "tile16", lambda c: 37, "rows", "ape_mlp_tile16", False),
    "tile-1/least": ("least", "tile16", lambda c: 17, "rows", "ape_mlp_tile16", False),
    "tile-1/most": ("most", "tile16", lambda c: 37, "rows", "ape_mlp_tile16", False),
    "tile-1/i33": ("i33", "tile16", lambda c: 16, "rows", "ape_mlp_tile16", False),
    "tile-2/W+37": ("pocket_like", "tile16", lambda c: _W(c) + 37, "rows", "ape_mlp_tile16", False),      # last workgroup: 5 rows, second tile all padding
    "tile-2/W+17": ("pocket_like", "tile16", lambda c: _W(c) + 17, "rows", "ape_mlp_tile16", False),      # last workgroup: 17 rows, one in the second tile
    "tile-2-128": ("small", "tile16", lambda c: _W(c) + 17, "rows", "ape_mlp_tile16", False),
    "tile-2-kx64": ("most", "tile16", lambda c: _W(c), "rows", "ape_mlp_tile16", False),
    "steps/all": ("pocket_like", "tile16", lambda c: 37, "all", "ape_mlp_tile16", False),
    "steps/last": ("pocket_like", "tile16", lambda c: 37, "last", "ape_mlp_tile16", False),
    "zscore/tile16": ("pocket_like", "tile16", lambda c: 37, "zscore", "ape_mlp_tile16", False),
    "zscore/auto": ("pocket_like", "auto", lambda c: _W(c) + 37, "zscore", "ape_mlp_pipe", True),
    "pipe/W": ("pocket_like", "auto", lambda c: _W(c), "rows", "ape_mlp_pipe", True),                    # exact fill
    "pipe/W+1": ("pocket_like", "auto", lambda c: _W(c) + 1, "rows", "ape_mlp_pipe", True),              # a one-row ragged tile
    "pipe/W+37": ("pocket_like", "auto", lambda c: _W(c) + 37, "rows", "ape_mlp_pipe", True),
    "pipe/wrap1": ("pocket_like", "auto", _ring(SLOTS, 32), "rows", "ape_mlp_pipe", True),               # one pair's fifth tile: slot 0 again
    "pipe/wrap2": ("pocket_like", "auto", _ring(2 * SLOTS + 1, 5), "rows", "ape_mlp_pipe", True),        # second wrap, a 5-row tile at the end
    "pipe-dims/most": ("pipe_most", "auto", lambda c: _W(c) + 37, "rows", "ape_mlp_pipe", True),
    "pipe-dims/least": ("pipe_least", "auto", lambda c: _W(c) + 37, "rows", "ape_mlp_pipe", True),
    "mc/small": ("small", "auto", lambda c: 50, "mc", "ape_mlp_tile16", False),
    "mc/most": ("most", "auto", lambda c: 50, "mc", "ape_mlp_tile16", False),
    "mc/pocket_like": ("pocket_like", "auto", lambda c: 50, "mc", "ape_mlp_tile16", False),
    "masks": ("pocket_like", "auto", lambda c: _W(c) + 37, "masks", "ape_mlp_tile16", False),            # AUTO falls back to the tile kernel
}
STEPS = 3
MC_SEED = 0x789AB                # manual_seed of the mc routes: the call is Monte-Carlo call 1, key (MC_SEED << 20) + 1
STATS = "pocket"                 # the norm stats of the zscore routes (22 features, as pocket_like)


def route_rows(route, n_cus):
    """-> N, or None where the device cannot form the shape (no pipeline below 16 compute units)"""
    model, kernel, n_of, mode, last, needs_pipe = ROUTES[route]
    if needs_pipe and n_cus < 16:
        return None
    return int(n_of(n_cus))


_CASES = {}


def make_case(route, case, n_cus, norm_stats=None):
    """everything the tests need of one (route, case) on a device of `n_cus` compute units, computed once and never written to afterwards:
    x (what the model is given), xn float32 [rows, I] (what the input layer sees), mask, ref float64 [rows, O], e_ref, budget"""
    key = (route, case, n_cus)
    if key in _CASES:
        return _CASES[key]
    model, kernel, n_of, mode, last, needs_pipe = ROUTES[route]
    I, H, n_hidden, O = MODELS[model]
    N = route_rows(route, n_cus)
    sd = state_dict(model, case)
    T = STEPS if mode in ("all", "last") else 1
    z = case_z(case, 1 if mode == "mc" else N, T, I)
    st = None
    if mode == "zscore":
        st = norm_stats[STATS]
        x, xn = hi.raw_and_normalised(st, z)
    else:
        x = xn = z.astype(np.float32)
    seen = xn[:, -1] if mode != "all" else xn.reshape(N * T, I)            # rows in (b, t) order
    mask = None
    if mode == "mc":
        seen = np.repeat(seen, N, axis=0)
        mask = ph.ff_mask(ph.lstm_call_seed(MC_SEED, 1), N, H, P_DROP)
    elif mode == "masks":
        mask = ((np.random.default_rng(9).random((N, H)) >= P_DROP).astype(np.float32) / np.float32(1.0 - P_DROP)).astype(np.float32)
    if mode in ("rows", "masks"):
        x = x[:, 0]
    ref = ff_forward64(sd, seen, mask)
    e_ref = float(np.abs(orc.ff_forward(sd, seen, mask=mask) - ref).max())
    for a in (x, xn, seen, ref, *sd.values()) + (() if mask is None else (mask,)):
        a.setflags(write=False)
    c = dict(route=route, case=case, model=model, mode=mode, kernel=kernel, last=last, N=N, T=T, sd=sd, st=st, x=x, xn=xn, seen=seen,
             mask=mask, ref=ref, e_ref=e_ref, budget=budget(e_ref), magnitude=float(np.abs(ref).max()))
    _CASES[key] = c
    return c


def line(c, kernel=None, err=None):
    """the record line: FFNUM|route|kernel|model|N|case|e_ref|err|budget|ratio"""
    s = f"FFNUM|{c['route']}|{kernel or c['last']}|{c['model']}|N {c['N']}|{c['case']}|e_ref {c['e_ref']:.2e}"
    if err is None:
        return s + f"|budget {c['budget']:.2e}||y|max {c['magnitude']:.2e}"
    return s + f"|err {err:.2e}|budget {c['budget']:.2e}|ratio {err / c['budget']:.2f}"


# ---------------- non-finite rows --------------------------------------------------------------------------------------------------------
BAD_COL = 0        # column 0: the one a padded-column over-read of the row in front would pick up first (mutant `pad_reads_next_row`)


def bad_rows(route, n_cus):
    """the rows that take the NaN / +Inf: the middle of a tile, the last valid row of the last tile, and for the pipeline a row in the
    middle of a tile that lands in a ring slot used before (tile 4 P is the fifth tile of pair 0)"""
    N = route_rows(route, n_cus)
    mid = (N // 2) // TILE * TILE + 24 if N >= 64 else 24
    rows = [mid, N - 1]
    if ROUTES[route][4] == "ape_mlp_pipe":
        rows.append(TILE * pipe_pairs(n_cus) * SLOTS + 8)
    return [r for r in rows if r < N]


# ---------------- oracle variants ----------------------------------------------------------------------------------------------------------
# mutant: the routes on which a kernel could make that mistake
MUTANTS = {
    "slope_on_positive": ("tile-1/", "pipe/", "pipe-dims/"),        # 1  v * slope whatever the sign
    "no_last_activation": ("tile-1/", "pipe/", "pipe-dims/"),       # 2  no leaky_relu behind the last hidden layer
    "bias_dropped": ("tile-1/", "pipe/", "pipe-dims/"),             # 3  the last hidden layer's bias dropped
    "pad_reads_next_row": ("tile-1/", "pipe/", "pipe-dims/"),       # 4  padded input columns k >= I hold what follows in memory, not 0
    "second_tile_reads_first": ("tile-2",),                         # 5  rows 16..31 of a 32-row workgroup computed from rows 0..15
    "row_offset_early": ("steps/last",),                            # 6  [B,T,I] read one step early
    "outputs_ge16_at_bias": ("tile-1/most", "tile-1/i33"),          # 7  outputs o >= 16 left at the bias
    "mask_row_neighbour": ("mc/", "masks"),                         # 8  mask row r + 1 on row r
    "mask_before_last_hidden": ("mc/small", "mc/most", "mc/pocket_like", "masks"),   # 9  mask on the last hidden layer's input
    "zscore_neighbour_sd": ("zscore/",),                            # 10 z-score with xx_s of column k + 1
}


def mutant_routes(mutant):
    return [r for r in ROUTES if r.startswith(MUTANTS[mutant])]


def variant_forward(sd, x, mask=None, mutant=None, x_mem=None):
    """`ff_forward64` restated with one switch per mutant; `mutant=None` is bit-equal to it (asserted in tests/test_ff_numerics_cpu.py).
    `x_mem`: for `pad_reads_next_row`, the flat float32 memory behind row 0's first value, rows `I` apart"""
    assert mutant is None or mutant in MUTANTS, mutant
    w = lambda k: sd[k].astype(np.float64)
    slope = np.float64(SLOPE)
    n_hidden = n_hidden_of(sd)
    act = (lambda v: slope * v) if mutant == "slope_on_positive" else (lambda v: np.where(v > 0, v, slope * v))
    a = np.asarray(x).astype(np.float64)
    w0 = w("_input_layer.weight")
    if mutant == "pad_reads_next_row":
        rows, I = a.shape
        KX = padded_input(I)
        mem = np.concatenate([np.asarray(x_mem, dtype=np.float64).reshape(-1), np.zeros(KX)])
        a = mem[np.arange(rows)[:, None] * I + np.arange(KX)[None, :]]
        w0 = np.concatenate([w0, np.zeros((w0.shape[0], KX - I))], axis=1)        # the packed weights are zero there
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n_hidden + 1):
            last = j == n_hidden
            if last and mask is not None and mutant == "mask_before_last_hidden":
                a = a * np.asarray(mask).astype(np.float64)
            wj, bj = (w0, w("_input_layer.bias")) if j == 0 else (w(f"_hidden_layers.{j - 1}.weight"), w(f"_hidden_layers.{j - 1}.bias"))
            a = a @ wj.T + (0.0 if last and mutant == "bias_dropped" else bj)
            a = a if last and mutant == "no_last_activation" else act(a)
        if mask is not None and mutant != "mask_before_last_hidden":
            m = np.asarray(mask).astype(np.float64)
            a = a * (np.roll(m, -1, axis=0) if mutant == "mask_row_neighbour" else m)
        y = a @ w("_output_layer.weight").T + w("_output_layer.bias")
        if mutant == "outputs_ge16_at_bias":
            y[:, 16:] = w("_output_layer.bias")[16:]
    return y


def mutant_output(c, mutant, x=None):
    """what a kernel with the defect computes (to rounding) on case `c`, float64 [rows, O].  `x`: other rows in place of the case's own
    `seen` (the poisoned batches of the non-finite tests), mode "rows" only"""
    seen = c["seen"] if x is None else x
    if mutant == "second_tile_reads_first":
        y = c["ref"] if x is None else ff_forward64(c["sd"], seen, c["mask"])
        r = np.arange(len(y))
        return y[np.where(r % TILE >= 16, r - 16, r)]
    if mutant == "row_offset_early":
        assert c["mode"] == "last"
        seen = c["xn"][:, -2]
    if mutant == "zscore_neighbour_sd":
        st = c["st"]
        seen = ((c["x"][:, -1].astype(np.float64) - st["xx_m"]) / np.roll(st["xx_s"], -1)).astype(np.float32)
    return variant_forward(c["sd"], seen, c["mask"], mutant, x_mem=seen)
