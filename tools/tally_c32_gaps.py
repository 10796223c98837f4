#!/usr/bin/env python3
"""What stands between two MFMAs in the steady-state sections of the long-window instantiations of lstm_cluster32.hip (profiles/r10_cluster32_hot_gaps.md).

The kernel marks those sections in its device assembly with comment lines (`; c32 steady section, layer N: begin / end`).  Between a `begin` and
the next `end` this cuts the instructions into RUNS: maximal stretches of straight-line code -- no label, no branch, no barrier -- that hold
MFMAs.  A run is a piece of the MFMA stream as the one wave of a SIMD issues it; what stands between two MFMAs of a run is a GAP, and every scalar
instruction in a gap costs about twelve cycles.  A section whose hooks carry no branch comes out as few long runs (layer 0: the recurrent span;
layer 1: the relocated input span + its own input span, and the recurrent span behind the barrier between the spans); a branch around a hook cuts
a run in two and is counted as a BREAK inside the stream when fewer than `near` instructions separate the MFMAs on either side of it.

    tools/tally_c32_gaps.py file.hip|file.s [extra hipcc flags] [--json]
prints per instantiation and layer: MFMAs, runs, breaks; in the gaps of the runs: scalar instructions (s_waitcnt / s_nop apart), lane moves; the
gaps that hold a 16-byte-per-lane LDS-DMA (PIECE gaps) by their instructions; and the lines of the branches between the first and the last MFMA.
`tally(path)` returns the same as a dict (tests/test_c32_hot_gaps_cpu.py).  (Another compiler may lay a foreign block between two markers: its MFMAs
then show up as extra runs, and the test that reads this says so.)"""
import json, re, subprocess, sys, tempfile

MARK = re.compile(r";\s*c32 steady section, layer (\d): (begin|end)")
QUIET = ("s_waitcnt", "s_nop")                    # scalar opcodes every hook-free gap holds as well
is_mfma = lambda t: t.startswith(("v_mfma", "v_smfmac"))
is_cut = lambda t: t.endswith(":") or t.split()[0].startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm"))


def functions(path):
    """{kernel name: [(line number, text)]}: instructions, labels (`NAME:`) and markers (`MARK layer kind`) of each cluster32 kernel"""
    out, cur = {}, None
    for n, line in enumerate(open(path), 1):
        t = line.strip()
        m = MARK.search(t)
        c = t.split(";")[0].strip()
        if c.endswith(":") and "ape_lstm_cluster32" in c and not c.startswith(".") and not c.endswith(".kd:"):
            cur = out.setdefault(c[:-1], [])
        elif cur is None:
            continue
        elif c.startswith(".Lfunc_end"):
            cur = None
        elif m:
            cur.append((n, f"MARK {m.group(1)} {m.group(2)}"))
        elif c and (c.endswith(":") or not c.startswith((".", "//"))):
            cur.append((n, c))
    return out


def tally_section(ins, near=40):
    res = {"mfma": 0, "runs": [], "breaks": 0, "scalar_in_breaks": 0, "branches_in_breaks": 0, "scalar": 0, "quiet_scalar": 0, "lane_moves": 0, "lane_moves_anywhere": 0, "piece_gaps": [], "branch_lines": []}
    mf = [i for i, (_, t) in enumerate(ins) if is_mfma(t)]
    res["mfma"] = len(mf)
    res["lane_moves_anywhere"] = sum(1 for _, t in ins if t.startswith(("v_readlane", "v_writelane")))
    if not mf:
        return res
    res["branch_lines"] = [n for n, t in ins[mf[0]:mf[-1]] if t.startswith(("s_cbranch", "s_branch"))]
    run = 1
    for a, b in zip(mf, mf[1:]):
        body = ins[a + 1:b]
        if any(is_cut(t) for _, t in body):
            res["runs"].append(run)
            run = 1
            if len(body) < near:                  # a branch around a hook, inside the stream: what it and its mask arithmetic cost
                res["breaks"] += 1
                res["scalar_in_breaks"] += sum(1 for _, t in body if t.startswith("s_") and not t.startswith(QUIET + ("s_cbranch", "s_branch")))
                res["branches_in_breaks"] += sum(1 for _, t in body if t.startswith(("s_cbranch", "s_branch")))
            continue
        run += 1
        ops = [t.split()[0] for _, t in body]
        res["scalar"] += sum(1 for o in ops if o.startswith("s_") and not o.startswith(QUIET))
        res["quiet_scalar"] += sum(1 for o in ops if o.startswith(QUIET))
        res["lane_moves"] += sum(1 for o in ops if o.startswith(("v_readlane", "v_writelane")))
        if any(t.startswith("buffer_load_dwordx4") and t.endswith(" lds") for _, t in body):
            res["piece_gaps"].append({"line": ins[a][0], "ops": sorted(ops)})
    res["runs"].append(run)
    return res


def tally_function(ins):
    out, start = {}, None
    for i, (_, t) in enumerate(ins):
        if t.startswith("MARK") and t.endswith("begin"):
            start = i
        elif t.startswith("MARK") and t.endswith("end") and start is not None:
            out.setdefault("layer" + t.split()[1], []).append(tally_section(ins[start + 1:i]))
            start = None
    return out


def tally(path, flags=()):
    if path.endswith(".s"):
        return {k: tally_function(v) for k, v in functions(path).items()}
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", *flags, path, "-o", f.name],
                       check=True, stderr=subprocess.DEVNULL)
        return tally(f.name)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--json"]
    r = tally(args[0], args[1:])
    if "--json" in sys.argv:
        print(json.dumps(r))
        sys.exit(0)
    for name, layers in r.items():
        print(name + (":" if layers else ": no marked section"))
        for layer, secs in sorted(layers.items()):
            for t in secs:
                print(f"  {layer}: {t['mfma']} MFMAs in runs of {t['runs']}, {t['breaks']} breaks inside the stream ({t['branches_in_breaks']} branches, {t['scalar_in_breaks']} scalar instructions in them); in the runs' gaps {t['scalar']} scalar instructions "
                      f"(+ {t['quiet_scalar']} s_waitcnt / s_nop), {t['lane_moves']} lane moves ({t['lane_moves_anywhere']} between the markers); {len(t['piece_gaps'])} piece gaps")
                kinds = {}
                for g in t["piece_gaps"]:
                    kinds.setdefault(" ".join(g["ops"]), []).append(g["line"])
                for k, lines in kinds.items():
                    print(f"      piece gap x {len(lines)} (behind the MFMA of line {lines[0]} ..): {k}")
                print(f"      branches between the first and the last MFMA, by line: {t['branch_lines']}")
