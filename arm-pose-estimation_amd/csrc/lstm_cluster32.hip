// Weight-stationary cluster LSTM kernel, second generation, exact float32 (BASELINE.json configs[2]/[3]: 1024 windows
// x 64 frames per GPU).  Same arithmetic as lstm_cluster.hip / lstm_tile16.hip up to float32 summation order
// (reference estimate/nn_models.py:169-174,180-189: L stacked LSTM layers, gates i,f,g,o, zero initial state, Linear
// head on the last step), restructured around what the first-generation kernel loses (~9 % in the
// instructions between its 16x16x4 MFMAs, ~9 % in exchange work and waits, ~5 % in the gate math):
//
//   * v_mfma_f32_32x32x2_f32 on ONE accumulator tile per wave: 32 gate columns (8 hidden units x i,f,g,o) x 32 windows.
//     Same 64 FLOP/cycle/SIMD as the 16x16x4 form, but half the instructions and half the activation reads per
//     FLOP, and the MFMAs of a layer-step form one dependent chain (64-cycle issue = 64-cycle dependent latency), so the
//     one ds_read_b128 + s_waitcnt per four MFMAs, the scalar bookkeeping and the exchange instructions issue inside the
//     shadow of the running MFMA instead of between two of them.
//   * 8 members per cluster instead of 16: a member owns 32 hidden units of both layers, a wave 8 of them; its slice of
//     [W_ih | W_hh] is 400 registers per lane -- layer 1's 256 in the accumulator file, layer 0's 144 in architectural
//     VGPRs -- resident for the whole launch.  A cluster owns 32 windows, 32 clusters fill the 256 CUs.  Half the peers,
//     half the flags, 32 KB instead of 64 KB gathered per layer-step and member.
//   * column order inside a wave's tile is gate * 8 + unit: with the weights as the A operand, lane (window n = lane & 31,
//     half hh = lane >> 5) then holds the four gates of units 4 hh .. 4 hh + 3 of window n in its sixteen accumulator
//     registers -- the cell update is lane-local, and the four fresh h values ARE one 16-byte piece of the exchange layout
//     [member][wave][window][8 units]: the publish is one store from registers, no staging.
//   * that exchange layout is also the MFMA fragment order of the activation operand (k-block of 8 = one wave's units, a
//     lane reads its window's half row), so gathered slices never pass through registers: a layer-step's 32 KB are copied
//     global -> LDS by 32 LDS-DMA instructions per workgroup (`buffer_load_dwordx4 ... lds`, inline asm, outside the
//     compiler's s_waitcnt bookkeeping), PREFETCHED under the other layer's section: layers are software-pipelined
//     (phase p: layer l works on step p - l), every section reads only what was published at least two sections ago, and
//     the section in front looks at the flags half-way through its MFMAs and starts the copy.
//   * XCD-pure clusters where the dispatcher allows it (membership by arrival ticket within the block-index class
//     blockIdx % 8, the XCD each member really runs on verified at run time): payload by plain stores that stay in the
//     XCD's L2, else sc1 write-through stores; flags always agent-scope stores; loads of handed-off bytes always sc1
//     (MI355X guide G16 / visibility table row 1).  Bounded spins, sticky status word, self-cleaning -- as
//     lstm_cluster_f16v2.hip, whose exchange this is.
//   * split form (end): every product but layer 0's input columns runs on v_mfma_f32_32x32x16_f16 as
//     W_hi h_hi + W_hi h_lo + W_lo h_hi of power-of-two scaled f16 hi / lo pairs (each product exact in the f32 accumulator), 96 cycles
//     per K = 16 instead of 512; weights in the split image of weight_pack.h (pack_c32_split), h exchanged in the split layout.
// Eval mode, last-step output (what the estimators' batched path and the benchmark use); dropout, all-steps output and
// other shapes stay on the first-generation kernels.
#include <type_traits>

#include "ape_internal.h"
#include "async_look.h"
#include "cluster_sync.h"
#include "mfma_stream.h"
#include "../../include/ape_hip.h"

namespace {

// diagnostic builds: timeline of a short launch (cluster 0, member 0, thread 0) in dbg_wg[256 + i] -- 0 entry, 1 rendezvous done, 2 step 0
// of layer 0 and the weights done, 8 + 2 * (2 * ph + l) / + 1: section (ph, l) behind its top barrier / at its end, 4 final gather, 5 head
#ifdef APE_CLUSTER_STAMPS
#define C32_TL(i) do { if (p.dbg_wg != nullptr && tid == 0 && cluster == 0 && member == 0 && (i) < 200) p.dbg_wg[256 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define C32_TL(i) do {} while (0)
#endif

// (mfma_stream.h: sigm / tanh_, mfma32 -- v_mfma_f32_32x32x2_f32 --, mfma_drain and span32, the f32 form of layer 0's input columns)

// v_mfma_f32_32x32x16_f16 on the same accumulator: the recurrent products.  A 32x32x2_f32 in front of it on the same, fully
// overlapping accumulator needs no wait states (SrcC = the previous vDst exactly; hipcc's hazard recognizer pads none for the builtins)
template <bool AG>
__device__ __forceinline__ void mfma32_f16(f32x16& acc, const u32x4& w, const u32x4& b) {
    if constexpr (AG) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
    else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
}

// NS K = 16 slices of h columns in the split form: acc += W_hi h_hi + W_hi h_lo + W_lo h_hi (each f16 x f16 product exact in the f32
// accumulator).  Weights: groups w[g0 + 2 s] (hi) / w[g0 + 2 s + 1] (lo) in the A-fragment order (weight_pack.h, pack_c32_split).
// Activations: the split exchange layout [block of 8 units][hi, lo][window 32][8 units as f16] (1 KiB per block); slice s = blocks
// 2 s, 2 s + 1, lane (n, hh) reads block 2 s + hh -- `src` = this lane's hi fragment of slice 0, hi / lo one ds_read_b128 each
// (conflict-free: 16 consecutive windows per lane group), fetched two slices ahead.  `mid(q)` runs with q = 2 s behind the second
// MFMA of slice s and q = 2 s + 1 behind the third: the k-block numbering of the f32 form (one slice = two blocks of 8).
template <int NS, bool AG, int NG, typename Mid>
__device__ __forceinline__ void span32_f16(f32x16& acc, const float* __restrict__ src, const u32x4 (&w)[NG], int g0, Mid&& mid) {
    constexpr int SL = 2 * 2 * 32 * 4;      // floats per slice (two blocks)
    u32x4 h0 = *reinterpret_cast<const u32x4*>(src), l0 = *reinterpret_cast<const u32x4*>(src + 128);
    u32x4 h1 = (NS > 1) ? *reinterpret_cast<const u32x4*>(src + SL) : h0, l1 = (NS > 1) ? *reinterpret_cast<const u32x4*>(src + SL + 128) : l0;
    u32x4 h2 = h1, l2 = l1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + 2 < NS) {
            h2 = *reinterpret_cast<const u32x4*>(src + SL * (s + 2));
            l2 = *reinterpret_cast<const u32x4*>(src + SL * (s + 2) + 128);
        }
        mfma32_f16<AG>(acc, w[g0 + 2 * s], h0);
        mfma32_f16<AG>(acc, w[g0 + 2 * s], l0);
        mid(2 * s);
        mfma32_f16<AG>(acc, w[g0 + 2 * s + 1], h0);
        mid(2 * s + 1);
        h0 = h1; l0 = l1;
        h1 = h2; l1 = l2;
    }
}

// one LDS-DMA wave-instruction: 64 lanes x 16 bytes from the buffer (lane offset `voff`, uniform `soff`) to 1 KiB of LDS at
// the wave-uniform byte address `lds_addr`; sc1 = L1-bypassing, like every load of handed-off bytes.  M0 is written in the
// same statement that reads it (the compiler does not preserve it across statements).
// HOT = inside a section's MFMA stream, where every scalar instruction between two MFMAs is paid for (round 4, 1024 x 64: `s_nop 3`
// instead of `s_nop 0` in the eight copies of a section +4.7 us per launch, one more s_add per copy +5.8 us): there `soff` comes straight
// from scalar arithmetic.  The copies of the blocking forms (pipeline fill, final gather) are not in anybody's way, and there hipcc does
// reload `soff` from a spill lane (v_readlane_b32) right in front of the statement -- a VALU write of an SGPR needs five wait states
// before a vector-memory instruction reads it, and hipcc does not look inside an asm statement.  tools/check_mfma_hazards.py scans
// the build for exactly that adjacency, so a reload that turns up in front of a HOT copy fails the build.
// The HOT form therefore takes the two addresses WITHOUT the piece's offset and adds it as an immediate inside the statement: no
// per-piece sums for hipcc to hoist out of the phase loop (with three more section forms in round 4 they no longer fitted the scalar
// registers), two SALU instructions per copy, and the second s_add is the wait state the M0 write needs in front of the LDS-DMA.
template <bool HOT>
__device__ __forceinline__ void dma_1k(unsigned lds_addr, unsigned voff, u32x4 rsrc, unsigned soff, int piece_bytes) {
    if constexpr (HOT) {
        unsigned tmp;
        asm volatile("s_add_i32 m0, %1, %5\n\ts_add_i32 %0, %4, %5\n\tbuffer_load_dwordx4 %2, %3, %0 offen sc1 lds"
                     : "=&s"(tmp) : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff), "i"(piece_bytes) : "memory", "scc");
        // ("scc": s_add_i32 writes it.  As long as every piece sat behind a branch of its own hipcc never held a condition in SCC across one; with the
        //  branches gone it kept layer 1's own judge there, from the head of the input span to the branch behind it -- the eight pieces in between
        //  cleared it, and every section took the blocking refill: same results, 4 % slower; tests/tools/counts_c32.py showed 60 of 60)
    } else {
        ::dma_1k(lds_addr + (unsigned)piece_bytes, voff, rsrc, soff + (unsigned)piece_bytes);     // (async_look.h: the `s_nop 3` form)
    }
}

// A flag look that does NOT stall the MFMA stream: hipcc hoists the comparison of a compiler-visible load up to the load and puts
// `s_waitcnt vmcnt(0)` right behind it -- an L2 round trip exposed in every section (found in round 3 in the disassembly of this
// kernel as round 2 shipped it).  The look is issued as LDS-DMA into the wave's landing zone (async_look.h: no destination register;
// rounds 3-4 had one, and round 5 found what hipcc may do to it), read back from LDS one k-block in front of the judge.

// ENDS: the forms for the ends of a launch (step 0 of layer 0 in front of the bulk of the weights, MODE 1 / MODE 2 sections, see there) --
// the instantiation for SHORT windows (T <= APE_C32_ENDS_MAX_T; every deployed model has T = 6 or 8).  The timeline stamps
// (tests/tools/timeline_c32.py) show what they do at T = 6: layer 0's second step starts 1.5 us behind the weights instead of a whole
// exchange behind them, layer 0's third step and layer 1's last one find their slices in LDS (top waits 0.2-0.3 us).  Same-box A/B,
// 1024 x 6: 83.8 -> 82.3 us (best blocks; 87.2 -> 85.6 medians).  But with these forms in the kernel hipcc's code for the steady-state
// sections comes out ~0.3-1 % slower per phase (register allocation / layout: 12.24 vs 12.27 us per phase; 1024 x 32: 402 -> 406 us; 1024 x 12: no difference left), so
// longer windows keep the instantiation without them.
// hook positions of a steady-state section (k-block indices; see `mid` in the kernel): QF = where the flag owed for the section in front's publish
// store goes up, QPD = shift of the look / judge / gather positions from the middle of the section
#ifndef C32_QF
#define C32_QF 3
#endif
#ifndef C32_QPD
#define C32_QPD 0
#endif
// long windows, steady state (the sections that carry layer 0's input span of the next step, `XS` in the kernel): C32_QFP = blocks into a layer-0
// section's recurrent span at which the flag owed for layer 1's publish store goes up; C32_QPX / C32_QJX = layer 1's look at the next section's
// flags and its judge; C32_XS = 0 builds those sections without the relocated span, for A/B runs
// (swept on MI355X, 1024 x 64, profiles/r09_cluster32_xspan.md: the look BEHIND the x staging of block 33 -- hipcc's own `vmcnt` waits in front of
//  the staging otherwise sit out the look's round trip -- and its judge a round trip, 21 blocks, further on)
#ifndef C32_XS
#define C32_XS 1
#endif
#ifndef C32_QFP
#define C32_QFP 12
#endif
#ifndef C32_QPX
#define C32_QPX 33
#endif
#ifndef C32_QJX
#define C32_QJX 54
#endif
// the hot gaps of the long-window steady-state sections (profiles/r10_cluster32_hot_gaps.md; each switch 0 = the form in front of it, for A/B runs):
// C32_UG = the eight pieces of both gathers go out without a branch, from a source base derived once per section (see `UG` in the kernel for why
// a copy nobody asked for harms nobody); C32_RS = the flag owed goes up as one buffer store through the looks' descriptor
#ifndef C32_UG
#define C32_UG 1
#endif
#ifndef C32_RS
#define C32_RS 1
#endif
// test builds only (lib/diag/libape_hip_c32late.so): the judges of both gathers read "not yet" in every N-th steady-state phase, whatever the flags say --
// the path of a late peer (0.05-2 sections per 1024 x 64 launch: never in a small test), which ends in the bounded blocking refill
#ifndef APE_C32_LATE_EVERY
#define APE_C32_LATE_EVERY 0
#endif
#if defined(APE_C32_COUNTS) && defined(APE_C32_WAITS)
#error "APE_C32_COUNTS and APE_C32_WAITS write the same words of dbg_wg: one build, one of them"
#endif
template <int H, int L, int KX, bool ENDS, int BXU>
__global__ __launch_bounds__(256, 1) void ape_lstm_cluster32(const ClusterParams p) {
    constexpr int UPW = 8;                  // hidden units per wave (x 4 gates = the 32 columns of its tile)
    constexpr int GH = H / (4 * UPW);       // members per cluster
    constexpr int MR = 32;                  // windows per cluster (one 32-row tile)
    constexpr int SX = KX + 4;              // LDS row stride of the x slab (floats): conflict-free ds_read_b128 (rows 36 dwords apart)
    constexpr int BX = KX / 8, BH = H / 8;  // k-blocks of 8
    constexpr int NW0 = 4 * (BX + BH);      // weight registers per lane, layer 0 (architectural VGPRs)
    constexpr int NW1 = 4 * (2 * BH);       //                            layer 1 (accumulator file)
    constexpr int NFL = 4 * GH;             // flags per (cluster, layer): one per member wave
    constexpr int HL = GH * 4 * MR * 8;     // floats of one gathered slice set [member][wave][window][8 units] = 32 KB
    constexpr int NDMA = HL * 4 / 1024 / 4; // LDS-DMA instructions per wave and gather
    static_assert(H == 256 && L == 2 && KX == 32 && GH == 8 && NDMA == 8, "built for the 2 x 256 models");
    // BXU: k-blocks of the x slab that layer 0's input span really multiplies -- ceil(I / 8) of the BX staged ones (the launcher's choice; columns
    // I .. KX - 1 are zeros, a block of them adds +0.0 to every sum; the staging layout and the weight image stay those of KX = 32)
    static_assert(BXU == BX || (BXU == BX - 1 && !ENDS), "the short-window instantiation keeps the four-block input span");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, hh = lane >> 5;     // window of the tile, half (units 4 hh .. 4 hh + 3 of the wave's 8)
    const int T = p.T, I = p.I, O = p.O;
    const bool normalize = (p.flags & APE_FLAG_NORMALIZE_INPUT) != 0;
    const bool bcast_x = (p.flags & APE_FLAG_BROADCAST_X) != 0;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* hb0 = smem;                      // [2 parity][HL]  h of layer 0, step parity (read by layer 0's recurrence AND layer 1's input)
    float* hb1 = hb0 + 2 * HL;              // [HL]           h of layer 1
    float* xin = hb1 + HL;                  // [2 parity][MR][SX]  x of a step, by step parity in the long-window instantiations (ENDS: buffer 0 only)
    f32x4* bias_s = reinterpret_cast<f32x4*>(xin + 2 * MR * SX); // [wave 4][L][4 gates][lane 64]: the accumulators' start values
    f32x4* park_s = bias_s + 4 * L * 4 * 64;                     // [wave 4][4 gates][lane 64]: layer 0's sums behind the input span of the NEXT step (thread-private)
    unsigned* look_s = reinterpret_cast<unsigned*>(park_s + 4 * 4 * 64);       // [wave 4][64]: landing zones of the flag looks (async_look.h)
    int* ctl = reinterpret_cast<int*>(look_s + 4 * 64);          // [0] abort, [1] class ticket, [2] last-out, [3] same XCD

    // control words (all zero between launches): [8 class tickets, one per 64-byte line][n_wg XCD words]
    unsigned* const class_ticket = p.xcc_slots + 64;
    unsigned* const xcc_words = p.xcc_slots + 64 + 8 * 16;
    const int cls = blockIdx.x & 7;
    const unsigned my_xcc = ape_xcc_id();
    const int drawn = ape_take_class_ticket(ctl, p.status, class_ticket, cls, tid);
    if (drawn < 0) return;
    const int ticket = __builtin_amdgcn_readfirstlane(drawn);
    const int cluster = (ticket / GH) * 8 + cls, member = ticket % GH;
    const int row0 = cluster * MR;
    C32_TL(0);
    if (tid == 0)
        __hip_atomic_store(xcc_words + cluster * GH + member, 0x10u | my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // ---- x: the first step's loads go out in front of the weights (loads return in order) -----------------------------
    constexpr int NE = (MR * KX) / 256;     // (window, k) elements of the step slab per thread, all with the same k
    const int xk = tid % KX, xrow = tid / KX;
    const int rows_here = bcast_x ? MR : max(0, min(MR, p.B - row0));
    // (descriptor words forced into scalar registers: in vector registers every load becomes a readfirstlane waterfall loop)
    const unsigned long long x_addr = reinterpret_cast<unsigned long long>(p.x + (bcast_x ? (size_t)0 : (size_t)row0 * T * I));
    const unsigned x_lo = __builtin_amdgcn_readfirstlane((unsigned)x_addr), x_hi = __builtin_amdgcn_readfirstlane((unsigned)(x_addr >> 32));
    const int x_bytes = __builtin_amdgcn_readfirstlane((int)((size_t)(bcast_x ? 1 : rows_here) * T * I * sizeof(float)));
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<float*>(((unsigned long long)x_hi << 32) | x_lo), 0, x_bytes, 0x00020000);
    const unsigned x_rowbytes = bcast_x ? 0u : (unsigned)(T * I * sizeof(float));
    // rows past the batch and the padded columns k >= I lie outside the descriptor and read as 0 (no predicates)
    const unsigned x_off0 = (xk < I) ? (unsigned)xrow * x_rowbytes + (unsigned)(xk * sizeof(float)) : 0x80000000u;
    const unsigned x_estride = (unsigned)(256 / KX) * x_rowbytes;
    float xr[NE];
    auto fetch_x = [&](int t) {
        const int slot = (t + p.x_ring >= T) ? t + p.x_ring - T : t + p.x_ring;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const unsigned off = (xrow + e * (256 / KX) < rows_here) ? x_off0 + (unsigned)e * x_estride : 0x80000000u;
            xr[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rsrc, off, (unsigned)(slot * I * sizeof(float)), 0));
        }
    };
    // f64 z-score, cast f32 (estimator.py:103-104, watch_phone_pocket_nn.py:100): (x - m) / s correctly rounded via the
    // host-rounded reciprocal and one residual step (bit-identical to the division, as in lstm_cluster.hip)
    double x_mean = (normalize && xk < I) ? p.xx_m[xk] : 0.0;
    double x_std = (normalize && xk < I) ? p.xx_s[xk] : 1.0;
    double x_rstd = (normalize && xk < I) ? p.xx_r[xk] : 1.0;
    // (opaque from here on: with more section forms in the kernel hipcc preferred to RE-LOAD the three constants inside the staging hook
    //  of every layer-1 section -- a global-memory round trip in the MFMA stream, 450 -> 950 cycles per section by the stamps)
    asm volatile("" : "+v"(x_mean), "+v"(x_std), "+v"(x_rstd));
    // (the fetched step goes to the buffer of its parity `t`; ENDS: always buffer 0)
    auto stage_x = [&](int t) {
        float* const dst = xin + (ENDS ? 0 : (t & 1) * (MR * SX));
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double d = (double)xr[e] - x_mean;
            const double q0 = d * x_rstd;
            const double rr = fma(-q0, x_std, d);
            const double q1 = fma(rr, x_rstd, q0);
            dst[(xrow + e * (256 / KX)) * SX + xk] = (float)((rr == rr) ? q1 : q0);
        }
    };
    // XA: how many steps further ahead than the short-window instantiation x is staged.  Long windows: a phase stages x of step ph + 2 and
    // fetches step ph + 3, because a steady-state layer-1 section runs layer 0's input span of the NEXT step (below); the prologue stages steps 0 and 1.
    constexpr int XA = ENDS ? 0 : 1;
    fetch_x(0);

    // ---- weights: registers, for the whole launch.  Host layout [member][wave][register / 4][lane][4]: register 4 kb + j of
    //      lane (column m = lane & 31, half hh) = W[gate(m) * H + unit(m)][8 kb + 4 hh + j] with m = gate * 8 + local unit
    //      Only layer 0's input columns (16 registers) are loaded here: step 0 of layer 0 needs nothing else (h_{-1} = 0), and its hand-over
    //      then travels while the other 384 registers come in (`load_weights`, called behind it).
    //      The image is the split one (pack_c32_split): layer 0's input columns as above times 2^S, every recurrent / layer-1 column as
    //      K = 16 slices of f16 hi / lo A fragments, two groups of four registers each -- the same 400 registers.
    float w0[4 * BXU];
    u32x4 w0h[NW0 / 4 - BX];
    u32x4 w1[NW1 / 4];
    const f32x4* const s0 = reinterpret_cast<const f32x4*>(p.wcl[0]) + ((size_t)(member * 4 + wave) * (NW0 / 4)) * 64 + lane;
    const u32x4* const s1 = reinterpret_cast<const u32x4*>(p.wcl[1]) + ((size_t)(member * 4 + wave) * (NW1 / 4)) * 64 + lane;
#pragma unroll
    for (int i = 0; i < BXU; ++i) {
        const f32x4 v = s0[i * 64];
        w0[4 * i] = v[0]; w0[4 * i + 1] = v[1]; w0[4 * i + 2] = v[2]; w0[4 * i + 3] = v[3];
    }
    auto load_weights = [&]() {
#pragma unroll
        for (int i = BX; i < NW0 / 4; ++i) w0h[i - BX] = reinterpret_cast<const u32x4*>(s0)[i * 64];
#pragma unroll
        for (int i = 0; i < NW1 / 4; ++i) w1[i] = s1[i * 64];
    };
    // accumulator start values (b_ih + b_hh) of this lane: registers 4 gate + j <-> unit member*32 + wave*8 + 4 hh + j; in LDS,
    // not in 32 more registers
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) {
            f32x4 bv;
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = p.bias[l][gate * H + member * 32 + wave * 8 + 4 * hh + j] * p.gate_scale[l];   // (exact: 2^S)
            bias_s[((wave * L + l) * 4 + gate) * 64 + lane] = bv;
        }
    float cst[L][4];
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) cst[l][j] = 0.0f;

    // exchange buffer: descriptor for the compiler's stores, and the same words as a scalar tuple for the DMA asm
    const __amdgpu_buffer_rsrc_t hx_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.hx, 0, (int)p.hx_bytes, 0x00020000);
    const u32x4 hx_desc = ape_make_desc(p.hx, (unsigned)p.hx_bytes);
    unsigned* const flags_of = p.xflags + (size_t)cluster * L * NFL;       // [layer][member*4 + wave] epoch = steps published
    // the looks at those flags (async_look.h): descriptor over the flag words, this cluster's byte offset, the lane's flag, the wave's zone
    const ape_desc_t fl_desc = ape_make_desc(p.xflags, (unsigned)((gridDim.x / GH) * L * NFL * sizeof(unsigned)));
    const unsigned fl_off = (unsigned)(cluster * L * NFL * sizeof(unsigned));
    const unsigned look_voff = (unsigned)((lane & (NFL - 1)) * sizeof(unsigned));
    const unsigned look_lds = (unsigned)reinterpret_cast<unsigned long long>(look_s) + (unsigned)(wave * 256);
    const unsigned* const look_mine = look_s + wave * 64 + lane;
    constexpr unsigned SET_BYTES = HL * sizeof(float);                     // one (layer, parity)
    auto hx_base = [&](int l, int par) -> unsigned { return (unsigned)((((size_t)cluster * L + l) * 2 + par) * SET_BYTES); };
    const unsigned hb0_lds = (unsigned)reinterpret_cast<unsigned long long>(hb0);     // LDS byte addresses
    const unsigned hb1_lds = (unsigned)reinterpret_cast<unsigned long long>(hb1);

    stage_x(0);
    if (T > 1) fetch_x(1);

    // ---- do all members of this cluster really share an XCD? ------------------------------------------------------
    if (wave == 0) ape_same_xcd<GH, 2, APE_ABORT_SPIN>(xcc_words, cluster, my_xcc, p.status, ctl, lane);
    __syncthreads();
    if (ctl[0] != 0) return;
    C32_TL(1);
        // hand-over form (ape_internal.h): write-through (`sc1`) payload stores unless the caller opted into the plain in-XCD form AND the
    // members were verified to share an XCD; uniform over the cluster
    const bool in_l2 = APE_HANDOVER_IN_L2(p.flags, ctl[3] != 0);

    // every wave polls for itself: have all member waves published epoch `want` of layer l?
    auto wait_flags = [&](int l, unsigned want) { ape_wait_words<NFL, 1, 1>(flags_of, l, want, p.status, ctl, lane); };
    // a layer-step's 32 KB straight from the exchange buffer into its LDS block: wave w copies KiB w, w + 4, ... (8 of them);
    // piece k of that copy on its own, so that the copy can be spread over the k-blocks of a span
    const unsigned dma_voff = (unsigned)(lane * 16);
    // (blocking forms: the per-wave offset is laundered through an empty asm at every use, or hipcc hoists the sums of all pieces of all
    //  section forms out of the loop and runs out of scalar registers -- lstm_upper32.hip)
    const unsigned wave_kib = (unsigned)(wave * 1024);
    auto issue_piece = [&](auto hot_tag, int l, int step, int k) {       // slices of layer l, step `step` -> hb0[step parity] / hb1
        constexpr bool HOT = decltype(hot_tag)::value;
        const unsigned wk = HOT ? wave_kib : opaque(wave_kib);
        // (long windows, blocking forms: the set's base opaque as well -- hipcc otherwise keeps `base | piece offset` of all eight pieces in scalars
        //  for the whole launch, and the steady-state sections then reload one of THEIR scalars from a spill lane in the middle of the MFMA stream)
        const unsigned src = ((HOT || ENDS) ? hx_base(l, step & 1) : opaque(hx_base(l, step & 1))) + wk;
        const unsigned dst = (l == 0 ? hb0_lds + (unsigned)((step & 1) * SET_BYTES) : hb1_lds) + wk;
        dma_1k<HOT>(dst, dma_voff, hx_desc, src, k * 4096);
    };
    constexpr std::true_type HOT{};
    constexpr std::false_type COLD{};
    // the flag a wave owes for the slice it stored last: raised once that store has drained
    // (EV, long windows with C32_RS: the epoch lives in a vector register from the publish on, for raise_hot() below, and NOT in a scalar beside it --
    //  the steady-state sections have no scalar register to spare)
    constexpr bool EV = !ENDS && C32_XS != 0 && C32_RS != 0;
    int pend_idx = -1;
    unsigned pend_epoch = 0u, pend_epoch_v = 0u;
    auto raise_pending = [&]() {              // caller has waited vmcnt(0)
        if (pend_idx < 0) return;
        if (lane == 0) __hip_atomic_store(flags_of + pend_idx, EV ? pend_epoch_v : pend_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pend_idx = -1;
    };
    // The same for the hooks of the long-window steady-state sections (C32_RS), where the flag owed is always the OTHER layer's (`lo`) and always
    // this wave's: ONE buffer store through the looks' descriptor, no branch, no 64-bit address.  Lane 0 stores at its flag's offset inside a
    // layer's row, every other lane points outside the descriptor (the 0x80000000 idiom of the x rows and the idle publishes: dropped by the
    // range check); `sc1` = the agent-scope store of raise_pending().  The epoch waits in a vector register since the publish (pend_epoch_v).
    // A wave that came through a blocking path has raised the flag already and stores the same epoch once more -- the word's only writer is this wave.
    const unsigned raise_voff = (lane == 0) ? (unsigned)((member * 4 + wave) * sizeof(unsigned)) : 0x80000000u;
    // (the layer's row as the instruction's immediate offset: one scalar, the cluster's `fl_off`, serves both layers)
    auto raise_hot = [&](auto lo_tag) {       // caller has waited vmcnt(0)
        constexpr int lo = decltype(lo_tag)::value;
        asm volatile("buffer_store_dword %0, %1, %2, %3 offen offset:%4 sc1"
                     :: "v"(pend_epoch_v), "v"(raise_voff), "s"(fl_desc), "s"(fl_off), "i"(lo * NFL * (int)sizeof(unsigned)) : "memory");
        pend_idx = -1;
    };
    auto bar = [&]() { ape_bar_lds(); };

    // ---- gates + cell update, lane-local: registers 4 gate + j = gate of unit 4 hh + j, window n ---------------------------
    // (two cells at a time, the plain arithmetic on float2 values: v_pk_mul / v_pk_add / v_pk_fma_f32 do both cells in one issue
    //  slot -- VALU work is serial with the MFMAs, tools/experiments/mfma_chain_rate.hip; the transcendentals stay one by one)
    // (the accumulators hold 2^S times the pre-activations: 2^-S sits in the gate constants, a product with a power of two, exact --
    //  the gate values are those of the unscaled sums)
    auto cell_update = [&](const f32x16& acc, int l, float (&c_)[4], float (&hn)[4]) {
        const float ks = -1.4426950408889634f * p.gate_descale[l], kt = -2.885390081777927f * p.gate_descale[l];
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            auto exp2_2 = [](f32x2 v) { return f32x2{__builtin_amdgcn_exp2f(v[0]), __builtin_amdgcn_exp2f(v[1])}; };
            auto rcp_2 = [](f32x2 v) { return f32x2{__builtin_amdgcn_rcpf(v[0]), __builtin_amdgcn_rcpf(v[1])}; };
            const f32x2 ai = {acc[j], acc[j + 1]}, af = {acc[4 + j], acc[5 + j]}, ag = {acc[8 + j], acc[9 + j]}, ao = {acc[12 + j], acc[13 + j]};
            const f32x2 iv = rcp_2(1.0f + exp2_2(ks * ai));
            const f32x2 fv = rcp_2(1.0f + exp2_2(ks * af));
            const f32x2 gv = 2.0f * rcp_2(1.0f + exp2_2(kt * ag)) - 1.0f;
            const f32x2 ov = rcp_2(1.0f + exp2_2(ks * ao));
            const f32x2 c = fv * f32x2{c_[j], c_[j + 1]} + iv * gv;
            c_[j] = c[0]; c_[j + 1] = c[1];
            const f32x2 h = ov * (2.0f * rcp_2(1.0f + exp2_2(-2.885390081777927f * c)) - 1.0f);
            hn[j] = h[0]; hn[j + 1] = h[1];
        }
    };
    const unsigned pub_off = (unsigned)((((member * 4 + wave) * MR + n) * 8 + 4 * hh) * sizeof(float));    // this lane's 16 bytes of a slice set
    // The split exchange layout (what span32_f16 reads): per block of 8 units [hi, lo][window][8 units as f16].  A lane's four fresh h
    // (units 4 hh .. 4 hh + 3) become f16 hi / lo of h * 2^APE_C32_HSHIFT (exact scaling; |h| <= 1), two dwords each; one
    // v_permlane32_swap per dword pair gives lanes 0-31 the hi of all eight units [own | upper's] and lanes 32-63 the lo [lower's | own]:
    // one 16-byte store per lane, at window n of the hi (hh = 0) / lo (hh = 1) half.
    // The LAST step of the top layer is read only by the head and is published as f32 at pub_off (the f32 layout [window][8 units]).
    const unsigned pub_off_split = (unsigned)(((member * 4 + wave) * 2 * MR + hh * MR + n) * 16);
    auto split_h = [&](const float (&h)[4]) -> u32x4 {
        unsigned hw[2], lw[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const float a = h[2 * d] * (float)(1 << APE_C32_HSHIFT), b = h[2 * d + 1] * (float)(1 << APE_C32_HSHIFT);
            const _Float16 ah = (_Float16)a, bh = (_Float16)b;
            const _Float16 al = (_Float16)(a - (float)ah), bl = (_Float16)(b - (float)bh);
            hw[d] = (unsigned)__builtin_bit_cast(unsigned short, ah) | ((unsigned)__builtin_bit_cast(unsigned short, bh) << 16);
            lw[d] = (unsigned)__builtin_bit_cast(unsigned short, al) | ((unsigned)__builtin_bit_cast(unsigned short, bl) << 16);
        }
        u32x4 r;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const auto sw = __builtin_amdgcn_permlane32_swap(hw[d], lw[d], false, false);
            r[d] = sw[0];
            r[2 + d] = sw[1];
        }
        return r;
    };

    // ---- step 0 of layer 0 IN FRONT of the bulk of the weights: its product is the input span alone (4 k-blocks, 16 weight registers),
    //      and its hand-over -- store, acknowledgement, flag, the peers' flags -- would otherwise be the first thing the launch waits
    //      for with nothing to do (round 4: ~3 us of the 89 us launch at T = 6).  Phase 0's layer-1 section is idle anyway; the loop
    //      below starts at phase 1.
    if constexpr (!ENDS) {
        // (x_1, whose loads went out in front of the rendezvous above, into its own buffer; its first reader sits behind phase 0's barriers)
        if (1 < T) {
            stage_x(1);
            if (2 < T) fetch_x(2);
        }
        load_weights();
    } else {
        f32x16 acc;
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) {
            const f32x4 bv = bias_s[((wave * L + 0) * 4 + gate) * 64 + lane];
            acc[4 * gate] = bv[0]; acc[4 * gate + 1] = bv[1]; acc[4 * gate + 2] = bv[2]; acc[4 * gate + 3] = bv[3];
        }
        span32<BXU, false, 4 * BXU>(acc, xin + n * SX + hh * 4, 8, w0, 0, [&](int) {});
        mfma_drain(acc);
        float h0[4];
        cell_update(acc, 0, cst[0], h0);
        const u32x4 hv = split_h(h0);
        if (in_l2) __builtin_amdgcn_raw_buffer_store_b128(hv, hx_rsrc, hx_base(0, 0) + pub_off_split, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b128(hv, hx_rsrc, hx_base(0, 0) + pub_off_split, 0, 16 /* sc1: write-through */);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(flags_of + member * 4 + wave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::: "memory");
        load_weights();
        bar();                                                    // every wave is through with x_0 in LDS
        if (1 < T) {
            stage_x(1);
            if (2 < T) fetch_x(2);
        }
    }
    C32_TL(2);

    // Section (ph, l) = layer l on step t = ph - l.  It reads x_t / h^{l-1}_t and h^l_{t-1}, all published in phase ph - 1,
    // i.e. at least two sections ago; the ONE slice set it is still missing in LDS -- layer 0: h^0_{t-1} (published by the
    // last layer-0 section), layer 1: h^1_{t-1} (by the last layer-1 section) -- is prefetched by the section in front.
    // Per wave the vector-memory queue of a steady-state section is, in issue order:
    //   [publish store of the section in front]  flag look (1 load)  [x fetch, layer 1 only]  gather DMA for the NEXT section (8)
    //   publish store (1)
    // so at the top of a section everything but the youngest entry is waited for (`vmcnt(1)`: the slices are in LDS); behind the
    // barrier the store itself is waited for and its flag goes up.
    const int P = T + L - 1;                 // phases 0 .. P-1 compute; "phase" P: the final gather for the head
    bool prefetched = false;
    // the layer-1 section in front has run layer 0's input span for this step and parked the sixteen sums in park_s (long windows, steady state)
    bool parked = false;
#ifdef APE_C32_COUNTS
    // light counters of a product-like build (tests/tools/counts_c32.py): per workgroup (wave 0), per layer -- sections whose gather took the
    // blocking form / was prefetched, shader clocks between a section's entry and the exit of its top barrier
    unsigned lc_block[2] = {0u, 0u}, lc_go[2] = {0u, 0u}, lc_n[2] = {0u, 0u};
    unsigned long long lc_top[2] = {0ull, 0ull}, lc_t0 = 0ull;
    const unsigned long long lc_start = __builtin_amdgcn_s_memtime();
#endif
#ifdef APE_C32_WAITS
    // a switch of its own (tests/tools/waits_c32.py; the record takes the place of APE_C32_COUNTS' in dbg_wg, so not both): shader clocks wave 0
    // spends in the waits of a steady-state phase, s_memtime around the wait only -- [0] layer 1's `look_landed()` for the own look, [1] the
    // same for the next section's look, [2] layer 1's wait + barrier between the spans, [3] layer 0's entry -> behind the top barrier;
    // lw_n: steady-state layer-1 / layer-0 sections, layer-1 sections whose own gather took the blocking form
    unsigned long long lw[4] = {0ull, 0ull, 0ull, 0ull}, lw_t0 = 0ull;
    unsigned lw_n[3] = {0u, 0u, 0u};
    const unsigned long long lw_start = __builtin_amdgcn_s_memtime();
#define C32_WAIT_T0() do { if (ST) lw_t0 = __builtin_amdgcn_s_memtime(); } while (0)
#define C32_WAIT_T1(k) do { if (ST) lw[k] += __builtin_amdgcn_s_memtime() - lw_t0; } while (0)
#else
#define C32_WAIT_T0() do {} while (0)
#define C32_WAIT_T1(k) do {} while (0)
#endif
#ifdef APE_CLUSTER_STAMPS
    unsigned long long dg_block[2] = {0, 0}, dg_go[2] = {0, 0};      // diagnostic counters per layer (cluster 0, member 0)
    unsigned long long dgh[2][6] = {};       // ... and inside the spans: store drain + flag, x staging, judge, gather issue, (unused), eight hook-free blocks
    unsigned long long dgc[2][5] = {};       // steady-state sections: cycles in the top wait, the barrier, the MFMA spans, everything behind the barrier; count
    auto now = [&]() -> unsigned long long {
        const unsigned long long c = __builtin_readcyclecounter();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        return c;
    };
#endif
    // Two forms for the ends of a launch, where a section has no section in front whose MFMA stream could carry its exchange (round 4:
    // at the deployed T = 6 four of the launch's exchanges were exposed, ~3 us each of an 89 us launch):
    //   MODE 1  layer 1 on step 0 runs its input span alone (h_{-1} = 0): 32 k-blocks, so the look at the next section's flags and
    //           its gather sit at blocks 16 / 20 .. 27 instead of 30 / 34 .. 41, which it never reaches;
    // and ONE form for every layer-1 section with a recurrent span (round 5; round 4 had it for the last step of a short window only):
    //   MODE 3  layer 1 on step t >= 1 gathers its OWN missing slice set h^1_{t-1} under its input span: that span reads h^0_t, in LDS since
    //           the layer-0 section in front, so the section starts without a wait and WITHOUT a barrier; the look at the own layer's flags
    //           sits at block QF + 1 -- a whole layer-0 section (>= 4 us) behind the publish, where round 4's look from inside that
    //           layer-0 section came 1.4 us behind the flag and, with write-through stores, found it down in one section of ten
    //           (6.5 blocking gathers per 1024 x 64 launch and member against 1.0 with plain stores; tests/tools/counts_c32.py) --
    //           the eight pieces follow it, and the wait for them and the section's ONE barrier sit between the spans
    //           (lstm_cluster16.hip's place for it): 16+ k-blocks for the copies to land in instead of 8.  x staging moves behind that
    //           barrier; layer-0 sections no longer carry a look or a gather.  Outside the steady state (the last step of a short
    //           window sits behind an idle, i.e. empty, layer-0 section) a second look follows at block QF + 13; a wave whose looks
    //           failed blocks in front of the barrier.
    // and, in the long-window instantiations, ONE more form of the steady-state MODE 3 section (`XS` below; DESIGN.md 4.10, end):
    //   the section starts with the look at its own layer's flags and, under that look's round trip, layer 0's INPUT span of the next step
    //   (x W_ih: the one product of a phase that waits for no hand-over); the sums are parked in LDS, the layer-0 section behind starts from
    //   them and goes straight into its recurrent span.  One `vmcnt(0)` behind the relocated span serves the flag owed for layer 0's publish
    //   store and the judge of the own look; the own gather's eight pieces go out in blocks 0 .. 7 of the input span.  x is staged one step
    //   further ahead than in the other forms, in two buffers by step parity.
    auto section = [&](auto steady_tag, auto layer_tag, auto mode_tag, const int ph) -> bool {
        constexpr bool ST = decltype(steady_tag)::value;          // steady state: 1 <= t <= T - 2 for both layers
        constexpr int l = decltype(layer_tag)::value;
        constexpr int MODE = decltype(mode_tag)::value;
        static_assert(MODE == 0 || (l == L - 1 && (MODE == 3 || !ST)), "the special forms are layer 1's");
        const int t = ph - l;
        // (a comment line in the device assembly, no instruction: tools/tally_c32_gaps.py counts what stands between the MFMAs of the long-window
        //  steady-state sections, from this line to the matching one in front of the drain)
        if constexpr (ST && !ENDS) asm volatile("; c32 steady section, layer %0: begin" :: "i"(l));
        const bool active = ST || (t >= 0 && t < T);
        // h^l_{t-1} exists and somebody reads it from here on (layer 0 at t == T: no layer-0 step any more, but layer 1's
        // last step takes h^0_{T-1} as its input)
        const bool need = ST || (t >= 1 && t <= T);
#ifdef APE_CLUSTER_STAMPS
        const unsigned long long c0 = ST ? now() : 0ull;
#endif
#ifdef APE_C32_COUNTS
        lc_t0 = __builtin_amdgcn_s_memtime();
#endif
        if constexpr (MODE != 3) C32_WAIT_T0();
        // ---- S0: this layer's slices of its last step into LDS ------------------------------------------------------------
        if (MODE == 3) {                                          // (the slices come in under the input span: nothing to wait for here)
        } else if (need) {
            if (!prefetched) {                                    // pipeline fill, a late peer, the final gather
#ifdef APE_CLUSTER_STAMPS
                dg_block[l] += 1;
#endif
#ifdef APE_C32_COUNTS
                lc_block[l] += 1u;
#endif
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                raise_pending();
                wait_flags(l, (unsigned)t);
#pragma unroll
                for (int k = 0; k < NDMA; ++k) issue_piece(COLD, l, t - 1, k);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // the prefetched copy; only the publish store is younger
            }
        }
        prefetched = false;
#ifdef APE_CLUSTER_STAMPS
        const unsigned long long c1 = ST ? now() : 0ull;
#endif
        if constexpr (MODE != 3) bar();
#ifdef APE_CLUSTER_STAMPS
        const unsigned long long c2 = ST ? now() : 0ull;
#endif
#ifdef APE_C32_COUNTS
        if (ST && MODE != 3) { lc_top[l] += __builtin_amdgcn_s_memtime() - lc_t0; lc_n[l] += 1u; }
#endif
#ifdef APE_C32_WAITS
        if constexpr (MODE != 3) { C32_WAIT_T1(3); if (ST) lw_n[1] += 1u; }
#endif
        const int abort_word = (MODE == 3) ? 0 : ctl[0];          // (MODE 3 looks behind its own barrier, between the spans)
        C32_TL(8 + 2 * (2 * ph + l));
        // the next section: layer ln on step tn = its phase - ln; the slice set it is missing is h^{ln}_{tn-1}, epoch tn
        constexpr int ln = (l + 1 < L) ? l + 1 : 0;
        const int tn = (l + 1 < L) ? t - 1 : t + L;
        // (layer 1 gathers for itself, MODE 3: only layer-1 sections prefetch, for the layer-0 section behind them)
        const bool pre = (l == L - 1) && (ST || (tn >= 1 && tn <= T));
        unsigned peek = (unsigned)tn;
        bool go = false;
        // exchange work hung into the MFMA stream (k-block q of the whole layer-step, a constant after unrolling):
        //   QF  the flag owed for the OTHER layer's publish store, issued at the end of the section in front: a few blocks
        //       in that store has drained (`vmcnt(0)` with nothing else in the queue) and the peers, who look half-way
        //       through THEIR next section, are in no hurry
        //   QP  look at the flags the next section needs (one load per lane)    QJ  judge
        //   QJ .. QJ+7  one piece of the next section's gather per block
        constexpr int NBL = (l == 0) ? BXU + BH : 2 * BH;
        // (positions swept on MI355X, 1024 x 64: QF 1 / 2 / 3 / 10 / 16 -> 826 / 833 / 819 / 828 / 858 us -- earlier stalls on the store's
        //  acknowledgement, later the peers' look finds nothing; look 12 blocks ahead of the judge instead of 4 -> 840: the flags are not up yet)
        // XS (long windows, steady state, layer 1): the section starts with layer 0's input span of the NEXT step (see `active` below); the flag owed
        // goes up behind that span, not at block QF, and the look for the next section / its judge sit at C32_QPX / C32_QJX.  The layer-0 sections
        // between two such sections start in their recurrent span, 768 cycles closer to the publish store in front: their QF is BXU + C32_QFP.
        // (C32_XS = 0, for A/B runs: the section keeps its own look at block QF + 1 and layer 0 its input span; C32_QPX / C32_QJX hold all the same)
        constexpr bool LW = ST && !ENDS && MODE == 3;
        constexpr bool XS = LW && C32_XS != 0;
        // (outside the steady state one layer-0 section starts from the park as well, the one behind the last such section: its QF must lie in the recurrent span)
        constexpr int QF = (!ENDS && l == 0 && C32_XS != 0) ? (ST ? BXU + C32_QFP : (C32_QF > BXU ? C32_QF : BXU)) : C32_QF;
        constexpr int QP = (MODE == 1) ? 16 : LW ? C32_QPX : NBL / 2 - 2 + C32_QPD, QJ = (MODE == 1) ? 20 : LW ? C32_QJX : NBL / 2 + 2 + C32_QPD;
        static_assert(!LW || (QP >= 0 && QP < QJ - 1 && QJ + NDMA <= 2 * BH), "the look, its judge and the eight pieces fit the section");
        // UG (long windows, steady state, layer 1): the eight pieces of BOTH gathers -- the next section's at blocks QJ .. QJ + 7, the own at blocks
        // 0 .. 7 of the input span -- go out whatever the judge says, at the blocks and addresses they always had: each piece is the three
        // instructions of dma_1k<true>, with no branch and no mask arithmetic around it, its source base derived ONCE (at the judge) and made opaque so
        // that hipcc keeps it in one scalar instead of re-deriving it per piece.  `pre` is always true here and a next section always exists, so the
        // copy has a buffer of its own to land in: hb0[ph & 1] for the next section (this section's input span reads the OTHER parity; layer 0's
        // recurrent span of phase ph + 1 is the buffer's next reader) resp. hb1 (next reader: this section's recurrent span, behind the barrier
        // between the spans; the head reads it only behind the final gather).  The judge keeps its place and its meaning: `go` / `got1` decide whether
        // that reader TRUSTS the copy.  Where a judge failed, the pieces have copied stale or half-written exchange bytes into the very block that the
        // blocking path then refills -- `vmcnt(0)` (the early pieces have landed), wait_flags, eight COLD pieces, `vmcnt(0)` -- in front of the
        // barrier every reader sits behind, and every wave refills exactly the KiBs it copied early.  The early copy lands in the same buffer at the same
        // time as a trusted one would: no reader sees anything new.  Sections outside the steady state keep the conditional form: there a next section
        // may not exist, and a copy nobody asked for would land in live data.
        constexpr bool UG = LW && C32_UG != 0;
        // RS: the hooks of these sections raise the flag owed by raise_hot() (layer 1 in its relocated form, and the layer-0 sections between two such)
        constexpr bool RS = ST && !ENDS && C32_XS != 0 && C32_RS != 0 && (l == 0 || XS);
        // (test builds: every APE_C32_LATE_EVERY-th steady-state phase judges "not yet")
        constexpr int LATE = APE_C32_LATE_EVERY;
        const bool late = LATE > 0 && ST && (ph % (LATE > 0 ? LATE : 1)) == 0;
        unsigned ug_src = 0u, ug_dst = 0u;
        bool staged = false;
#ifdef APE_CLUSTER_STAMPS
        unsigned long long hk0 = 0, hk_free = 0;
#define HK_BEGIN() do { if (ST) hk0 = now(); } while (0)
#define HK_END(k) do { if (ST) dgh[l][k] += now() - hk0; } while (0)
#else
#define HK_BEGIN() do {} while (0)
#define HK_END(k) do {} while (0)
#endif
        auto mid = [&](int q) {
#ifdef APE_CLUSTER_STAMPS
            // eight k-blocks without any hook (after QF + 1, before QP): what does a bare block cost inside the real kernel?
            if (ST && q == QF + 2) hk_free = now();
            if (ST && q == QF + 10) dgh[l][5] += now() - hk_free;
#endif
            if (!XS && q == QF) {
                HK_BEGIN();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if constexpr (RS) raise_hot(std::integral_constant<int, 1 - l>{});
                else raise_pending();
                HK_END(0);
            }
            // x of the next layer-0 step: registers -> LDS (layer 0's readers of xin finished before this section's barrier), and
            // the fetch of the step after it EARLY in the section: issued at its end the loads were the youngest entries but one of
            // the memory queue, and the counted wait at the top of the next section sat out their whole latency (13 us per launch)
            // (long windows, XA = 1: one step further ahead, into the buffer of that step's parity -- its last reader, of step ph, is either
            //  layer 0's section of this phase or the layer-1 section of the phase in front, both behind this section's barrier)
            if (l == L - 1 && q == ((MODE == 3) ? BH + 1 : QF + 1) && (ST || ph + 1 + XA < T)) {
                HK_BEGIN();
                stage_x(ph + 1 + XA);
                // (no branch around the loads inside a steady-state section: the last one fetches "step T", which wraps to a step of the ring --
                //  memory of this cluster's rows -- and is never staged)
                if (ST || ph + 2 + XA < T) fetch_x(ph + 2 + XA);
                staged = true;
                HK_END(1);
            }
            if constexpr (l == L - 1) {
                if (q == QP) look_issue(look_lds, look_voff, fl_desc, fl_off + (unsigned)(ln * NFL * sizeof(unsigned)));     // (always: no branch around it)
                if (q == QJ - 1) {                                // (the ds_read's latency passes under the next k-block)
                    C32_WAIT_T0();
                    look_landed();
                    C32_WAIT_T1(1);
                    peek = *look_mine;
                }
                if (q == QJ) {
                    HK_BEGIN();
                    go = pre && !late && __all((int)(peek >= (unsigned)tn)) != 0;
                    if constexpr (UG) {
                        ug_src = hx_base(ln, (tn - 1) & 1) + wave_kib;
                        // (hb0[parity], counted back from the own gather's LDS base hb1 = hb0 + 2 sets, which hipcc holds in a scalar anyway:
                        //  `hb0_lds + wave_kib` beside it was one scalar more than the section has)
                        ug_dst = (hb1_lds + wave_kib) - (unsigned)((2 - ((tn - 1) & 1)) * SET_BYTES);
                        asm volatile("" : "+s"(ug_src));
                    }
                    HK_END(2);
                }
                if constexpr (UG) {
                    if (q >= QJ && q < QJ + NDMA) {
                        HK_BEGIN();
                        dma_1k<true>(ug_dst, dma_voff, hx_desc, ug_src, (q - QJ) * 4096);
                        HK_END(3);
                    }
                } else if (q >= QJ && q < QJ + NDMA && go) {
                    HK_BEGIN();
                    issue_piece(HOT, ln, tn - 1, q - QJ);
                    HK_END(3);
                }
            }
        };
        float hnew[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (active) {
            // ---- stacked-gate product: one dependent chain of 32x32x2 MFMAs ---------------------------------------------------
            if constexpr (XS) {
                // ---- layer 0's input span of step ph + 1 (x_{t+2} W_ih: the one product of a phase that waits for no hand-over), under the
                //      round trip of the look at the own layer's flags.  The sixteen sums wait in this thread's slot of park_s; layer 0's next
                //      section starts from them instead of from its bias, the sums in the same order.  Only one accumulator is live at a time.
                look_issue(look_lds, look_voff, fl_desc, fl_off + (unsigned)(l * NFL * sizeof(unsigned)));
                f32x16 ax;
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) {
                    const f32x4 bv = bias_s[((wave * L + 0) * 4 + gate) * 64 + lane];
                    ax[4 * gate] = bv[0]; ax[4 * gate + 1] = bv[1]; ax[4 * gate + 2] = bv[2]; ax[4 * gate + 3] = bv[3];
                }
                span32<BXU, false, 4 * BXU>(ax, xin + ((ph + 1) & 1) * (MR * SX) + n * SX + hh * 4, 8, w0, 0, [&](int) {});
                mfma_drain(ax);
#pragma unroll
                for (int gate = 0; gate < 4; ++gate)
                    park_s[(wave * 4 + gate) * 64 + lane] = f32x4{ax[4 * gate], ax[4 * gate + 1], ax[4 * gate + 2], ax[4 * gate + 3]};
                parked = true;
            }
            // the accumulators' start values: the bias, or (layer 0 behind such a section) the parked sums of this step's input span
            bool from_park = false;
            if constexpr (l == 0 && !ENDS) {
                from_park = parked;
                parked = false;
            }
            const f32x4* const start_s = from_park ? park_s + wave * 4 * 64 + lane : bias_s + (wave * L + l) * 4 * 64 + lane;
            f32x16 acc;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const f32x4 bv = start_s[gate * 64];
                acc[4 * gate] = bv[0]; acc[4 * gate + 1] = bv[1]; acc[4 * gate + 2] = bv[2]; acc[4 * gate + 3] = bv[3];
            }
            const int frag = hh * 2 * MR * 4 + n * 4;             // this lane's hi fragment of slice 0: block hh, window n
            if constexpr (l == 0) {
                if (!from_park) span32<BXU, false, 4 * BXU>(acc, xin + (ENDS ? 0 : (t & 1) * (MR * SX)) + n * SX + hh * 4, 8, w0, 0, [&](int q) { mid(q); });
                if (ST || t > 0) span32_f16<BH / 2, false, NW0 / 4 - BX>(acc, hb0 + ((t - 1) & 1) * HL + frag, w0h, 0, [&](int q) { mid(BXU + q); });
            } else if constexpr (MODE == 3) {
                // input span: the common hooks (flag owed at QF, the look for the NEXT section at QP) + the look at the OWN layer's flags at
                // QO, the judge four blocks on, the gather behind it; outside the steady state a second look twelve blocks after the first
                constexpr int QO = QF + 1, QO2 = QO + 12;
                static_assert(XS || (QO2 + 4 + NDMA <= QP && (LW || QP < BH)), "the own gather's hooks sit in front of the look for the next section");
                unsigned pk = (unsigned)t;
                bool got1 = false, got2 = false;
                if constexpr (XS) {
                    // one wait for both: layer 0's publish store has drained (its flag goes up) and the own look has landed, a relocated span
                    // behind its issue; the eight pieces go out in the first blocks and have the rest of the span to land in
                    C32_WAIT_T0();
                    look_landed();
                    C32_WAIT_T1(0);
                    if constexpr (RS) raise_hot(std::integral_constant<int, 1 - l>{});
                    else raise_pending();
                    pk = *look_mine;
                    got1 = !late && __all((int)(pk >= (unsigned)t)) != 0;
                    // (UG: the own gather's source base, once; the judge above decides only whether the wait between the spans trusts the copy)
                    unsigned own_src = hx_base(l, (t - 1) & 1) + wave_kib;
                    if constexpr (UG) asm volatile("" : "+s"(own_src));
                    span32_f16<BH / 2, true, NW1 / 4>(acc, hb0 + (t & 1) * HL + frag, w1, 0, [&](int q) {
                        mid(q);
                        if constexpr (UG) {
                            if (q < NDMA) dma_1k<true>(hb1_lds + wave_kib, dma_voff, hx_desc, own_src, q * 4096);
                        } else if (q < NDMA && got1) issue_piece(HOT, l, t - 1, q);
                    });
                } else
                span32_f16<BH / 2, true, NW1 / 4>(acc, hb0 + (t & 1) * HL + frag, w1, 0, [&](int q) {
                    mid(q);
                    if (q == QO) look_issue(look_lds, look_voff, fl_desc, fl_off + (unsigned)(l * NFL * sizeof(unsigned)));
                    if (q == QO + 3) {
                        C32_WAIT_T0();
                        look_landed();
                        C32_WAIT_T1(0);
                        pk = *look_mine;
                    }
                    if (q == QO + 4) got1 = !late && __all((int)(pk >= (unsigned)t)) != 0;
                    if (q >= QO + 4 && q < QO + 4 + NDMA && got1) issue_piece(HOT, l, t - 1, q - (QO + 4));
                    if constexpr (!ST) {
                        if (q == QO2 && !got1) look_issue(look_lds, look_voff, fl_desc, fl_off + (unsigned)(l * NFL * sizeof(unsigned)));
                        if (q == QO2 + 3 && !got1) {
                            look_landed();
                            pk = *look_mine;
                        }
                        if (q == QO2 + 4 && !got1) got2 = __all((int)(pk >= (unsigned)t)) != 0;
                        if (q >= QO2 + 4 && q < QO2 + 4 + NDMA && got2) issue_piece(HOT, l, t - 1, q - (QO2 + 4));
                    }
                });
#ifdef APE_C32_COUNTS
                lc_t0 = __builtin_amdgcn_s_memtime();
#endif
                C32_WAIT_T0();
                if (!got1 && !got2) {
#ifdef APE_C32_WAITS
                    if (ST) lw_n[2] += 1u;
#endif
#ifdef APE_CLUSTER_STAMPS
                    dg_block[l] += 1;
#endif
#ifdef APE_C32_COUNTS
                    lc_block[l] += 1u;
#endif
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    raise_pending();                              // (a section entered with its flag still owed: T = 2's only one)
                    wait_flags(l, (unsigned)t);
#pragma unroll
                    for (int k = 0; k < NDMA; ++k) issue_piece(COLD, l, t - 1, k);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bar();                                            // every wave's pieces of h^1_{t-1} are in LDS; xin's readers are through
#ifdef APE_C32_COUNTS
                if (ST) { lc_top[l] += __builtin_amdgcn_s_memtime() - lc_t0; lc_n[l] += 1u; }
#endif
#ifdef APE_C32_WAITS
                C32_WAIT_T1(2);
                if (ST) lw_n[0] += 1u;
#endif
                if (ctl[0] != 0) return false;
                span32_f16<BH / 2, true, NW1 / 4>(acc, hb1 + frag, w1, BH, [&](int q) { mid(BH + q); });
            } else {
                span32_f16<BH / 2, true, NW1 / 4>(acc, hb0 + (t & 1) * HL + frag, w1, 0, [&](int q) { mid(q); });
                if (ST || t > 0) span32_f16<BH / 2, true, NW1 / 4>(acc, hb1 + frag, w1, BH, [&](int q) { mid(BH + q); });
                // (a section without a recurrent span -- step 0 of the long-window instantiation -- issues its look at block QP and never
                //  reaches the judge at QJ.  With a register destination that look stayed in flight over whatever hipcc gave the register to
                //  next: 2-4 % of the launches beside a memory-bound kernel returned a 32-window cluster off by 1e-2 at step 0 of layer 1,
                //  5e-4 at the end of a 9-step window, nothing visible from 24 steps on.  In its landing zone it harms nobody.)
            }
#ifdef APE_CLUSTER_STAMPS
            const unsigned long long c3 = ST ? now() : 0ull;
            if (ST) { dgc[l][0] += c1 - c0; dgc[l][1] += c2 - c1; dgc[l][2] += c3 - c2; }
#endif
            if constexpr (ST && !ENDS) asm volatile("; c32 steady section, layer %0: end" :: "i"(l));
            mfma_drain(acc);
            cell_update(acc, l, cst[l], hnew);
        }
        if (abort_word != 0) return false;                        // (a wave of this workgroup gave up in a blocking wait)
        if (!ST && pend_idx >= 0) {                               // (a section too short to reach block QF, or an idle one)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            raise_pending();
        }
        // (first step of a layer, idle sections: the hooks did not run, the next section gathers in the blocking form)
        if (go) prefetched = true;
#ifdef APE_CLUSTER_STAMPS
        if (go) dg_go[ln] += 1;
#endif
#ifdef APE_C32_COUNTS
        if (go) lc_go[ln] += 1u;
#endif
        if constexpr (l == L - 1) {
            // (an idle section, whose hooks did not run: the same here)
            if (!ST && !staged && ph + 1 + XA < T) {
                stage_x(ph + 1 + XA);
                if (ph + 2 + XA < T) fetch_x(ph + 2 + XA);
            }
        }
        // ---- publish: this lane's four fresh h values are one 16-byte piece of the exchange layout ----------------------------
        //      (exactly ONE store instruction per wave and section: the counted wait at the top of the next section relies on it)
        {
            const bool head_only = (l == L - 1) && !ST && t == T - 1;        // h^{L-1}_{T-1}: f32 for the head
            const u32x4 hs = split_h(hnew);
            const u32x4 hv = head_only ? u32x4{__builtin_bit_cast(unsigned, hnew[0]), __builtin_bit_cast(unsigned, hnew[1]),
                                               __builtin_bit_cast(unsigned, hnew[2]), __builtin_bit_cast(unsigned, hnew[3])} : hs;
            const unsigned off = active ? hx_base(l, t & 1) + (head_only ? pub_off : pub_off_split) : 0x80000000u;
            if (in_l2) __builtin_amdgcn_raw_buffer_store_b128(hv, hx_rsrc, off, 0, 0);
            else __builtin_amdgcn_raw_buffer_store_b128(hv, hx_rsrc, off, 0, 16 /* sc1: write-through */);
            if (active) {
                pend_idx = l * NFL + member * 4 + wave;
                // (long windows: the wave-uniform epoch goes to its vector register HERE, outside any MFMA stream, for raise_hot())
                if constexpr (EV) {
                    pend_epoch_v = (unsigned)(t + 1);
                    asm volatile("" : "+v"(pend_epoch_v));
                } else pend_epoch = (unsigned)(t + 1);
            }
        }
#ifdef APE_CLUSTER_STAMPS
        if (ST) { dgc[l][3] += now() - c2; dgc[l][4] += 1; }
#endif
        C32_TL(9 + 2 * (2 * ph + l));
        return true;
    };
    bool ok = true;
#pragma unroll 1
    for (int ph = ENDS ? 1 : 0; ph < P && ok; ++ph) {               // (ENDS: phase 0 = step 0 of layer 0, done above)
        // steady state: both layers active with a recurrent span, a next section to prefetch for, x to stage and to fetch
        const bool st0 = ph >= 2 && ph <= T - 3, st1 = st0;
        using M0 = std::integral_constant<int, 0>;
        using L0 = std::integral_constant<int, 0>;
        using L1 = std::integral_constant<int, 1>;
        ok = st0 ? section(std::true_type{}, L0{}, M0{}, ph) : section(std::false_type{}, L0{}, M0{}, ph);
        if (!ok) break;
        const int t1 = ph - 1;
        bool done1 = false;
        if constexpr (ENDS) {
            if (!st1 && t1 == 0 && T > 1) {
                ok = section(std::false_type{}, L1{}, std::integral_constant<int, 1>{}, ph);
                done1 = true;
            }
        }
        // (a step with a recurrent span: the section gathers h^1_{t-1} for itself, MODE 3; idle sections and step 0 of the long-window
        //  instantiation: the plain form)
        using M3 = std::integral_constant<int, 3>;
        if (!done1 && t1 >= 1 && t1 < T) {
            ok = st1 ? section(std::true_type{}, L1{}, M3{}, ph) : section(std::false_type{}, L1{}, M3{}, ph);
            done1 = true;
        }
        if (!done1) ok = section(std::false_type{}, L1{}, M0{}, ph);
    }
    if (!ok) return;
    // ---- final gather: h^{L-1}_{T-1} of every member (a section of layer L-1 "on step T": S0 only) -------------------------------
    {
        // the last step's flags go up per MEMBER: every wave has drained its store in front of the barrier, wave 0 stores the member's four
        // words in one instruction.  (Round 6: a cluster's 32 per-wave flag stores to one cache line, all issued at about the same time,
        // complete one after the other on the memory side -- the last one turned visible 3 .. 7 us after its issue, measured on
        // lstm_cluster16.hip's final gather, profiles/r06_flag_serialisation.md.  In the sections the looks are asynchronous and the
        // stores spread out; here every wave of the cluster is waiting for exactly these words.  The arrival-counter form of the other
        // kernels -- the last of a member's waves to drain raises for all four -- was tried in the sections of the short-window instantiation
        // and DEADLOCKS here: with two layers (and MODE 3's own gather) a wave on the blocking path waits, in front of the section's barrier, for
        // flags that include its OWN member's newest ones, which then need the arrival of waves that wait for it behind that barrier.  In
        // lstm_cluster.hip / lstm_cluster16.hip a blocking wait is only ever for flags at least a section older than the member's own pending
        // raise, and every wave of the member has passed that raise.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
        if (pend_idx >= 0) {
            if (wave == 0 && lane < 4)
                __hip_atomic_store(flags_of + (pend_idx - wave) + lane, EV ? pend_epoch_v : pend_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pend_idx = -1;
        }
        if (!prefetched) {
            wait_flags(L - 1, (unsigned)T);
#pragma unroll
            for (int k = 0; k < NDMA; ++k) issue_piece(COLD, L - 1, T - 1, k);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
        if (ctl[0] != 0) return;
        C32_TL(4);
    }

#ifdef APE_CLUSTER_STAMPS
    if (p.dbg_wg != nullptr && tid == 0 && cluster == 0 && member == 0)
        for (int k = 0; k < 2; ++k) { p.dbg_wg[16 + k] = dg_block[k]; p.dbg_wg[18 + k] = dg_go[k]; }
    if (p.dbg_wg != nullptr && lane == 0 && cluster == 0 && member == 0)
        for (int l = 0; l < 2; ++l)
            for (int k = 0; k < 5; ++k) p.dbg_wg[32 + wave * 16 + l * 5 + k] = dgc[l][k];
    if (p.dbg_wg != nullptr && lane == 0 && cluster == 0 && member == 0)
        for (int l = 0; l < 2; ++l)
            for (int k = 0; k < 6; ++k) p.dbg_wg[128 + wave * 16 + l * 6 + k] = dgh[l][k];
#endif
#ifdef APE_C32_COUNTS
    if (p.dbg_wg != nullptr && tid == 0 && cluster < 24) {
        unsigned long long* o = p.dbg_wg + 512 + (cluster * GH + member) * 8;
        o[0] = lc_block[0]; o[1] = lc_block[1]; o[2] = lc_go[0]; o[3] = lc_go[1];
        o[4] = lc_top[0]; o[5] = lc_top[1]; o[6] = lc_n[0]; o[7] = __builtin_amdgcn_s_memtime() - lc_start;
    }
#endif
#ifdef APE_C32_WAITS
    if (p.dbg_wg != nullptr && tid == 0 && cluster < 24) {
        unsigned long long* o = p.dbg_wg + 512 + (cluster * GH + member) * 8;
        o[0] = lw[0]; o[1] = lw[1]; o[2] = lw[2]; o[3] = lw[3];
        o[4] = lw_n[0]; o[5] = lw_n[1]; o[6] = lw_n[2]; o[7] = __builtin_amdgcn_s_memtime() - lw_start;
    }
#endif
    // ---- head: member m finishes windows 4m .. 4m+3 of the cluster's 32 ----------------------------------------------------------------
    {
        constexpr int RPM = MR / GH;
        // (window, target) dot products over H, 4 lanes each (k-blocks interleaved by 4), combined by lane shuffles
        const int part = tid & 3;
        for (int oi = tid >> 2; oi < ((RPM * O + 63) / 64) * 64; oi += 64) {
            const bool live = oi < RPM * O;
            const int rr = live ? oi / O : 0, o = live ? oi - rr * O : 0;
            const int row = member * RPM + rr, b = row0 + row;
            float s_acc = 0.0f;
            if (live) {
                const float* wv = p.w_out + (size_t)o * H;
                // unit k of window `row` lives at hb1[(k / 8) * (MR * 8) + row * 8 + (k % 8)]
                for (int kb = part; kb < H / 8; kb += 4) {
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(hb1 + kb * MR * 8 + row * 8);
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(hb1 + kb * MR * 8 + row * 8 + 4);
                    const f32x4 u0 = *reinterpret_cast<const f32x4*>(wv + kb * 8), u1 = *reinterpret_cast<const f32x4*>(wv + kb * 8 + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s_acc = fmaf(a0[j], u0[j], s_acc);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s_acc = fmaf(a1[j], u1[j], s_acc);
                }
            }
            s_acc += __shfl_xor(s_acc, 1, 64);
            s_acc += __shfl_xor(s_acc, 2, 64);
            if (p.y != nullptr && live && part == 0 && b < p.B) p.y[(size_t)b * O + o] = s_acc + p.b_out[o];
        }
    }
    C32_TL(5);
    // ---- self-cleaning: the last workgroup out re-zeroes every polled word ------------------------------------------
    __syncthreads();
    if (tid == 0)
        ctl[2] = (__hip_atomic_fetch_add(p.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) ? 1 : 0;
    __syncthreads();
    if (ctl[2] != 0) {
        const int n_flags = (int)(gridDim.x / GH) * L * NFL;
        for (int i = tid; i < n_flags; i += 256) __hip_atomic_store(p.xflags + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int i = tid; i < (int)gridDim.x; i += 256) __hip_atomic_store(xcc_words + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 8) __hip_atomic_store(class_ticket + tid * 16, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) __hip_atomic_store(p.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

constexpr size_t smem_bytes32() {
    return ((size_t)3 * 8 * 4 * 32 * 8 + (size_t)2 * 32 * 36) * sizeof(float) + (size_t)4 * (2 + 1) * 4 * 64 * 16 + (size_t)4 * 64 * sizeof(unsigned) + 16;
}

}  // namespace

bool ape_cluster32_supported(int H, int L, int KX) { return H == 256 && L == 2 && KX == 32; }

hipError_t ape_prepare_lstm_cluster32(int H, int L, int KX) {
    if (!ape_cluster32_supported(H, L, KX)) return hipSuccess;
    static_assert(smem_bytes32() <= APE_LDS_BYTES, "LDS layout exceeds a CU");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_lstm_cluster32<256, 2, 32, false, 3>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, APE_LDS_BYTES);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_lstm_cluster32<256, 2, 32, false, 4>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, APE_LDS_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_lstm_cluster32<256, 2, 32, true, 4>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, APE_LDS_BYTES);
}

// `clusters` = 32-window clusters needed; the grid is rounded up to whole block-index classes (8 clusters), the extra
// clusters own windows past the batch and only take part in the formation
hipError_t ape_launch_lstm_cluster32(int H, int L, int KX, int clusters, const ClusterParams& p, hipStream_t stream) {
    if (!ape_cluster32_supported(H, L, KX)) return hipErrorInvalidValue;
    const int grid_clusters = (clusters + 7) / 8 * 8;
    constexpr size_t smem = smem_bytes32();
    // (long windows: the input span skips the x slab's fourth k-block when it is all padding -- I = 22 / 20 of the deployed models)
    if (p.T <= APE_C32_ENDS_MAX_T) hipLaunchKernelGGL((ape_lstm_cluster32<256, 2, 32, true, 4>), dim3(grid_clusters * 8), dim3(256), smem, stream, p);
    else if (p.I <= 24) hipLaunchKernelGGL((ape_lstm_cluster32<256, 2, 32, false, 3>), dim3(grid_clusters * 8), dim3(256), smem, stream, p);
    else hipLaunchKernelGGL((ape_lstm_cluster32<256, 2, 32, false, 4>), dim3(grid_clusters * 8), dim3(256), smem, stream, p);
    return hipGetLastError();
}
