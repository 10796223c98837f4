// Reaches and holds: a label per frame from a key with hysteresis and minimum lengths (ape_segment_frames), the run-length table of any
// labels (ape_segment_runs) and per-segment reductions of per-frame columns in a stated order (ape_segment_stats).  DESIGN.md 4.45; the
// reference has no counterpart; include/ape_hip.h states the rules.
//
// Every kernel runs on (tile, set) workgroups of 256 lanes over aligned tiles of 1024 frames; the two scans have the reduce-then-scan
// shape of ape_frame_times (an aggregate per tile and set, one workgroup per set scanning them, a third launch applying the carries): no
// workgroup waits for another.
//
// sf_reduce / sf_scan / sf_labels   step 1 and 2 of the labeller.  A frame's code is 0, 1 or PASS (undecided); a recording's first frame
//                          is never PASS (undecided there means first_label), so "the last code that is not PASS" needs no flag for the
//                          recording boundary.  The aggregate of a tile is that code over its frames: two bits.
// sf_minlen                steps 3 and 4 from the scratch s of the call's slot: the tile and (min_hold - 1) + (min_move - 1) <= 510 frames on
//                          either side in LDS, one byte each (bit 0: s, bit 1: the frame starts a recording); the fill of the tile and
//                          min_move - 1 frames on either side into a second byte array, then the drop of the tile's own frames.
// sr_reduce / sr_scan / sr_write    boundary flags (a recording's first frame, or a label that differs from the frame before); their count
//                          gives the id, the running maximum of their positions the first frame; the last frame of a run writes its row.
// ss_pieces / ss_fold      a workgroup owns the pieces (1024 frames counted from a segment's first frame) that start in its tile, lanes take
//                          (piece, column) pairs and walk them in frame order; the second launch adds the pieces of a long segment in order.
//
// Integer work in the first two entries; in the third every sum is one lane's own, in the order the header states: the same inputs give
// the same bits.  The only atomic is an LDS counter that compacts a tile's list of pieces (the order of the list reaches no result).
// No inline assembly.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "bank_host.h"
#include "score_host.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)
#include "score_device.h"

namespace {

using ape_scoredev::find_rec;

constexpr int SG_TILE = APE_SEG_PIECE;                  // frames per workgroup; a piece of ape_segment_stats
constexpr int SG_BLOCK = 256;
constexpr int SG_PER = SG_TILE / SG_BLOCK;              // consecutive frames of a lane in the scans
constexpr int SG_WAVES = SG_BLOCK / 64;
constexpr int SG_HALO = 2 * (APE_SEGMENT_MAX_MIN - 1);
constexpr int PASS = 2;
static_assert(SG_PER == 4 && SG_WAVES == 4, "the scans below are written for 256 lanes of 4 frames");

// ---- ape_segment_frames ----------------------------------------------------------------------------------------------------------------
struct SfParams {
    const void* keys;
    const int* starts;                                  // [R]
    const double* thresholds;                           // [P, 2]
    const int* mins;                                    // [P, 2]
    unsigned char* agg;                                 // [S, tiles]: the last code of a tile that is not PASS
    unsigned char* carry;                               // [S, tiles]: s of the frame before the tile (NULL: one tile)
    unsigned char* s;                                   // [S, F]: step 2 (the labels themselves where no set has a minimum above 1)
    unsigned char* labels;                              // [S, F]
    long long set_stride, frame_stride;
    int F, R, P, first_label, tiles;
};

// The last code that is not PASS among the lanes before this one (PASS: none), and among all lanes of the workgroup (*all).
// Every lane of the workgroup calls it; lwave: SG_WAVES ints of LDS.
__device__ __forceinline__ int last_code_before(int code, int* lwave, int* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long dec = __ballot(code != PASS), one = __ballot(code == 1);
    if (lane == 0) lwave[wave] = dec ? (int)((one >> (63 - __clzll((long long)dec))) & 1ull) : PASS;
    __syncthreads();
    const unsigned long long below = dec & ((1ull << lane) - 1ull);
    int in = PASS;
    if (below) in = (int)((one >> (63 - __clzll((long long)below))) & 1ull);
    else
        for (int w = wave - 1; w >= 0 && in == PASS; --w) in = lwave[w];
    int a = PASS;
    for (int w = SG_WAVES - 1; w >= 0 && a == PASS; --w) a = lwave[w];
    *all = a;
    __syncthreads();                                    // (lwave may be written again)
    return in;
}

// lcode[i] = the code of frame t0 + i, i < SG_TILE (PASS past F); returns the lane's own last code over its SG_PER frames
template <typename T>
__device__ __forceinline__ int tile_codes(const SfParams& p, long long t0, int set, unsigned char* lcode) {
    const int tid = threadIdx.x, pi = p.P > 1 ? set : 0;
    const double lo = p.thresholds[2 * pi], hi = p.thresholds[2 * pi + 1];
    const T* keys = static_cast<const T*>(p.keys) + (long long)set * p.set_stride;
    for (int i = tid; i < SG_TILE; i += SG_BLOCK) {
        const long long f = t0 + i;
        int c = PASS;
        if (f < p.F) {
            const double v = (double)keys[f * p.frame_stride];
            c = v > hi ? 1 : (v <= lo ? 0 : PASS);
        }
        lcode[i] = (unsigned char)c;
    }
    __syncthreads();
    const long long t1 = t0 + SG_TILE < p.F ? t0 + SG_TILE : p.F;
    for (int r = find_rec(p.starts, p.R, t0) + tid; r < p.R; r += SG_BLOCK) {          // an undecided first frame: first_label
        const long long s = p.starts[r];
        if (s >= t1) break;
        if (s >= t0 && lcode[s - t0] == PASS) lcode[s - t0] = (unsigned char)p.first_label;
    }
    __syncthreads();
    int own = PASS;
#pragma unroll
    for (int j = 0; j < SG_PER; ++j) {
        const int c = lcode[SG_PER * tid + j];
        own = c != PASS ? c : own;
    }
    return own;
}

template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void sf_reduce(const SfParams p) {
    __shared__ unsigned char lcode[SG_TILE];
    __shared__ int lwave[SG_WAVES];
    const int set = blockIdx.y;
    const int own = tile_codes<T>(p, (long long)blockIdx.x * SG_TILE, set, lcode);
    int all;
    (void)last_code_before(own, lwave, &all);
    if (threadIdx.x == 0) p.agg[(size_t)set * p.tiles + blockIdx.x] = (unsigned char)all;
}

// one workgroup per set; a lane takes a run of consecutive tiles
__global__ __launch_bounds__(SG_BLOCK) void sf_scan(const SfParams p) {
    __shared__ int lwave[SG_WAVES];
    const int set = blockIdx.x, tid = threadIdx.x;
    const int per = (p.tiles + SG_BLOCK - 1) / SG_BLOCK;
    const long long a = (long long)tid * per, b = a + per < p.tiles ? a + per : p.tiles;
    const unsigned char* agg = p.agg + (size_t)set * p.tiles;
    int own = PASS;
    for (long long t = a; t < b; ++t) {
        const int c = agg[t];
        own = c != PASS ? c : own;
    }
    int all;
    int in = last_code_before(own, lwave, &all);
    if (in == PASS) in = p.first_label;                 // (tile 0 begins a recording: never read)
    unsigned char* carry = p.carry + (size_t)set * p.tiles;
    for (long long t = a; t < b; ++t) {
        carry[t] = (unsigned char)in;
        const int c = agg[t];
        in = c != PASS ? c : in;
    }
}

template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void sf_labels(const SfParams p) {
    __shared__ unsigned char lcode[SG_TILE];
    __shared__ int lwave[SG_WAVES];
    const int set = blockIdx.y, tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * SG_TILE;
    const int own = tile_codes<T>(p, t0, set, lcode);
    int all;
    int in = last_code_before(own, lwave, &all);
    if (in == PASS) in = p.carry ? (int)p.carry[(size_t)set * p.tiles + blockIdx.x] : p.first_label;
#pragma unroll
    for (int j = 0; j < SG_PER; ++j) {                  // (a lane's own four bytes)
        const int c = lcode[SG_PER * tid + j];
        in = c != PASS ? c : in;
        lcode[SG_PER * tid + j] = (unsigned char)in;
    }
    __syncthreads();
    for (int i = tid; i < SG_TILE; i += SG_BLOCK)
        if (t0 + i < p.F) p.s[(size_t)set * (size_t)p.F + (size_t)(t0 + i)] = lcode[i];
}

// bit 1 of ls[g - g0] for every recording start g in [g0, g1)
__device__ __forceinline__ void mark_starts(const int* starts, int R, long long g0, long long g1, unsigned char* ls) {
    for (int r = find_rec(starts, R, g0) + threadIdx.x; r < R; r += SG_BLOCK) {
        const long long s = starts[r];
        if (s >= g1) break;
        if (s >= g0) ls[s - g0] |= 2;
    }
}

__global__ __launch_bounds__(SG_BLOCK) void sf_minlen(const SfParams p) {
    __shared__ unsigned char ls[SG_TILE + 2 * SG_HALO];  // frame g0 + i: bit 0 s, bit 1 starts a recording
    __shared__ unsigned char lf[SG_TILE + 2 * SG_HALO];  // s after the fill
    const int set = blockIdx.y, tid = threadIdx.x, pi = p.P > 1 ? set : 0;
    const int mh = p.mins[2 * pi], mm = p.mins[2 * pi + 1];
    const long long F = p.F, t0 = (long long)blockIdx.x * SG_TILE, t1 = t0 + SG_TILE < F ? t0 + SG_TILE : F;
    const long long g0 = t0 - (mh - 1) - (mm - 1) > 0 ? t0 - (mh - 1) - (mm - 1) : 0;
    const long long g1 = t1 + (mh - 1) + (mm - 1) < F ? t1 + (mh - 1) + (mm - 1) : F;
    const long long h0 = t0 - (mm - 1) > 0 ? t0 - (mm - 1) : 0, h1 = t1 + (mm - 1) < F ? t1 + (mm - 1) : F;
    const unsigned char* s = p.s + (size_t)set * (size_t)F;
    const int n = (int)(g1 - g0);
    for (int i = tid; i < n; i += SG_BLOCK) ls[i] = s[g0 + i] & 1;
    __syncthreads();
    mark_starts(p.starts, p.R, g0, g1, ls);
    __syncthreads();
    // the fill, for [h0, h1): the nearest 1 on the left at distance dl < min_hold, then one on the right with dl + dr <= min_hold; a walk
    // ends at its recording's edge (frame 0 starts a recording: no index below g0 is read)
    for (int i = (int)(h0 - g0) + tid; i < (int)(h1 - g0); i += SG_BLOCK) {
        int v = ls[i] & 1;
        if (v == 0 && mh > 1) {
            int dl = 0;
            for (int d = 1; d < mh; ++d) {
                if (ls[i - d + 1] & 2) break;
                if (ls[i - d] & 1) { dl = d; break; }
            }
            if (dl)
                for (int d = 1; dl + d <= mh; ++d) {
                    if (g0 + i + d >= F || (ls[i + d] & 2)) break;
                    if (ls[i + d] & 1) { v = 1; break; }
                }
        }
        lf[i] = (unsigned char)v;
    }
    __syncthreads();
    // the drop, for the tile's own frames: contiguous 1s on either side until min_move are counted
    for (int i = (int)(t0 - g0) + tid; i < (int)(t1 - g0); i += SG_BLOCK) {
        int v = lf[i];
        if (v && mm > 1) {
            int run = 1;
            for (int d = 1; run < mm; ++d) {
                if ((ls[i - d + 1] & 2) || !lf[i - d]) break;
                ++run;
            }
            for (int d = 1; run < mm; ++d) {
                if (g0 + i + d >= F || (ls[i + d] & 2) || !lf[i + d]) break;
                ++run;
            }
            v = run >= mm;
        }
        p.labels[(size_t)set * (size_t)F + (size_t)(g0 + i)] = (unsigned char)v;
    }
}

// ---- ape_segment_runs ------------------------------------------------------------------------------------------------------------------
struct SrParams {
    const unsigned char* labels;                        // [S, F]
    const int* starts;                                  // [R]
    int* tcount;                                        // [S, tiles]: boundaries in a tile
    int* tlast;                                         // [S, tiles]: the last boundary of a tile, -1 without one
    int* cbase;                                         // [S, tiles]: boundaries before the tile
    int* cfirst;                                        // [S, tiles]: the last boundary before the tile
    int* seg_of_frame;                                  // [S, F] or NULL
    int* n_segs;                                        // [S]
    int* table;                                         // [S, cap, 4]
    int F, R, cap, tiles;
};

// Exclusive prefix, in lane order over the workgroup, of a count and of a maximum (-1: none), and the workgroup's totals.
// Every lane calls it; lds: 2 * SG_WAVES ints.
__device__ __forceinline__ void block_scan(int cnt, int mx, int* lds, int* ex_cnt, int* ex_max, int* tot_cnt, int* tot_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ic = cnt, im = mx;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(ic, o, 64), u = __shfl_up(im, o, 64);
        if (lane >= o) { ic += t; im = u > im ? u : im; }
    }
    if (lane == 63) { lds[wave] = ic; lds[SG_WAVES + wave] = im; }
    __syncthreads();
    int pc = __shfl_up(ic, 1, 64), pm = __shfl_up(im, 1, 64);
    if (lane == 0) { pc = 0; pm = -1; }
    int tc = 0, tm = -1;
#pragma unroll
    for (int w = 0; w < SG_WAVES; ++w) {
        if (w == wave) { *ex_cnt = tc + pc; *ex_max = pm > tm ? pm : tm; }
        tc += lds[w];
        tm = lds[SG_WAVES + w] > tm ? lds[SG_WAVES + w] : tm;
    }
    *tot_cnt = tc; *tot_max = tm;
    __syncthreads();
}

// lflag[i] = 1 iff frame t0 + i begins a segment, for i <= SG_TILE and t0 + i < F; llab[i] = the label of frame t0 + i - 1
__device__ __forceinline__ void tile_flags(const SrParams& p, long long t0, int set, unsigned char* llab, unsigned char* lflag) {
    const int tid = threadIdx.x;
    const unsigned char* lab = p.labels + (size_t)set * (size_t)p.F;
    const long long g1 = t0 + SG_TILE + 1 < p.F ? t0 + SG_TILE + 1 : p.F;
    for (int i = tid; i < SG_TILE + 2; i += SG_BLOCK) {
        const long long f = t0 - 1 + i;
        llab[i] = f >= 0 && f < p.F ? lab[f] : 0;
        if (i < SG_TILE + 1) lflag[i] = 0;
    }
    __syncthreads();
    mark_starts(p.starts, p.R, t0, g1, lflag);
    __syncthreads();
    for (int i = tid; i < (int)(g1 - t0); i += SG_BLOCK) lflag[i] = (lflag[i] || llab[i + 1] != llab[i]) ? 1 : 0;
    __syncthreads();
}

__global__ __launch_bounds__(SG_BLOCK) void sr_reduce(const SrParams p) {
    __shared__ unsigned char llab[SG_TILE + 2], lflag[SG_TILE + 1];
    __shared__ int lds[2 * SG_WAVES];
    const int set = blockIdx.y, tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * SG_TILE;
    tile_flags(p, t0, set, llab, lflag);
    int cnt = 0, last = -1;
#pragma unroll
    for (int j = 0; j < SG_PER; ++j) {
        const int i = SG_PER * tid + j;
        if (t0 + i < p.F && lflag[i]) { ++cnt; last = (int)(t0 + i); }
    }
    int ec, em, tc, tm;
    block_scan(cnt, last, lds, &ec, &em, &tc, &tm);
    if (tid == 0) {
        p.tcount[(size_t)set * p.tiles + blockIdx.x] = tc;
        p.tlast[(size_t)set * p.tiles + blockIdx.x] = tm;
    }
}

__global__ __launch_bounds__(SG_BLOCK) void sr_scan(const SrParams p) {
    __shared__ int lds[2 * SG_WAVES];
    const int set = blockIdx.x, tid = threadIdx.x;
    const int per = (p.tiles + SG_BLOCK - 1) / SG_BLOCK;
    const long long a = (long long)tid * per, b = a + per < p.tiles ? a + per : p.tiles;
    const int* tcount = p.tcount + (size_t)set * p.tiles;
    const int* tlast = p.tlast + (size_t)set * p.tiles;
    int cnt = 0, last = -1;
    for (long long t = a; t < b; ++t) {
        cnt += tcount[t];
        last = tlast[t] > last ? tlast[t] : last;
    }
    int ec, em, tc, tm;
    block_scan(cnt, last, lds, &ec, &em, &tc, &tm);
    for (long long t = a; t < b; ++t) {
        p.cbase[(size_t)set * p.tiles + t] = ec;
        p.cfirst[(size_t)set * p.tiles + t] = em;
        ec += tcount[t];
        em = tlast[t] > em ? tlast[t] : em;
    }
    if (tid == 0) p.n_segs[set] = tc;
}

__global__ __launch_bounds__(SG_BLOCK) void sr_write(const SrParams p) {
    __shared__ unsigned char llab[SG_TILE + 2], lflag[SG_TILE + 1];
    __shared__ int lds[2 * SG_WAVES];
    const int set = blockIdx.y, tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * SG_TILE;
    tile_flags(p, t0, set, llab, lflag);
    int cnt = 0, last = -1;
#pragma unroll
    for (int j = 0; j < SG_PER; ++j) {
        const int i = SG_PER * tid + j;
        if (t0 + i < p.F && lflag[i]) { ++cnt; last = (int)(t0 + i); }
    }
    int ec, em, tc, tm;
    block_scan(cnt, last, lds, &ec, &em, &tc, &tm);
    if (p.cbase) {                                      // (NULL: one tile)
        ec += p.cbase[(size_t)set * p.tiles + blockIdx.x];
        const int c = p.cfirst[(size_t)set * p.tiles + blockIdx.x];
        em = c > em ? c : em;
    } else if (tid == 0) {
        p.n_segs[set] = tc;
    }
#pragma unroll
    for (int j = 0; j < SG_PER; ++j) {
        const int i = SG_PER * tid + j;
        const long long f = t0 + i;
        if (f >= p.F) break;
        if (lflag[i]) { ++ec; em = (int)f; }
        const int id = ec - 1;                          // (frame 0 is a boundary: ec >= 1)
        if (p.seg_of_frame) p.seg_of_frame[(size_t)set * (size_t)p.F + (size_t)f] = id;
        if ((f + 1 == p.F || lflag[i + 1]) && id < p.cap) {                            // the last frame of a run writes its row
            int* row = p.table + ((size_t)set * (size_t)p.cap + (size_t)id) * APE_SEG_TABLE_WIDTH;
            row[0] = find_rec(p.starts, p.R, em);
            row[1] = em;
            row[2] = (int)(f - em) + 1;
            row[3] = (int)llab[i + 1];
        }
    }
}

// ---- ape_segment_stats -----------------------------------------------------------------------------------------------------------------
constexpr int SS_REC = APE_SEG_STAT_WIDTH;              // a piece's record in the workspace has the width of a segment's
constexpr int SS_FOLD_TILES = 64 / APE_SEG_MAX_VALUES;  // tiles of a workgroup of ss_fold

struct SsParams {
    const void* values;
    const int* seg_of_frame;                            // [S, F]
    const int* table;                                   // [S, cap, 4]
    const int* n_segs;                                  // [S]
    double* ws;                                         // [S, tiles, V, 5]: the piece that starts in a tile and is not its segment's first
    int* second;                                        // [S, tiles]: the segment whose second piece starts in the tile, or -1
    double* out;                                        // [S, cap, V, 5]
    long long set_stride, frame_stride, col_stride;
    int F, V, cap, tiles;
};

template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void ss_pieces(const SsParams p) {
    __shared__ int lp_id[SG_TILE];
    __shared__ unsigned short lp_off[SG_TILE], lp_len[SG_TILE];
    __shared__ unsigned char lp_first[SG_TILE];
    __shared__ int lcount, lsecond;
    const int set = blockIdx.y, tid = threadIdx.x;
    const long long F = p.F, t0 = (long long)blockIdx.x * SG_TILE;
    if (tid == 0) { lcount = 0; lsecond = -1; }
    __syncthreads();
    const int* sof = p.seg_of_frame + (size_t)set * (size_t)F;
    const int* table = p.table + (size_t)set * (size_t)p.cap * APE_SEG_TABLE_WIDTH;
    const int nseg = p.n_segs[set] < p.cap ? p.n_segs[set] : p.cap;
    for (int i = tid; i < SG_TILE; i += SG_BLOCK) {
        const long long f = t0 + i;
        if (f >= F) break;
        const int id = sof[f];
        if (id < 0 || id >= nseg) continue;
        const long long first = table[(size_t)id * APE_SEG_TABLE_WIDTH + 1], len = table[(size_t)id * APE_SEG_TABLE_WIDTH + 2];
        const long long off = f - first;
        // (a table that does not belong to these ids is not followed out of the batch)
        if (first < 0 || len < 1 || first + len > F || off < 0 || off >= len || off % SG_TILE != 0) continue;
        const int at = atomicAdd(&lcount, 1);           // LDS; the order of the list reaches no result
        const long long left = len - off;
        lp_id[at] = id;
        lp_off[at] = (unsigned short)i;
        lp_len[at] = (unsigned short)(left < SG_TILE ? left : SG_TILE);
        lp_first[at] = off == 0;
        if (off == SG_TILE) lsecond = id;
    }
    __syncthreads();
    if (p.second && tid == 0) p.second[(size_t)set * p.tiles + blockIdx.x] = lsecond;
    const T* vals = static_cast<const T*>(p.values) + (long long)set * p.set_stride;
    const int pairs = lcount * p.V;
    for (int q = tid; q < pairs; q += SG_BLOCK) {
        const int pc = q / p.V, v = q - pc * p.V;
        const long long f0 = t0 + lp_off[pc];
        const int len = lp_len[pc];
        const T* src = vals + f0 * p.frame_stride + (long long)v * p.col_stride;
        double sum = 0.0, sq = 0.0, mx = -INFINITY;
        int cnt = 0, arg = -1;
#pragma unroll 4
        for (int k = 0; k < len; ++k) {
            const double x = (double)src[(long long)k * p.frame_stride];
            if (x == x) {
                if (cnt == 0 || x > mx) { mx = x; arg = (int)f0 + k; }
                ++cnt;
                sum = sum + x;
                const double xx = x * x;
                sq = sq + xx;
            }
        }
        double* dst = lp_first[pc] ? p.out + (((size_t)set * (size_t)p.cap + (size_t)lp_id[pc]) * p.V + v) * SS_REC
                                   : p.ws + (((size_t)set * (size_t)p.tiles + blockIdx.x) * p.V + v) * SS_REC;
        dst[0] = (double)cnt; dst[1] = sum; dst[2] = sq; dst[3] = mx; dst[4] = (double)arg;
    }
}

// lane (tile, column): where a segment's second piece starts in the tile, its pieces are added in order
__global__ __launch_bounds__(64) void ss_fold(const SsParams p) {
    const int set = blockIdx.y, v = threadIdx.x % APE_SEG_MAX_VALUES;
    const long long tile = (long long)blockIdx.x * SS_FOLD_TILES + threadIdx.x / APE_SEG_MAX_VALUES;
    if (tile >= p.tiles || v >= p.V) return;
    const int id = p.second[(size_t)set * p.tiles + tile];
    if (id < 0) return;
    const int* row = p.table + ((size_t)set * (size_t)p.cap + (size_t)id) * APE_SEG_TABLE_WIDTH;
    const long long first = row[1], len = row[2];
    double* o = p.out + (((size_t)set * (size_t)p.cap + (size_t)id) * p.V + v) * SS_REC;
    double cnt = o[0], sum = 0.0 + o[1], sq = 0.0 + o[2], mx = o[3], arg = o[4];
    for (long long off = SG_TILE; off < len; off += SG_TILE) {
        const double* w = p.ws + (((size_t)set * (size_t)p.tiles + (size_t)((first + off) / SG_TILE)) * p.V + v) * SS_REC;
        if (w[0] > 0.0 && (cnt == 0.0 || w[3] > mx)) { mx = w[3]; arg = w[4]; }
        cnt = cnt + w[0];
        sum = sum + w[1];
        sq = sq + w[2];
    }
    o[0] = cnt; o[1] = sum; o[2] = sq; o[3] = mx; o[4] = arg;
}

// the staging of a call: host arrays, tile aggregates, scratch (score_host.h); one pool per entry
ApeSlotPool g_frames("segment_frames"), g_runs("segment_runs"), g_stats("segment_stats");

inline size_t up8(size_t n) { return (n + 7) & ~(size_t)7; }

inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}

inline int check_sets(const char* who, int32_t n_sets) {
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "%s: S=%d sets (1 .. %d)", who, n_sets, APE_POST_MAX_CONFIGS);
    return APE_OK;
}

}  // namespace

int ape_segment_frames(const void* keys_dev, int32_t keys_dtype, int32_t n_sets, int64_t set_stride, int32_t F, int64_t frame_stride,
                       const int32_t* seg_starts_host, int32_t R, const double* thresholds_host, const int32_t* mins_host, int32_t P,
                       int32_t first_label, uint8_t* labels_dev, void* stream) {
    const char* who = "segment_frames";
    if (!keys_dev || !seg_starts_host || !thresholds_host || !mins_host || !labels_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (keys_dtype != APE_F32 && keys_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector %d", who, keys_dtype);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (int rc = check_sets(who, n_sets)) return rc;
    if (P != 1 && P != n_sets) return ape_fail(APE_ERR_INVALID_ARG, "%s: P=%d rows of thresholds (1 or S = %d)", who, P, n_sets);
    bool plain = true;                                  // no set has a minimum above 1: step 2 is the result
    for (int i = 0; i < P; ++i) {
        const double lo = thresholds_host[2 * i], hi = thresholds_host[2 * i + 1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || hi < lo)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: thresholds[%d] = (%g, %g) (finite, lo <= hi)", who, i, lo, hi);
        for (int j = 0; j < 2; ++j) {
            const int m = mins_host[2 * i + j];
            if (m < 1 || m > APE_SEGMENT_MAX_MIN)
                return ape_fail(APE_ERR_INVALID_ARG, "%s: mins[%d][%d] = %d outside 1..%d", who, i, j, m, APE_SEGMENT_MAX_MIN);
            plain = plain && m == 1;
        }
    }
    if (first_label != 0 && first_label != 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: first_label %d (0 or 1)", who, first_label);
    if (frame_stride < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: frame_stride %lld below 1", who, (long long)frame_stride);
    // the last element read, in elements from keys_dev: every stride is positive from here on
    long long extent = 0, term = 0;
    bool fits = !__builtin_mul_overflow((long long)(F - 1), (long long)frame_stride, &extent);
    if (n_sets > 1) {
        if (!fits || set_stride <= extent)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: set_stride %lld does not clear a set of F frames", who, (long long)set_stride);
        fits = !__builtin_mul_overflow((long long)(n_sets - 1), (long long)set_stride, &term) && !__builtin_add_overflow(extent, term, &extent);
    }
    const long long esize = keys_dtype == APE_F32 ? 4 : 8;
    fits = fits && !__builtin_add_overflow(extent, 1ll, &extent) && !__builtin_mul_overflow(extent, esize, &extent);
    if (!fits) return ape_fail(APE_ERR_INVALID_ARG, "%s: the extent of the keys does not fit 63 bits", who);
    if ((uintptr_t)keys_dev & (uintptr_t)(esize - 1)) return ape_fail(APE_ERR_INVALID_ARG, "%s: keys_dev is not aligned to its element", who);
    const size_t SF = (size_t)n_sets * (size_t)F;
    if (overlaps(keys_dev, (size_t)extent, labels_dev, SF)) return ape_fail(APE_ERR_INVALID_ARG, "%s: labels_dev overlaps keys_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_frames.prefix, hipGetDevice(&device));

    const int tiles = (int)(((long long)F + SG_TILE - 1) / SG_TILE);
    const size_t thr_bytes = (size_t)P * 2 * sizeof(double), min_bytes = up8((size_t)P * 2 * sizeof(int));
    const size_t host_bytes = up8(thr_bytes + min_bytes + (size_t)R * sizeof(int));   // thresholds, minimum lengths, starts
    const size_t agg_bytes = up8((size_t)n_sets * tiles);
    const size_t dev_bytes = host_bytes + 2 * agg_bytes + (plain ? 0 : SF);            // + aggregates, carries, scratch s

    std::lock_guard<std::mutex> lock(g_frames.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_frames.take(device, host_bytes, dev_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, thresholds_host, thr_bytes);
    memcpy(pin + thr_bytes, mins_host, (size_t)P * 2 * sizeof(int));
    memcpy(pin + thr_bytes + min_bytes, seg_starts_host, (size_t)R * sizeof(int));
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return g_frames.finish(who, slot, e, st);

    SfParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.keys = keys_dev;
    p.thresholds = reinterpret_cast<const double*>(dev);
    p.mins = reinterpret_cast<const int*>(dev + thr_bytes);
    p.starts = reinterpret_cast<const int*>(dev + thr_bytes + min_bytes);
    p.agg = reinterpret_cast<unsigned char*>(dev + host_bytes);
    p.carry = tiles > 1 ? p.agg + agg_bytes : nullptr;
    p.s = plain ? labels_dev : p.agg + 2 * agg_bytes;
    p.labels = labels_dev;
    p.set_stride = n_sets > 1 ? (long long)set_stride : 0; p.frame_stride = frame_stride;
    p.F = F; p.R = R; p.P = P; p.first_label = first_label; p.tiles = tiles;

    const dim3 grid((unsigned)tiles, (unsigned)n_sets), block(SG_BLOCK);
    const bool f32 = keys_dtype == APE_F32;
    if (tiles > 1) {
        if (f32) hipLaunchKernelGGL(sf_reduce<float>, grid, block, 0, st, p);
        else hipLaunchKernelGGL(sf_reduce<double>, grid, block, 0, st, p);
        hipLaunchKernelGGL(sf_scan, dim3((unsigned)n_sets), block, 0, st, p);
    }
    if (f32) hipLaunchKernelGGL(sf_labels<float>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(sf_labels<double>, grid, block, 0, st, p);
    if (!plain) hipLaunchKernelGGL(sf_minlen, grid, block, 0, st, p);
    return g_frames.finish(who, slot, hipGetLastError(), st);
}

int ape_segment_runs(const uint8_t* labels_dev, int32_t n_sets, int32_t F, const int32_t* seg_starts_host, int32_t R,
                     int32_t* seg_of_frame_dev, int32_t* n_segs_dev, int32_t* table_dev, int32_t cap, void* stream) {
    const char* who = "segment_runs";
    if (!labels_dev || !seg_starts_host || !n_segs_dev || !table_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (int rc = check_sets(who, n_sets)) return rc;
    if (cap < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: cap=%d must be >= 1", who, cap);
    if (((uintptr_t)seg_of_frame_dev | (uintptr_t)n_segs_dev | (uintptr_t)table_dev) & 3u)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: an int32 output is not aligned to its element", who);
    const size_t SF = (size_t)n_sets * (size_t)F;
    const size_t sof_bytes = seg_of_frame_dev ? SF * sizeof(int) : 0, n_bytes = (size_t)n_sets * sizeof(int);
    const size_t tab_bytes = (size_t)n_sets * (size_t)cap * APE_SEG_TABLE_WIDTH * sizeof(int);
    if (overlaps(labels_dev, SF, n_segs_dev, n_bytes) || overlaps(labels_dev, SF, table_dev, tab_bytes) ||
        (seg_of_frame_dev && overlaps(labels_dev, SF, seg_of_frame_dev, sof_bytes)))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: an output overlaps labels_dev", who);
    if (overlaps(n_segs_dev, n_bytes, table_dev, tab_bytes) ||
        (seg_of_frame_dev && (overlaps(seg_of_frame_dev, sof_bytes, n_segs_dev, n_bytes) || overlaps(seg_of_frame_dev, sof_bytes, table_dev, tab_bytes))))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: two outputs overlap", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_runs.prefix, hipGetDevice(&device));

    const int tiles = (int)(((long long)F + SG_TILE - 1) / SG_TILE);
    const size_t host_bytes = up8((size_t)R * sizeof(int));
    const size_t agg_ints = (size_t)n_sets * tiles;
    const size_t dev_bytes = host_bytes + 4 * agg_ints * sizeof(int);

    std::lock_guard<std::mutex> lock(g_runs.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_runs.take(device, host_bytes, dev_bytes, &slot)) return rc;
    memcpy(slot->pinned, seg_starts_host, (size_t)R * sizeof(int));
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return g_runs.finish(who, slot, e, st);

    SrParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.labels = labels_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.tcount = reinterpret_cast<int*>(dev + host_bytes);
    p.tlast = p.tcount + agg_ints;
    p.cbase = tiles > 1 ? p.tlast + agg_ints : nullptr;
    p.cfirst = tiles > 1 ? p.tlast + 2 * agg_ints : nullptr;
    p.seg_of_frame = seg_of_frame_dev; p.n_segs = n_segs_dev; p.table = table_dev;
    p.F = F; p.R = R; p.cap = cap; p.tiles = tiles;

    const dim3 grid((unsigned)tiles, (unsigned)n_sets), block(SG_BLOCK);
    if (tiles > 1) {
        hipLaunchKernelGGL(sr_reduce, grid, block, 0, st, p);
        hipLaunchKernelGGL(sr_scan, dim3((unsigned)n_sets), block, 0, st, p);
    }
    hipLaunchKernelGGL(sr_write, grid, block, 0, st, p);
    return g_runs.finish(who, slot, hipGetLastError(), st);
}

int ape_segment_stats(const void* values_dev, int32_t values_dtype, int32_t n_value_sets, int64_t set_stride, int64_t frame_stride,
                      int64_t col_stride, int32_t V, int32_t n_sets, int32_t F, const int32_t* seg_of_frame_dev, const int32_t* table_dev,
                      const int32_t* n_segs_dev, int32_t cap, double* out_dev, void* stream) {
    const char* who = "segment_stats";
    if (!values_dev || !seg_of_frame_dev || !table_dev || !n_segs_dev || !out_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (values_dtype != APE_F32 && values_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector %d", who, values_dtype);
    if (F < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: F=%d must be >= 1", who, F);
    if (int rc = check_sets(who, n_sets)) return rc;
    if (n_value_sets != 1 && n_value_sets != n_sets)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %d sets of values (1 or S = %d)", who, n_value_sets, n_sets);
    if (V < 1 || V > APE_SEG_MAX_VALUES) return ape_fail(APE_ERR_INVALID_ARG, "%s: V=%d columns (1 .. %d)", who, V, APE_SEG_MAX_VALUES);
    if (cap < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: cap=%d must be >= 1", who, cap);
    if (frame_stride < 1 || col_stride < 1)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: frame_stride %lld, col_stride %lld below 1", who, (long long)frame_stride, (long long)col_stride);
    long long extent = 0, term = 0;
    bool fits = !__builtin_mul_overflow((long long)(F - 1), (long long)frame_stride, &extent) &&
                !__builtin_mul_overflow((long long)(V - 1), (long long)col_stride, &term) && !__builtin_add_overflow(extent, term, &extent);
    if (n_value_sets > 1) {
        if (!fits || set_stride <= extent)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: set_stride %lld does not clear a set of F frames of V columns", who, (long long)set_stride);
        fits = !__builtin_mul_overflow((long long)(n_value_sets - 1), (long long)set_stride, &term) && !__builtin_add_overflow(extent, term, &extent);
    }
    const long long esize = values_dtype == APE_F32 ? 4 : 8;
    fits = fits && !__builtin_add_overflow(extent, 1ll, &extent) && !__builtin_mul_overflow(extent, esize, &extent);
    if (!fits) return ape_fail(APE_ERR_INVALID_ARG, "%s: the extent of the values does not fit 63 bits", who);
    if ((uintptr_t)values_dev & (uintptr_t)(esize - 1)) return ape_fail(APE_ERR_INVALID_ARG, "%s: values_dev is not aligned to its element", who);
    if ((((uintptr_t)seg_of_frame_dev | (uintptr_t)table_dev | (uintptr_t)n_segs_dev) & 3u) || ((uintptr_t)out_dev & 7u))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: an int32 input or out_dev is not aligned to its element", who);
    const size_t SF = (size_t)n_sets * (size_t)F;
    const size_t out_bytes = (size_t)n_sets * (size_t)cap * (size_t)V * APE_SEG_STAT_WIDTH * sizeof(double);
    if (overlaps(out_dev, out_bytes, values_dev, (size_t)extent) || overlaps(out_dev, out_bytes, seg_of_frame_dev, SF * sizeof(int)) ||
        overlaps(out_dev, out_bytes, table_dev, (size_t)n_sets * (size_t)cap * APE_SEG_TABLE_WIDTH * sizeof(int)) ||
        overlaps(out_dev, out_bytes, n_segs_dev, (size_t)n_sets * sizeof(int)))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: out_dev overlaps an input", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "a workspace is staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_stats.prefix, hipGetDevice(&device));

    const int tiles = (int)(((long long)F + SG_TILE - 1) / SG_TILE);
    const size_t ws_bytes = tiles > 1 ? (size_t)n_sets * tiles * (size_t)V * SS_REC * sizeof(double) : 0;
    const size_t second_bytes = tiles > 1 ? (size_t)n_sets * tiles * sizeof(int) : 0;

    std::lock_guard<std::mutex> lock(g_stats.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_stats.take(device, 8, 8 + ws_bytes + second_bytes, &slot)) return rc;

    SsParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.values = values_dev; p.seg_of_frame = seg_of_frame_dev; p.table = table_dev; p.n_segs = n_segs_dev;
    p.ws = tiles > 1 ? reinterpret_cast<double*>(dev + 8) : nullptr;                   // (one tile: every piece is a first piece)
    p.second = tiles > 1 ? reinterpret_cast<int*>(dev + 8 + ws_bytes) : nullptr;
    p.out = out_dev;
    p.set_stride = n_value_sets > 1 ? (long long)set_stride : 0; p.frame_stride = frame_stride; p.col_stride = col_stride;
    p.F = F; p.V = V; p.cap = cap; p.tiles = tiles;

    const dim3 grid((unsigned)tiles, (unsigned)n_sets);
    if (values_dtype == APE_F32) hipLaunchKernelGGL(ss_pieces<float>, grid, dim3(SG_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(ss_pieces<double>, grid, dim3(SG_BLOCK), 0, st, p);
    if (tiles > 1) hipLaunchKernelGGL(ss_fold, dim3((unsigned)((tiles + SS_FOLD_TILES - 1) / SS_FOLD_TILES), (unsigned)n_sets), dim3(64), 0, st, p);
    return g_stats.finish(who, slot, hipGetLastError(), st);
}
