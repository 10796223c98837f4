// Host-side plumbing shared by the scoring entries (score.hip, frame_fit.hip, body_fit.hip, resample.hip, motion.hip): which
// layouts have a pose to score, the width of a truth row, the check of a lag sweep, and the staging slots of a call.  Inline host
// functions only, no device code; errors go through ape_fail.  The layout, width and lag-sweep checks make no HIP call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <vector>
#include "../../include/ape_hip.h"

// (ape_internal.h's declaration, repeated: this header also compiles on its own, in a host-only program that brings its own ape_fail)
int ape_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- argument checks; `who` names the entry in the message ---------------------------------------------------------------------------
// the layouts whose rows hold an arm pose
inline bool ape_scoring_layout(int32_t layout) {
    return layout == APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS || layout == APE_LAYOUT_ORI_CAL_LARM_UARM || layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS;
}

// values of a truth row of a scoring layout: the NN targets, or the est row
inline int ape_truth_width(int32_t layout, int32_t truth_kind) {
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    if (truth_kind == APE_TRUTH_TARGETS) return layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS ? 20 : (hips ? 14 : 12);
    return hips ? 21 : 14;
}

// The sweep lag_min .. lag_max on top of the recordings' offsets rec_lag_host[R] (NULL: none): at most APE_SCORE_MAX_LAGS lags, every
// lag of every recording within +-APE_SCORE_MAX_LAG.  *L: lags in the sweep; *back, *fwd: how far below / above its own rows a
// workgroup's truth window reaches, max(0, max_r(o_r + lag_max)) and max(0, -min_r(o_r + lag_min))
inline int ape_check_lag_sweep(const char* who, int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host, int32_t R, int* L, int* back,
                               int* fwd) {
    if (lag_min > lag_max) return ape_fail(APE_ERR_INVALID_ARG, "%s: lag_min %d above lag_max %d", who, lag_min, lag_max);
    const long long span = (long long)lag_max - (long long)lag_min + 1;
    if (span > APE_SCORE_MAX_LAGS) return ape_fail(APE_ERR_INVALID_ARG, "%s: %lld lags in the sweep, at most %d", who, span, APE_SCORE_MAX_LAGS);
    long long top = lag_max, bottom = lag_min;          // the largest and the smallest lag of any pair
    for (int r = 0; r < R; ++r) {
        const long long o = rec_lag_host ? rec_lag_host[r] : 0, lo = o + lag_min, hi = o + lag_max;
        if (lo < -APE_SCORE_MAX_LAG || lo > APE_SCORE_MAX_LAG || hi < -APE_SCORE_MAX_LAG || hi > APE_SCORE_MAX_LAG)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: recording %d: lags %lld .. %lld, |lag| is at most %d", who, r, lo, hi, APE_SCORE_MAX_LAG);
        top = r == 0 || hi > top ? hi : top;
        bottom = r == 0 || lo < bottom ? lo : bottom;
    }
    *L = (int)span;
    *back = top > 0 ? (int)top : 0;
    *fwd = bottom < 0 ? (int)-bottom : 0;
    return APE_OK;
}

// (ape_internal.h's APE_TRY with a prefix in front of the message: the file's pool's)
#define APE_SCORE_TRY(prefix, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: %s failed: %s", prefix, #expr, hipGetErrorString(_e)); } while (0)

// ---- the staging slots of a call -----------------------------------------------------------------------------------------------------
// A slot: a pinned block the host arrays are copied into (so they are consumed when the call returns and the copy to the device needs
// no wait) and the device block behind it (host arrays, partial records, tile aggregates).  A slot is taken again once the event
// recorded behind its last call has completed; slots only grow, and live as long as the process.  The first call on a device, and any
// call whose sizes outgrow the slot it takes, allocates (hipHostMalloc / hipMalloc, which may wait for the device): "the call does not
// wait" holds from the second call of a size on.  Up to MAX_SLOTS calls may be in flight per device; one more waits for the oldest.
// Every file has a pool of its own (its calls wait for each other only); `prefix` is what its HIP-error messages start with.
// lock mu -> take() -> fill slot->pinned, copy, launch -> finish().
struct ApeSlot {
    int device = -1;
    void* pinned = nullptr;
    void* dev = nullptr;
    size_t pcap = 0, dcap = 0;
    hipEvent_t done = nullptr;
    bool used = false;
    unsigned long long seq = 0;                         // order of the calls that took the slot
};

// (hidden: inline members the compiler keeps out of line would otherwise join the library's exported symbols)
struct __attribute__((visibility("hidden"))) ApeSlotPool {
    static constexpr size_t MAX_SLOTS = 8;
    const char* const prefix;
    std::mutex mu;                                      // held by a call from take() to finish()
    std::vector<ApeSlot*> slots;
    unsigned long long seq = 0;

    explicit ApeSlotPool(const char* prefix_) : prefix(prefix_) {}

    int take(int device, size_t pbytes, size_t dbytes, ApeSlot** out) {
        ApeSlot* s = nullptr;
        size_t mine = 0;
        for (ApeSlot* q : slots) {
            if (q->device != device) continue;
            ++mine;
            if (!q->used || hipEventQuery(q->done) == hipSuccess) { s = q; break; }
        }
        (void)hipGetLastError();                        // hipErrorNotReady of a busy slot is no error of this call
        if (s == nullptr && mine >= MAX_SLOTS) {        // every slot in flight: wait for the oldest
            for (ApeSlot* q : slots)
                if (q->device == device && (s == nullptr || q->seq < s->seq)) s = q;
            APE_SCORE_TRY(prefix, hipEventSynchronize(s->done));
        }
        if (s == nullptr) {
            s = new ApeSlot();
            s->device = device;
            const hipError_t e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
            if (e != hipSuccess) {
                delete s;
                return ape_fail(APE_ERR_HIP, "%s: hipEventCreate failed: %s", prefix, hipGetErrorString(e));
            }
            slots.push_back(s);
        }
        s->used = false;                                // (its last call is complete; set again once this call has recorded its event)
        if (s->pcap < pbytes) {
            if (s->pinned) (void)hipHostFree(s->pinned);
            s->pinned = nullptr; s->pcap = 0;
            APE_SCORE_TRY(prefix, hipHostMalloc(&s->pinned, pbytes, hipHostMallocDefault));
            s->pcap = pbytes;
        }
        if (s->dcap < dbytes) {
            if (s->dev) (void)hipFree(s->dev);
            s->dev = nullptr; s->dcap = 0;
            APE_SCORE_TRY(prefix, hipMalloc(&s->dev, dbytes));
            s->dcap = dbytes;
        }
        s->seq = ++seq;
        *out = s;
        return APE_OK;
    }

    // records the slot's event behind the launches and reports what became of them; `who` names the entry
    int finish(const char* who, ApeSlot* slot, hipError_t launched, hipStream_t st) {
        const hipError_t er = hipEventRecord(slot->done, st);  // the slot is in flight whatever became of the launches
        slot->used = er == hipSuccess;
        if (launched != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(launched));
        if (er != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return ape_fail(APE_ERR_HIP, "%s: hipEventRecord failed: %s", who, hipGetErrorString(er));
        }
        return APE_OK;
    }
};
