// Stand-alone check of ApeSlotPool (csrc/score_host.h), the staging slots under every scoring entry, without a GPU and without the HIP
// runtime: the dozen HIP functions the pool calls are fakes defined here.  An event is a completion flag this program sets by hand,
// synchronisations are counted, and the pinned and device blocks come from malloc, so that the address sanitizer sees every leak,
// double free and use after free of a slot's blocks (the fakes also keep their own list of live blocks, for a build without
// sanitizers).  Brings its own ape_fail, which records code and text.  Built and run by tests/test_slot_pool_cpu.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../../arm-pose-estimation_amd/csrc/score_host.h"

// ---- ape_fail and the bookkeeping of the checks ----------------------------------------------------------------------------------------
static int g_code = 0;
static std::string g_text;

int ape_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_code = code;
    g_text = buf;
    return code;
}

static int g_bad = 0;

static void expect(bool ok, const char* what) {
    if (ok) return;
    printf("FAILED: %s (last error %d \"%s\")\n", what, g_code, g_text.c_str());
    g_bad += 1;
}

static bool starts_with(const std::string& s, const char* head) { return s.compare(0, strlen(head), head) == 0; }

// ---- the fake runtime ------------------------------------------------------------------------------------------------------------------
struct FakeEvent {
    bool complete = true;                               // set by hand; a record clears it, a synchronise sets it (the wait is over)
    int records = 0;
};

static std::set<void*> g_pinned, g_device;              // the live blocks
static std::set<FakeEvent*> g_events;
static int g_host_allocs = 0, g_dev_allocs = 0, g_bad_frees = 0;
static int g_queries = 0, g_event_syncs = 0, g_stream_syncs = 0, g_records = 0;
static FakeEvent* g_last_synced = nullptr;
static hipError_t g_sticky = hipSuccess;                // what hipGetLastError returns and clears
static int g_fail_host_malloc = 0, g_fail_malloc = 0, g_fail_record = 0, g_fail_create = 0;   // fail the next n calls

static FakeEvent* fake(hipEvent_t e) { return reinterpret_cast<FakeEvent*>(e); }

hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
    (void)flags;
    if (g_fail_create > 0) { g_fail_create -= 1; return g_sticky = hipErrorOutOfMemory; }
    FakeEvent* e = new FakeEvent();
    g_events.insert(e);
    *event = reinterpret_cast<hipEvent_t>(e);
    return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t event) {
    g_queries += 1;
    if (fake(event)->complete) return hipSuccess;
    return g_sticky = hipErrorNotReady;
}

hipError_t hipEventSynchronize(hipEvent_t event) {
    g_event_syncs += 1;
    g_last_synced = fake(event);
    fake(event)->complete = true;
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    (void)stream;
    if (g_fail_record > 0) { g_fail_record -= 1; return g_sticky = hipErrorInvalidHandle; }
    g_records += 1;
    fake(event)->records += 1;
    fake(event)->complete = false;
    return hipSuccess;
}

hipError_t hipGetLastError(void) {
    const hipError_t e = g_sticky;
    g_sticky = hipSuccess;
    return e;
}

hipError_t hipHostMalloc(void** ptr, size_t size, unsigned flags) {
    (void)flags;
    if (g_fail_host_malloc > 0) { g_fail_host_malloc -= 1; return g_sticky = hipErrorOutOfMemory; }
    *ptr = malloc(size);
    memset(*ptr, 0x5a, size);
    g_pinned.insert(*ptr);
    g_host_allocs += 1;
    return hipSuccess;
}

hipError_t hipHostFree(void* ptr) {
    if (g_pinned.erase(ptr) != 1) { g_bad_frees += 1; return hipErrorInvalidValue; }    // not (or no longer) a live pinned block
    free(ptr);
    return hipSuccess;
}

hipError_t hipMalloc(void** ptr, size_t size) {
    if (g_fail_malloc > 0) { g_fail_malloc -= 1; return g_sticky = hipErrorOutOfMemory; }
    *ptr = malloc(size);
    memset(*ptr, 0xa5, size);
    g_device.insert(*ptr);
    g_dev_allocs += 1;
    return hipSuccess;
}

hipError_t hipFree(void* ptr) {
    if (g_device.erase(ptr) != 1) { g_bad_frees += 1; return hipErrorInvalidValue; }
    free(ptr);
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t stream) {
    (void)stream;
    g_stream_syncs += 1;
    return hipSuccess;
}

const char* hipGetErrorString(hipError_t e) {
    switch (e) {
        case hipSuccess: return "no error";
        case hipErrorOutOfMemory: return "out of memory";
        case hipErrorNotReady: return "not ready";
        case hipErrorInvalidHandle: return "invalid handle";
        case hipErrorLaunchFailure: return "launch failure";
        default: return "another error";
    }
}

// ---- a pool under test -----------------------------------------------------------------------------------------------------------------
static const hipStream_t STREAM = nullptr;

// (hidden, as the pool it holds is)
struct __attribute__((visibility("hidden"))) Bench {
    ApeSlotPool pool{"pool"};
    unsigned long long last_seq = 0;

    Bench() {                                           // every case counts from zero
        g_host_allocs = g_dev_allocs = g_bad_frees = g_queries = g_event_syncs = g_stream_syncs = g_records = 0;
        g_last_synced = nullptr;
        g_sticky = hipSuccess;
    }

    // take() held to what holds for every call: no slot in flight is handed out, the slot is of the calling device and large enough,
    // seq rises, the not-ready answer of a busy slot is not left behind as the call's error
    ApeSlot* take(int device, size_t pbytes, size_t dbytes, const char* what) {
        ApeSlot* s = nullptr;
        const int rc = pool.take(device, pbytes, dbytes, &s);
        expect(rc == APE_OK && s != nullptr, what);
        if (rc != APE_OK || s == nullptr) return nullptr;
        expect(fake(s->done)->complete || fake(s->done)->records == 0, "take: the slot handed out has an event that is not complete");
        expect(!s->used, "take: the slot handed out is still marked in flight");
        expect(s->device == device, "take: the slot handed out belongs to another device");
        expect(s->pcap >= pbytes && s->dcap >= dbytes, "take: the slot handed out is too small");
        expect((pbytes == 0 || g_pinned.count(s->pinned) == 1) && (dbytes == 0 || g_device.count(s->dev) == 1), "take: the slot's blocks are live");
        expect(s->seq > last_seq && s->seq == pool.seq, "take: seq rises with every take");
        expect(g_sticky == hipSuccess, "take: the not-ready answer of a busy slot is cleared");
        last_seq = s->seq;
        if (pbytes > 0) memset(s->pinned, 1, pbytes);    // (the sanitizer checks the whole block is there)
        if (dbytes > 0) memset(s->dev, 2, dbytes);
        return s;
    }

    void finish(ApeSlot* s) {
        expect(pool.finish("entry", s, hipSuccess, STREAM) == APE_OK && s->used && !fake(s->done)->complete, "finish: the slot is in flight");
    }

    size_t count(int device) const {
        size_t n = 0;
        for (const ApeSlot* q : pool.slots) n += q->device == device ? 1 : 0;
        return n;
    }

    // a process keeps its slots for good; this program gives everything back, so that what a slot lost on the way shows as a leak
    ~Bench() {
        for (ApeSlot* q : pool.slots) {
            if (q->pinned) expect(hipHostFree(q->pinned) == hipSuccess, "teardown: a slot's pinned block is live");
            if (q->dev) expect(hipFree(q->dev) == hipSuccess, "teardown: a slot's device block is live");
            g_events.erase(fake(q->done));
            delete fake(q->done);
            delete q;
        }
        expect(g_pinned.empty() && g_device.empty(), "teardown: no block outlives the slots");
        expect(g_events.empty(), "teardown: no event outlives the slots");
        expect(g_bad_frees == 0, "no block was freed twice");
    }
};

// nine calls in flight, the oldest not the first of the list
static void nine_in_flight() {
    Bench b;
    ApeSlot* s[8];
    for (int i = 0; i < 8; ++i) {
        s[i] = b.take(0, 64, 128, "take 1..8");
        if (!s[i]) return;
        for (int j = 0; j < i; ++j) expect(s[i] != s[j], "a slot in flight is not handed out a second time");
        b.finish(s[i]);
    }
    expect(b.pool.slots.size() == 8 && g_event_syncs == 0, "8 calls in flight: 8 slots and no wait");
    // the first call completes and its slot is taken again: now the oldest call in flight is the second one
    fake(s[0]->done)->complete = true;
    ApeSlot* again = b.take(0, 64, 128, "take 9: the first slot, free again");
    expect(again == s[0] && b.pool.slots.size() == 8 && g_event_syncs == 0, "a completed slot is taken again without a wait");
    if (!again) return;
    b.finish(again);
    const int queries = g_queries;
    ApeSlot* tenth = b.take(0, 64, 128, "take 10: every slot in flight");
    expect(g_queries - queries == 8, "every slot of the device is asked once");
    expect(g_event_syncs == 1 && g_stream_syncs == 0, "one more call waits exactly once");
    expect(g_last_synced == fake(s[1]->done), "it waits for the call with the smallest seq");
    expect(tenth == s[1], "and takes that call's slot");
    expect(b.pool.slots.size() == 8, "no ninth slot");
    if (tenth) b.finish(tenth);
}

// the first free slot in the list's order, whatever order the calls completed in
static void first_free() {
    Bench b;
    ApeSlot* s[4];
    for (int i = 0; i < 4; ++i) {
        s[i] = b.take(0, 32, 32, "take 1..4");
        if (!s[i]) return;
        b.finish(s[i]);
    }
    fake(s[2]->done)->complete = true;
    fake(s[1]->done)->complete = true;
    const int syncs = g_event_syncs;
    ApeSlot* t = b.take(0, 32, 32, "take with slots 1 and 2 free");
    expect(t == s[1], "the first free slot is taken");
    expect(b.pool.slots.size() == 4 && g_event_syncs == syncs, "no new slot and no wait");
    if (t) b.finish(t);
    ApeSlot* u = b.take(0, 32, 32, "take with slot 2 free");
    expect(u == s[2], "then the next free one");
}

// slots of another device are neither counted nor taken nor waited for
static void two_devices() {
    Bench b;
    ApeSlot* other = b.take(1, 16, 16, "device 1: first take");     // the smallest seq of all belongs to device 1
    if (!other) return;
    b.finish(other);
    ApeSlot* s[8];
    for (int i = 0; i < 8; ++i) {
        s[i] = b.take(0, 16, 16, "device 0: take 1..8");
        if (!s[i]) return;
        expect(s[i] != other, "device 0 does not take device 1's slot");
        b.finish(s[i]);
    }
    expect(b.count(0) == 8 && b.count(1) == 1 && g_event_syncs == 0, "8 slots of device 0 beside device 1's: no wait (the other device's slot is not counted)");
    // device 1's slot is free, all of device 0's are in flight: device 0 waits for its own oldest
    fake(other->done)->complete = true;
    const int syncs = g_event_syncs;
    ApeSlot* ninth = b.take(0, 16, 16, "device 0: take 9");
    expect(ninth == s[0] && g_event_syncs == syncs + 1 && g_last_synced == fake(s[0]->done), "device 0 waits for its own oldest call, not for device 1's");
    if (ninth) b.finish(ninth);
    // device 1 with its one slot in flight and a free slot on device 0: a second slot of its own
    ApeSlot* o2 = b.take(1, 16, 16, "device 1: second take");
    if (!o2) return;
    expect(o2 == other, "device 1 takes its own free slot");
    b.finish(o2);
    fake(s[3]->done)->complete = true;
    ApeSlot* o3 = b.take(1, 16, 16, "device 1: third take");
    expect(o3 != nullptr && o3 != s[3] && o3->device == 1 && b.count(1) == 2 && b.count(0) == 8, "device 1 gets a new slot, not device 0's free one");
    expect(g_event_syncs == syncs + 1, "and does not wait");
}

// blocks only grow, on the slot taken alone; a slot large enough is reused without an allocation
static void growth() {
    Bench b;
    ApeSlot* s = b.take(0, 100, 200, "first take");
    if (!s) return;
    expect(g_host_allocs == 1 && g_dev_allocs == 1 && s->pcap == 100 && s->dcap == 200, "the first call allocates both blocks");
    void* const pinned = s->pinned;
    void* const dev = s->dev;
    b.finish(s);
    // in flight: a larger call leaves it alone and gets a slot of its own
    ApeSlot* t = b.take(0, 1000, 2000, "larger take while the first is in flight");
    if (!t) return;
    expect(t != s && s->pinned == pinned && s->dev == dev && s->pcap == 100 && s->dcap == 200 && s->used, "a slot in flight keeps its blocks");
    expect(g_pinned.count(pinned) == 1 && g_device.count(dev) == 1, "and they are live");
    b.finish(t);
    fake(s->done)->complete = true;
    const int ha = g_host_allocs, da = g_dev_allocs;
    ApeSlot* u = b.take(0, 50, 100, "smaller take");
    expect(u == s && u->pinned == pinned && u->dev == dev && u->pcap == 100 && u->dcap == 200, "a smaller call reuses the slot as it is");
    expect(g_host_allocs == ha && g_dev_allocs == da, "without any allocation");
    if (!u) return;
    b.finish(u);
    fake(s->done)->complete = true;
    ApeSlot* v = b.take(0, 101, 200, "take one byte above the pinned block");
    expect(v == s && v->pcap == 101 && v->dcap == 200 && v->dev == dev, "only the block that is too small grows");
    expect(g_host_allocs == ha + 1 && g_dev_allocs == da && g_pinned.count(pinned) == 0 && g_pinned.size() == 2, "and the old block is freed");
    if (!v) return;
    b.finish(v);
    fake(s->done)->complete = true;
    ApeSlot* w = b.take(0, 0, 201, "take one byte above the device block");
    expect(w == s && w->pcap == 101 && w->dcap == 201 && g_dev_allocs == da + 1 && g_device.count(dev) == 0 && g_device.size() == 2, "the same for the device block");
}

// a failed allocation: refused under the pool's name, capacity 0 and no stale pointer, the next call is served
static void failed_allocations() {
    Bench b;
    ApeSlot* s = b.take(0, 100, 200, "first take");
    if (!s) return;
    b.finish(s);
    fake(s->done)->complete = true;

    ApeSlot* out = nullptr;
    g_fail_host_malloc = 1;
    int rc = b.pool.take(0, 150, 200, &out);
    expect(rc == APE_ERR_HIP && g_code == APE_ERR_HIP && starts_with(g_text, "pool: ") && g_text.find("hipHostMalloc") != std::string::npos &&
           g_text.find("out of memory") != std::string::npos, "hipHostMalloc fails: refused with the pool's prefix");
    expect(out == nullptr, "a refused take hands out nothing");
    expect(s->pinned == nullptr && s->pcap == 0 && g_pinned.empty(), "the pinned block is gone and its capacity is 0");
    expect(s->dev != nullptr && s->dcap == 200 && !s->used, "the device block stays, the slot is free");
    (void)hipGetLastError();
    ApeSlot* t = b.take(0, 60, 200, "the next take, smaller than the block that was lost");
    expect(t == s && t->pcap == 60 && g_pinned.size() == 1 && g_bad_frees == 0, "is served with a fresh block, nothing freed twice");
    if (!t) return;
    b.finish(t);
    fake(s->done)->complete = true;

    g_fail_malloc = 1;
    rc = b.pool.take(0, 60, 300, &out);
    expect(rc == APE_ERR_HIP && starts_with(g_text, "pool: ") && g_text.find("hipMalloc") != std::string::npos, "hipMalloc fails: refused with the pool's prefix");
    expect(s->dev == nullptr && s->dcap == 0 && g_device.empty() && s->pinned != nullptr && s->pcap == 60, "the device block is gone and its capacity is 0");
    (void)hipGetLastError();
    ApeSlot* u = b.take(0, 60, 120, "the next take, smaller than the block that was lost");
    expect(u == s && u->dcap == 120 && g_device.size() == 1 && g_bad_frees == 0, "is served with a fresh block, nothing freed twice");
    if (!u) return;
    b.finish(u);

    // no event: no slot joins the list
    g_fail_create = 1;
    const size_t before = b.pool.slots.size();
    rc = b.pool.take(0, 8, 8, &out);
    expect(rc == APE_ERR_HIP && starts_with(g_text, "pool: ") && g_text.find("hipEventCreate") != std::string::npos && b.pool.slots.size() == before,
           "hipEventCreate fails: refused with the pool's prefix and no slot added");
    (void)hipGetLastError();
}

// finish: what became of the launches and of the record
static void finishes() {
    Bench b;
    ApeSlot* s = b.take(0, 8, 8, "take");
    if (!s) return;
    g_fail_record = 1;
    const int ss = g_stream_syncs;
    int rc = b.pool.finish("entry", s, hipSuccess, STREAM);
    expect(rc == APE_ERR_HIP && g_text == "entry: hipEventRecord failed: invalid handle", "hipEventRecord fails: an error under the entry's name");
    expect(!s->used && g_stream_syncs == ss + 1, "the slot is left unused and the stream is synchronised once");
    (void)hipGetLastError();
    ApeSlot* t = b.take(0, 8, 8, "take after the failed record");
    expect(t == s, "the unused slot is taken again");
    if (!t) return;
    const int rec = fake(t->done)->records;
    rc = b.pool.finish("entry", t, hipErrorLaunchFailure, STREAM);
    expect(rc == APE_ERR_HIP && g_text == "entry: launch failed: launch failure", "the launch fails: an error under the entry's name");
    expect(fake(t->done)->records == rec + 1 && t->used && g_stream_syncs == ss + 1, "the event is still recorded and the slot is in flight");
    ApeSlot* u = b.take(0, 8, 8, "take while the failed launch's slot is in flight");
    expect(u != nullptr && u != t, "a slot in flight behind a failed launch is not handed out");
}

int main() {
    static_assert(ApeSlotPool::MAX_SLOTS == 8, "the cases below count to 8");
    nine_in_flight();
    first_free();
    two_devices();
    growth();
    failed_allocations();
    finishes();
    if (g_bad == 0) printf("slot_pool ok\n");
    return g_bad == 0 ? 0 : 1;
}
