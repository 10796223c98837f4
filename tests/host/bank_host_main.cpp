// Stand-alone check of csrc/bank_host.h's helpers that make no HIP call: the list and recording-start checks with their exact
// messages, the awaited value of the completion words and the wait for them.  Brings its own ape_fail, which records code and text.
// Built and run by tests/test_bank_host_cpu.py (address + undefined-behaviour sanitizers where the runtime is installed).
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <thread>

#include "../../arm-pose-estimation_amd/csrc/bank_host.h"

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

static void accepted(int rc, const char* what) { expect(rc == APE_OK, what); }

static void refused(int rc, const char* text, const char* what) {
    expect(rc == APE_ERR_INVALID_ARG && g_code == APE_ERR_INVALID_ARG && g_text == text, what);
}

int main() {
    // ---- stream lists of a bank of S = 4
    const int S = 4;
    const int32_t perm[4] = {2, 0, 3, 1};
    accepted(ape_check_stream_list("e", perm, 0, S, true), "list: K = 0");
    accepted(ape_check_stream_list("e", perm, S, S, true), "list: K = S, a permutation");
    accepted(ape_check_stream_list("e", perm, 3, S, false), "list: K = 3");
    accepted(ape_check_stream_list("e", nullptr, S, S, true), "list: NULL with K = S");
    refused(ape_check_stream_list("e", perm, -1, S, true), "e: K=-1 outside [0, S=4]", "list: K = -1");
    refused(ape_check_stream_list("e", perm, S + 1, S, false), "e: K=5 outside [0, S=4]", "list: K = S + 1");
    const int32_t neg[2] = {1, -1};
    refused(ape_check_stream_list("e", neg, 2, S, true), "e: stream index -1 (entry 1) outside [0, 4)", "list: index -1");
    const int32_t high[3] = {0, 1, 4};
    refused(ape_check_stream_list("e", high, 3, S, false), "e: stream index 4 (entry 2) outside [0, 4)", "list: index S");
    const int32_t dup[3] = {3, 1, 3};
    refused(ape_check_stream_list("e", dup, 3, S, true), "e: stream 3 listed twice", "list: duplicate");
    refused(ape_check_stream_list("e", nullptr, 2, S, true), "e: no stream list: K=2 must be S=4", "list: NULL with K != S");

    // ---- recording starts
    const int32_t one[1] = {0}, three[3] = {0, 1, 2};
    accepted(ape_check_segments("r", 1, one, 1), "segments: {0}, F = 1");
    accepted(ape_check_segments("r", 3, three, 3), "segments: {0, 1, 2}, F = 3");
    refused(ape_check_segments("r", 0, one, 1), "r: F=0 must be >= 1", "segments: F = 0");
    refused(ape_check_segments("r", 3, three, 0), "r: 0 recording starts for 3 frames (1 <= R <= F)", "segments: R = 0");
    refused(ape_check_segments("r", 2, three, 3), "r: 3 recording starts for 2 frames (1 <= R <= F)", "segments: R = F + 1");
    refused(ape_check_segments("r", 3, nullptr, 1), "r: NULL seg_starts", "segments: NULL");
    const int32_t late[1] = {1};
    refused(ape_check_segments("r", 3, late, 1), "r: seg_starts[0] = 1, must be 0", "segments: {1}");
    const int32_t flat[3] = {0, 2, 2};
    refused(ape_check_segments("r", 3, flat, 3), "r: seg_starts[2] = 2 (strictly rising, below F = 3)", "segments: {0, 2, 2}");
    const int32_t past[2] = {0, 3};
    refused(ape_check_segments("r", 3, past, 2), "r: seg_starts[1] = 3 (strictly rising, below F = 3)", "segments: {0, 3}, F = 3");

    // ---- the awaited value: + 1, never 0
    unsigned v = 0;
    ape_done_next(&v); expect(v == 1, "done_next: 0 -> 1");
    v = 7;
    ape_done_next(&v); expect(v == 8, "done_next: 7 -> 8");
    v = 0xFFFFFFFFu;
    ape_done_next(&v); expect(v == 1, "done_next: 0xFFFFFFFF -> 1");

    // ---- the wait: another thread writes the words one by one, as the frame's last kernel does
    volatile unsigned words[3] = {4, 4, 4};
    std::thread writer([&words] {
        for (int k = 0; k < 3; ++k) {
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
            __atomic_store_n(&words[k], 5u, __ATOMIC_RELEASE);
        }
    });
    expect(ape_done_wait(words, 3, 5u), "done_wait: three words written by a thread");
    writer.join();
    words[1] = 4;
    expect(!ape_done_wait(words, 3, 5u, 1000), "done_wait: one word left at the old value, 1000 spins");
    expect(ape_done_wait(words, 0, 9u, 1000), "done_wait: n = 0");

    if (g_bad == 0) printf("bank_host ok\n");
    return g_bad == 0 ? 0 : 1;
}
