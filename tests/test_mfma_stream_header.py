"""The inline-asm primitives of the hand-scheduled kernels have ONE definition each (csrc/mfma_stream.h, csrc/async_look.h): the wait states
and the comments that record why they are there were once copied from kernel file to kernel file, and sat on some copies and not on others.
A source check: where each definition text occurs over csrc/*.hip and csrc/*.h."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arm-pose-estimation_amd", "csrc")

# definition text -> {file: occurrences}, complete over the directory
ONCE = {
    "float sigm(": {"mfma_stream.h": 1},
    "float tanh_(": {"mfma_stream.h": 1},
    "float gate_act(": {"mfma_stream.h": 1},
    "void mfma32(": {"mfma_stream.h": 1},
    "void mfma_drain(f32x16": {"mfma_stream.h": 1},
    "void span32(": {"mfma_stream.h": 1},
    "void mfma16(f32x4&": {"mfma_stream.h": 1},              # (the f32 form: v_mfma_f32_16x16x4_f32)
    "void mfma16_last(f32x4&": {"mfma_stream.h": 1},
    "SPIN_LIMIT =": {"mfma_stream.h": 1},
    # the raw buffer descriptor is ape_make_desc -- and two kernels that spell it out, because through the helper their device assembly
    # comes out in another order (profiles/mfma_stream_header.md: lstm_cluster16.hip's exchange buffer in every build, lstm_upper128.hip's
    # mask words in the build with cycle stamps)
    "0x00020000u": {"async_look.h": 1, "lstm_cluster16.hip": 1, "lstm_upper128.hip": 1},
}


def test_each_stream_primitive_is_defined_once():
    found = {text: {} for text in ONCE}
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")): continue
        src = open(os.path.join(CSRC, fn)).read()
        for text in ONCE:
            if src.count(text): found[text][fn] = src.count(text)
    assert found == ONCE, {t: found[t] for t in ONCE if found[t] != ONCE[t]}
