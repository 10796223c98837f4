"""The co-residency protocol of the cluster kernels has ONE definition of each step (csrc/cluster_sync.h): the XCC id read,
the class-ticket draw, the same-XCD rendezvous, the wait for flag words, the give-up block and the LDS-only barrier were once copied from
kernel file to kernel file.  No test can run the give-up paths on a GPU, so that every kernel says the same thing is their only protection.
A source check: where each definition text occurs over csrc/*.hip and csrc/*.h."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arm-pose-estimation_amd", "csrc")

# definition text -> {file: occurrences}, complete over the directory
ONCE = {
    "hwreg(HW_REG_XCC_ID)": {"cluster_sync.h": 1},
    "s_waitcnt lgkmcnt(0)\\n\\ts_barrier": {"cluster_sync.h": 1},
    # the give-up block: the workgroup's abort flag (mlp_pipe.hip calls its control words ctl_s), then the status word
    "ctl[0] = 1;": {"cluster_sync.h": 1},
    "ctl_s[0] = 1;": {},
    # the wait for a row of flag words
    "if (__all((int)(v >= want))) return;": {"cluster_sync.h": 1},
    # the class-ticket draw -- and lstm_cluster.hip's, which draws from one of two counters (its `cls_mode`)
    "__hip_atomic_fetch_add(class_ticket": {"cluster_sync.h": 1, "lstm_cluster.hip": 1},
    # ... and the two kernels with launch-order tickets (no classes)
    "__hip_atomic_fetch_add(p.ticket": {"lstm_cluster.hip": 1, "lstm_cluster_f16.hip": 1},
    # the rendezvous -- and two kernels that spell it out, because through the helper their device assembly comes out differently
    # (profiles/cluster_sync_header.md: lstm_upper128.hip forms the address of the XCD words in another order, lstm_cluster.hip numbers the
    # states of its structurised control flow differently)
    "(v & 0xFu) == my_xcc": {"cluster_sync.h": 1, "lstm_upper128.hip": 1, "lstm_cluster.hip": 1},
}


def sources():
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h")): yield fn, open(os.path.join(CSRC, fn)).read()


def test_each_step_of_the_protocol_is_defined_once():
    found = {text: {} for text in ONCE}
    for fn, src in sources():
        for text in ONCE:
            if src.count(text): found[text][fn] = src.count(text)
    assert found == ONCE, {t: found[t] for t in ONCE if found[t] != ONCE[t]}


def test_no_kernel_stores_a_bare_number_to_the_status_word():
    """the give-up codes are ApeAbort (ape_internal.h); the status word is written with one of them, through ape_give_up or -- the ticket
    draws -- directly"""
    stores = {}
    for fn, src in sources():
        for m in re.finditer(r"__hip_atomic_store\(\s*(?:p\.)?status\s*,\s*([^,]+),", src):
            stores.setdefault(fn, []).append(m.group(1).strip())
    assert stores == {"cluster_sync.h": ["code", "APE_ABORT_TICKET"], "lstm_cluster.hip": ["APE_ABORT_TICKET"],
                      "lstm_cluster_f16.hip": ["APE_ABORT_TICKET"]}, stores
    internal = open(os.path.join(CSRC, "ape_internal.h")).read()
    codes = dict(re.findall(r"^\s*(APE_ABORT_\w+) = (\d+),", internal, re.M))
    assert codes == {"APE_ABORT_SPIN": "1", "APE_ABORT_TICKET": "2", "APE_ABORT_XCD_RENDEZVOUS": "5", "APE_ABORT_BUILDER_ROW": "6",
                     "APE_ABORT_COLLECT": "16"}, codes
