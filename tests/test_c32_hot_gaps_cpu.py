"""The MFMA stream of lstm_cluster32.hip's long-window steady-state sections, read from the device assembly of the committed source
(tools/tally_c32_gaps.py; profiles/r10_cluster32_hot_gaps.md): no branch and no spill-lane move between two MFMAs, and a gather piece that is
two scalar adds and its LDS-DMA.  Counts only branches, lane moves and scalar opcodes; needs hipcc, no GPU."""
import importlib.util
import os
import shutil

import pytest

from tests.conftest import REPO

HIPCC = next((c for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
QUIET = ("s_waitcnt", "s_nop")


@pytest.fixture(scope="module")
def tallies():
    spec = importlib.util.spec_from_file_location("tally_c32_gaps", REPO / "tools" / "tally_c32_gaps.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t = mod.tally(str(REPO / "arm-pose-estimation_amd" / "csrc" / "lstm_cluster32.hip"))
    # <256, 2, 32, ENDS, BXU>: the two long-window instantiations by their input blocks, and the short-window one
    pick = lambda tag: next(v for k, v in t.items() if tag in k)
    return {3: pick("Lb0ELi3EE"), 4: pick("Lb0ELi4EE"), "ends": pick("Lb1ELi4EE")}


@pytest.mark.parametrize("bxu", [3, 4])
def test_layer0_stream_has_no_branch(tallies, bxu):
    (s,) = tallies[bxu]["layer0"]
    # input span (skipped behind a parked one: the label between the runs) + sixteen K = 16 slices of three MFMAs
    assert s["mfma"] == 4 * bxu + 48 and s["runs"] == [4 * bxu, 48]
    assert s["branches_in_breaks"] == 0 and s["branch_lines"] == []
    assert s["lane_moves"] == 0 and s["lane_moves_anywhere"] == 0
    assert s["piece_gaps"] == []


@pytest.mark.parametrize("bxu", [3, 4])
def test_layer1_stream_has_no_branch_and_bare_pieces(tallies, bxu):
    (s,) = tallies[bxu]["layer1"]
    # the relocated input span and the own input span in ONE run, the recurrent span in one behind the barrier between the spans
    # (hipcc lays blocks of other sections between the two markers as well: their runs lie in between)
    # (a branch around a hook would cut either run; the breaks the tally reports here are those of the foreign blocks)
    assert s["runs"][0] == 4 * bxu + 48 and s["runs"][-1] == 48, s["runs"]
    assert s["lane_moves"] == 0 and s["lane_moves_anywhere"] == 0
    # eight pieces of the own gather + eight of the next section's, each two s_add_i32 and the LDS-DMA beside what a hook-free gap holds
    assert len(s["piece_gaps"]) == 16
    for g in s["piece_gaps"]:
        scalar = [o for o in g["ops"] if o.startswith("s_") and not o.startswith(QUIET)]
        assert scalar == ["s_add_i32", "s_add_i32"], g
        assert g["ops"].count("buffer_load_dwordx4") == 1, g


def test_short_window_instantiation_carries_no_marked_section(tallies):
    assert tallies["ends"] == {}
