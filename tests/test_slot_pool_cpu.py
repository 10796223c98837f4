"""csrc/score_host.h: ApeSlotPool, the staging slots under every scoring entry, alone in a stand-alone program (no GPU, no HIP runtime, no
Python binding).

tests/host/slot_pool_main.cpp defines the HIP functions the pool calls as fakes -- an event is a completion flag the program sets by
hand, synchronisations are counted, pinned and device blocks come from malloc -- and holds take() and finish() to what the header
promises: a slot in flight is never handed out, the first free slot of the calling device is taken, another device's slots are neither
counted nor taken, the ninth call in flight waits exactly once, for the call with the smallest seq, and takes its slot, blocks only
grow and only on the slot taken, a failed allocation leaves capacity 0 and the next call is served without a double free, and finish
records the event whatever became of the launches.  It is built with the address and undefined-behaviour sanitizers (runtimes linked
statically, so that the program runs as it is) where the host compiler has them, without otherwise: the leak check then sees a block a
slot dropped on the way, since the program gives every slot back before it ends."""
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "host" / "slot_pool_main.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _compile(exe, extra):
    # (headers of the HIP runtime only: the program defines what it calls and links no libamdhip64)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", str(SRC), "-pthread",
           "-o", str(exe)]
    return subprocess.run(cmd, capture_output=True, text=True)


def _have_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0


def test_slot_pool(tmp_path):
    exe = tmp_path / "slot_pool_main"
    sanitized = _have_sanitizers(tmp_path)
    r = _compile(exe, SANITIZE if sanitized else [])
    assert r.returncode == 0, r.stderr
    needed = subprocess.run(["readelf", "-d", str(exe)], capture_output=True, text=True).stdout
    assert "amdhip64" not in needed, "the program must not link the HIP runtime"
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(f"sanitizers: {'address, undefined' if sanitized else 'not installed, built without'}")
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "slot_pool ok" in run.stdout
