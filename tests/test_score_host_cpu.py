"""csrc/score_host.h: the host helpers the scoring entries share, checked in a stand-alone program (no GPU, no Python binding).

tests/host/score_host_main.cpp brings its own ape_fail and calls only the helpers that make no HIP call: the width of a truth row for
the three layouts and two kinds, the layouts that have a pose, and the lag-sweep check with the exact messages the entries have always
given and the window reach (back, fwd) written out by hand.  It is built with the address and undefined-behaviour sanitizers
(runtimes linked statically, so that the program runs as it is) where the host compiler has them, without otherwise."""
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "host" / "score_host_main.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _compile(exe, extra):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", str(SRC),
           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", str(exe)]
    return subprocess.run(cmd, capture_output=True, text=True)


def _have_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0


def test_score_host_helpers(tmp_path):
    exe = tmp_path / "score_host_main"
    sanitized = _have_sanitizers(tmp_path)
    r = _compile(exe, SANITIZE if sanitized else [])
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(f"sanitizers: {'address, undefined' if sanitized else 'not installed, built without'}")
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "score_host ok" in run.stdout
