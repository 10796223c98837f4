"""csrc/weight_pack.h: the register images of the weights, checked in a stand-alone program (no GPU, no HIP, no Python binding).

tests/host/weight_pack_main.cpp packs every image of every deployed model shape -- the 2 x 256 pocket (I = 22) and watch (I = 20) LSTMs,
the 3 x 128 upper-arm LSTM (I = 38), ImuPoseLSTM's 2 x 256 behind its 256-wide input layer, and a DropoutFF the MLP pipeline accepts --
from weights of a small integer generator and prints a 64-bit FNV-1a hash per image, plus the scale exponent S that pack_c32_split
returns.  The expected values in tests/golden/weight_images.json were recorded from the loops as they stood inside
ape_model_load_weights before they became this header: same generator, same shapes, each device copy replaced by the hash.  The program
itself checks that every packer writes exactly its *_elems() elements (two prefill patterns must give the same image; a canary behind
each buffer).  ROCm's clang++ builds it, as the header uses _Float16; with the address and undefined-behaviour sanitizers where they
link, without otherwise."""
import json
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "host" / "weight_pack_main.cpp"
GOLDEN = REPO / "tests" / "golden" / "weight_images.json"
CXX = "/opt/rocm/llvm/bin/clang++"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _have_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    exe = tmp_path / "probe"
    r = subprocess.run([CXX, *SANITIZE, str(probe), "-o", str(exe)], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 0


def test_weight_images_match_the_recorded_hashes(tmp_path):
    exe = tmp_path / "weight_pack_main"
    sanitized = _have_sanitizers(tmp_path)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(SANITIZE if sanitized else []), str(SRC), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(f"sanitizers: {'address, undefined' if sanitized else 'do not link here, built without'}")
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "weight_pack ok" in run.stdout
    got = dict(line.split() for line in run.stdout.splitlines() if len(line.split()) == 2 and "." in line.split()[0])
    want = json.loads(GOLDEN.read_text())
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
