"""The choice of middle-kernel instantiation (poulpy_amd/csrc/mid_forms.hpp) and of the blind-rotation block step's (br_forms.hpp), host side:
the stand-alone check under the host sanitizers.  Nothing here needs a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mid128_forms.txt")


def test_form_choice_stand_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/test_mid_forms.cpp, no HIP, its own main: over every shape the launcher can be handed the chosen form has an entry in its list and
    keeps the kernels' preconditions; the dispatch notes recorded in tests/golden/mid128_forms.txt from the selection code that preceded
    mid_forms.hpp are re-derived string for string; the block step's one form without an entry is (9, 4) without LDS.  Built with
    -fsanitize=address,undefined with the sanitizer runtimes linked INTO the program where the host compiler has them, plain otherwise; run as a
    child process."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_mid_forms")
    base = [cxx, "-std=c++17", "-O1", "-g", os.path.join(ROOT, "tests", "cpp", "test_mid_forms.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[mid_forms] host compiler without sanitizer runtimes: built plain")
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "all middle-kernel form checks passed" in r.stdout, r.stdout[-2000:]


def test_recorded_notes_cover_both_kernels_and_every_trailing_text():
    notes = {line.split(" | ", 1)[1].rstrip("\n") for line in open(GOLDEN) if " | " in line and not line.startswith("#")}
    assert len(notes) == 37, sorted(notes)   # 19 k_mid128 + 18 k_mid128r list entries, each reachable
    assert sum(n.startswith("k_mid128<") for n in notes) == 19 and sum(n.startswith("k_mid128r<") for n in notes) == 18
    assert any(n.endswith("(two output-column passes per tile of 4 ciphertexts)") for n in notes)
    assert any(n.endswith("(8 ciphertexts per key value)") for n in notes)
