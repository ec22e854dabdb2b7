"""The launch plan of the fused tail (poulpy_amd/csrc/tail_plan.hpp), host side: the stand-alone check under the host sanitizers.  Nothing here
needs a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tail_plans.txt")
KINDS = ["PLAIN", "RSH", "SGN", "NZ1", "NZ2", "ACC32", "NZ1W", "NZ2R", "NZ1O", "NZ2O", "SGN16", "SGN16R"]


def test_tail_plan_stand_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/test_tail_plan.cpp, no HIP, its own main: over every call shape of its sweep that tail_plan does not refuse, every launch's form has
    an entry for the plan, there are at most four launches and none is empty, and every column is written by exactly one launch or by exactly one
    pair (16-bit operand on a 16-bit form / operand variant that keeps body16_wide); the launches and refusals recorded in
    tests/golden/tail_plans.txt from the launcher that preceded tail_plan.hpp are re-derived string for string; the file holds every form, every
    branch of the split and every refusal.  Built with -fsanitize=address,undefined with the sanitizer runtimes linked INTO the program where the
    host compiler has them, plain otherwise; run as a child process."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_tail_plan")
    base = [cxx, "-std=c++17", "-O2", "-g", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_tail_plan.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[tail_plan] host compiler without sanitizer runtimes: built plain")
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "all fused-tail plan checks passed" in r.stdout, r.stdout[-2000:]


def test_recorded_plans_hold_every_form_and_every_refusal():
    results = [line.split(" | ", 1)[1].rstrip("\n") for line in open(GOLDEN) if " | " in line and not line.startswith("#")]
    launches = [l for r in results if not r.startswith("refuse") for l in r.split(" ; ")]
    assert {l.split("(")[0] for l in launches} == set(KINDS)
    assert {l.split(" ")[0] for l in launches if l.startswith("PLAIN(")} == {"PLAIN(0,0)", "PLAIN(0,1)", "PLAIN(1,0)", "PLAIN(1,1)"}
    refusals = {r for r in results if r.startswith("refuse")}
    assert len(refusals) == 14, sorted(refusals)   # 12 of launch_inv_tail and its column launcher, 2 of launch_inv_tail_nz
    assert max(len(r.split(" ; ")) for r in results) == 4
