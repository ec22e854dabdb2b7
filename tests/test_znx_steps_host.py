"""CPU: the shared base-2^k carry steps, the same-base normalization plan and its walk (poulpy_amd/csrc/znx_steps.hpp: znx_inter_plan,
znx_normalize_inter_walk and the step functions under them) run on the host by a stand-alone program built with the host sanitizers, on
the oracle's digits.  (The shifted steps also run under tests/test_ckks_lincomb_host.py and tests/test_ckks_sum_host.py; the kernels
that call them: tests/test_gpu_parity.py and the other device parity tests.)"""
import os
import re
import shutil
import subprocess

import pytest

from poulpy_amd.layouts import VecZnx
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, COLS = 16, 2
BASES = (5, 12, 17, 50)
SIZES = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def _offsets(B, a_size, res_size):
    """every multiple of B in [-(a_size + 1) B, (res_size + 1) B], plus or minus 0, 1 and B - 1"""
    return sorted({m * B + s * d for m in range(-(a_size + 1), res_size + 2) for d in (0, 1, B - 1) for s in (1, -1)})


def _ranges(B, a_size, res_size, off):
    """(lsh, carry-only limbs, stored limbs, carry-spread limbs, res_start) of normalize.rs:83-101, by floor division"""
    lsh, lo = off % B, off // B

    def clamp(v, hi):
        return max(0, min(v, hi))
    res_end, res_start = clamp(-lo, res_size), clamp(a_size - lo, res_size)
    a_end, a_start = clamp(lo, a_size), clamp(res_size + lo, a_size)
    return lsh, a_size - a_start, max(a_start - a_end, 0), res_end, res_start


def _cases(ref):
    """(B, off, a, want) over every base, pair of sizes and offset, on normalized digits and on limbs over the full i64 range"""
    out = []
    for B in BASES:
        rng = seeded(7100 + B)
        for a_size in SIZES:
            for res_size in SIZES:
                for off in _offsets(B, a_size, res_size):
                    for log_bound in (B, 64):
                        a = VecZnx(N, COLS, a_size).fill_uniform(log_bound, rng)
                        want = VecZnx(N, COLS, res_size)
                        want.data[...] = 0x5A
                        for c in range(COLS):
                            ref.vec_znx_big_normalize(want, B, off, c, a, B, c)
                        out.append((B, off, a, want))
    return out


def test_plan_and_walk_stand_alone_under_the_host_sanitizers(ref, tmp_path):
    """tests/cpp/test_znx_steps.cpp includes znx_steps.hpp alone and calls znx_inter_plan / znx_normalize_inter_walk - the functions
    k_normalize_inter, k_mul_const_nz, k_lincomb_const and the launchers call - per coefficient on exactly-sized buffers, with its own
    main.  Built by the HIP compiler with -fsanitize=address,undefined on the host side only (plain where the compiler has no sanitizer
    runtimes); run as a child process on every case the oracle ran, at N = 16 with 2 columns."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert shutil.which(hipcc) is not None, "the HIP compiler that builds the library"
    cases = _cases(ref)
    shapes = [_ranges(B, a.size, want.size, off) for B, off, a, want in cases]
    for r in (1, 2, 3):   # the three ranges of the walk: each empty in some case and non-empty in another
        assert any(s[r] == 0 for s in shapes) and any(s[r] > 0 for s in shapes), r
    assert any(s[4] == 0 for s in shapes), "res_start == 0: a lies wholly below res"
    assert any(s[0] != 0 and off < 0 for s, (_, off, _, _) in zip(shapes, cases)) and any(s[0] == 0 for s in shapes)
    assert any(off > want.size * B for B, off, _, want in cases) and any(off < -a.size * B for B, off, a, _ in cases)
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for B, off, a, want in cases:
            f.write("%d %d %d %d %d %d\n" % (N, COLS, want.size, a.size, B, off))
            f.write(" ".join(map(str, a.data.reshape(-1).tolist())) + "\n")
            f.write(" ".join(map(str, want.data.reshape(-1).tolist())) + "\n")
    exe = str(tmp_path / "test_znx_steps")
    base = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "poulpy_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "test_znx_steps.cpp"), "-o", exe]
    san = subprocess.run(base + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[znx] HIP compiler without host sanitizer runtimes: built plain")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"all znx step checks passed: (\d+) cases", r.stdout)
    assert m and int(m.group(1)) == len(cases) >= 2000, r.stdout[-2000:]
