"""GPU parity of GLWE x plaintext (pz_glwe_mul_plain_batched) and GLWE x constant (pz_glwe_mul_const_batched) against the oracle
compositions of tests/plain_oracle.py (poulpy-core operations/glwe.rs:66-303, poulpy-ckks leveled/default/mul.rs:342-415), bit-exact on the
normalized i64 limbs."""
import ctypes as C
import os

import numpy as np
import pytest

from poulpy_amd.layouts import VecZnx
from tests import plain_oracle as po
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu


def _run_plain(hip, ref, n, rank, a_size, b_size, res_size, ab, rb, off, mode, shared, batch, seed, chunk=0, abo=0, bbo=0, pool=None, a_fill=None,
               pt_fill=None):
    """`pool` distinct inputs (default: batch) tiled over the batch: every output is checked against its input's oracle result.  a_fill /
    pt_fill(t, data, rng) overwrite input t's ciphertext / plaintext digits in place (tests/unnormalized.py)."""
    from poulpy_amd.hal import GlweTensorParams
    rng = seeded(seed)
    cols = rank + 1
    assign = mode == "assign"
    if assign:
        a_size = res_size
    pool = pool or batch
    a_k, b_k = ab * a_size - abo, ab * b_size - bbo
    a_p = np.stack([VecZnx(n, cols, a_size).fill_uniform(ab, rng).data for _ in range(pool)])
    pt_p = np.stack([VecZnx(n, 1, b_size).fill_uniform(ab, rng).data for _ in range(1 if shared else pool)])
    for t in range(pool):
        if a_fill is not None:
            a_fill(t, a_p[t], rng)
        if pt_fill is not None and t < len(pt_p):
            pt_fill(t, pt_p[t], rng)
    want_p = np.empty((pool, res_size, cols, n), dtype=np.int64)
    for t in range(pool):
        pt = VecZnx(n, 1, b_size, pt_p[0 if shared else t].copy())
        if assign:
            r = VecZnx(n, cols, res_size, a_p[t].copy())
            po.glwe_mul_plain_assign(ref, off, r, a_k, pt, b_k, ab)
        else:
            r = VecZnx(n, cols, res_size)
            po.glwe_mul_plain(ref, off, r, rb, VecZnx(n, cols, a_size, a_p[t].copy()), a_k, pt, b_k, ab)
        want_p[t] = r.data
    idx = np.arange(batch) % pool
    a_all = np.ascontiguousarray(a_p[idx])
    pt_all = np.ascontiguousarray(pt_p if shared else pt_p[idx])
    with on_device(hip) as dev:
        d_a = dev.upload(a_all)
        d_pt = dev.upload(pt_all)
        if assign:
            d_r = d_a
        else:
            d_r = dev.alloc(batch * res_size * cols * n * 8)
        p = GlweTensorParams(rank=rank, a_size=a_size, b_size=b_size, ab_base2k=ab, a_effective_k=a_k, b_effective_k=b_k, res_size=res_size,
                             res_base2k=rb if not assign else ab, cnv_offset=off)
        assert hip.glwe_mul_plain_workspace_bytes(p, mode, shared, batch) > 0
        with on_device(hip, chunk=chunk):
            hip.glwe_mul_plain_batched(d_r.ptr, None if assign else d_a.ptr, d_pt.ptr, shared, p, mode, batch)
            hip.sync()
        got = d_r.download(np.int64, batch * res_size * cols * n).reshape(batch, res_size, cols, n)
    return got, want_p[idx]


# (n, rank, a_size, b_size, res_size, ab, rb, cnv_offset, a_bits_off, b_bits_off)
PLAIN_GRID = [
    (256, 1, 4, 3, 5, 12, 12, 24, 3, 0),     # hi = 1, lo = 0
    (256, 2, 4, 1, 4, 13, 13, 5, 0, 4),      # BS = 1, cnv_offset < base2k (hi = 0, lo < 0)
    (256, 1, 4, 4, 6, 12, 15, 30, 7, 0),     # BS = AS, cross-base
    (1024, 2, 5, 3, 5, 12, 12, 31, 0, 2),    # CKKS-like offset: 3 limbs of plaintext - 5 bits
    (4096, 1, 8, 3, 8, 12, 12, 31, 0, 0),    # N = 4096: the per-op kernels
    (8192, 1, 8, 3, 8, 12, 12, 31, 0, 0),    # pipeline plan: per-column k_mid_cnv (POULPY_DBG_MULPLAIN_FUSED=1: k_mid_cnv_pt<8, 3>)
    (8192, 2, 8, 8, 9, 12, 12, 0, 5, 3),     # <8, 8>, three columns, cnv_offset 0
    (8192, 2, 16, 1, 16, 12, 12, 25, 3, 0),  # <16, 1>
    (8192, 1, 16, 3, 16, 12, 12, 31, 0, 2),  # <16, 3>, CKKS-like offset
    (8192, 1, 16, 16, 16, 12, 12, 0, 0, 0),  # <16, 16>, poulpy-bench's layout
    (8192, 1, 5, 2, 5, 12, 12, 20, 0, 0),    # outside k_mid_cnv_pt's instantiations: per-column k_mid_cnv either way
    (4096, 1, 6, 3, 6, 12, 14, 29, 0, 0),    # cross-base on a pipeline plan: the per-op kernels
]


@pytest.mark.parametrize("shared", [False, True], ids=["per_ct", "shared"])
@pytest.mark.parametrize("mode", ["into", "assign"])
@pytest.mark.parametrize("case", PLAIN_GRID)
def test_glwe_mul_plain_batched(mods, case, mode, shared):
    n, rank, a_size, b_size, res_size, ab, rb, off, abo, bbo = case
    if mode == "assign" and rb != ab:
        pytest.skip("the assign form has one base2k (operations/glwe.rs:271)")
    ref, hip = mods(n)
    got, want = _run_plain(hip, ref, n, rank, a_size, b_size, res_size, ab, rb, off, mode, shared, batch=5, seed=n + off + rank, chunk=2,
                           abo=abo, bbo=bbo)
    assert np.array_equal(got, want), case


def _run_plain_pool(hip, ref, n, b_size, off, shared, batch, pool, chunk, seed):
    """rank 1, 16 limbs, base2k 12 on `batch` ciphertexts tiled from `pool` distinct inputs (uploaded / checked one ciphertext at a time, so
    that the host holds the pool only); returns the number of outputs checked."""
    from poulpy_amd.hal import GlweTensorParams
    rng = seeded(seed)
    cols, size, k = 2, 16, 12
    a_p = [VecZnx(n, cols, size).fill_uniform(k, rng) for _ in range(pool)]
    pt_p = [VecZnx(n, 1, b_size).fill_uniform(k, rng) for _ in range(1 if shared else pool)]
    want = []
    for t in range(pool):
        r = VecZnx(n, cols, size)
        po.glwe_mul_plain(ref, off, r, k, a_p[t].copy(), size * k, pt_p[0 if shared else t].copy(), b_size * k, k)
        want.append(r.data)
    ct, pb = size * cols * n * 8, b_size * n * 8
    with on_device(hip) as dev:
        d_a, d_r = dev.alloc(batch * ct, poison=False), dev.alloc(batch * ct, poison=False)
        d_pt = dev.alloc((1 if shared else batch) * pb, poison=False)
        for t in range(batch):
            hip._ck(hip.lib.pz_memcpy_h2d(hip.handle, d_a.at(t * ct), a_p[t % pool].data.ctypes.data_as(C.c_void_p), C.c_size_t(ct)))
            if not shared:
                hip._ck(hip.lib.pz_memcpy_h2d(hip.handle, d_pt.at(t * pb), pt_p[t % pool].data.ctypes.data_as(C.c_void_p), C.c_size_t(pb)))
        if shared:
            d_pt.upload(pt_p[0].data)
        hip.lib.pz_memset_d(hip.handle, d_r.ptr, 0x5A, C.c_size_t(batch * ct))
        p = GlweTensorParams(rank=1, a_size=size, b_size=b_size, ab_base2k=k, a_effective_k=size * k, b_effective_k=b_size * k, res_size=size, res_base2k=k,
                             cnv_offset=off)
        with on_device(hip, chunk=chunk):
            hip.glwe_mul_plain_batched(d_r.ptr, d_a.ptr, d_pt.ptr, shared, p, "into", batch)
            hip.sync()
        bad = [t for t in range(batch) if not np.array_equal(d_r.download(np.int64, ct // 8, t * ct).reshape(size, cols, n), want[t % pool])]
    assert not bad, bad[:8]
    return batch


def test_glwe_mul_plain_n65536_ckks_two_waves(mods):
    """N = 2^16, rank 1, 16 limbs, base2k 12, a 3-limb plaintext shared by 256 ciphertexts, cnv_offset from get_mul_pt_params
    (mul.rs:480-496: b.max_k + res_offset); a pool of 8 distinct inputs, a second wave forced with set_chunk; every output checked; the
    default middle kernel is k_mid_cnv per column (k_mid_cnv_pt<16, 3>: test_knobs_force_the_compositions_same_digits)."""
    n = 65536
    ref, hip = mods(n)
    hip.dispatch_notes(reset=True)
    assert _run_plain_pool(hip, ref, n, 3, 3 * 12, True, batch=256, pool=8, chunk=160, seed=1616) == 256
    notes = hip.dispatch_notes()
    assert "k_mid_cnv (a 16 + b 3 limbs" in notes and "k_mid_cnv_pt" not in notes, notes


def test_glwe_mul_plain_n65536_per_ciphertext_two_waves(mods):
    """The same shape with one plaintext per ciphertext: 256 ciphertexts from a pool of 8, two waves."""
    n = 65536
    ref, hip = mods(n)
    hip.dispatch_notes(reset=True)
    assert _run_plain_pool(hip, ref, n, 3, 31, False, batch=256, pool=8, chunk=200, seed=1618) == 256
    assert "k_mid_cnv (a 16 + b 3 limbs" in hip.dispatch_notes()


_KNOB_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle.ref import RefModule
from poulpy_amd.hal import Module
from tests import test_gpu_mul_plain as T
out = {}
for i, (n, rank, a_size, b_size, res_size, ab, rb, off, abo, bbo) in enumerate(T.PLAIN_GRID):
    ref, hip = RefModule(n), Module(n)
    for shared in (False, True):
        hip.dispatch_notes(reset=True)
        got, want = T._run_plain(hip, ref, n, rank, a_size, b_size, res_size, ab, rb, off, "into", shared, batch=3, seed=n + off + rank, chunk=2,
                                 abo=abo, bbo=bbo)
        assert (n >= 8192 and rb == ab and a_size in (8, 16)) == ("k_mid_cnv_pt" in hip.dispatch_notes()), (n, a_size, b_size)
        out["p%d_%d" % (i, shared)] = got
    rng = np.random.default_rng(n)
    re = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
    im = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
    hip.dispatch_notes(reset=True)
    got, want = T._run_const(hip, ref, n, rank, a_size, res_size, ab, ab, off, "into", re, im, batch=3, seed=n + 5)
    assert "k_mul_const_nz" not in hip.dispatch_notes()
    out["c%d" % i] = got
n = 65536
ref, hip = RefModule(n), Module(n)
for shared, off, chunk in ((True, 36, 160), (False, 31, 200)):
    hip.dispatch_notes(reset=True)
    assert T._run_plain_pool(hip, ref, n, 3, off, shared, batch=256, pool=8, chunk=chunk, seed=1616 + off) == 256
    notes = hip.dispatch_notes()
    assert "k_mid_cnv_pt<16,3>" in notes and "k_mid_cnv (" not in notes, notes
    assert ("shared plaintext" in notes) == shared, notes
np.savez(sys.argv[2], **out)
"""


def test_knobs_force_the_compositions_same_digits(mods, tmp_path):
    """POULPY_DBG_MULPLAIN_FUSED=1 (one k_mid_cnv_pt for all columns instead of the default per-column k_mid_cnv: dispatched on every pipeline
    shape it instantiates, N = 2^16 / 16 limbs / 256 ciphertexts in two waves included) and POULPY_DBG_MULCONST_FUSED=0
    (k_cnv_by_const_batched + normalize + rotate + add instead of k_mul_const_nz), read once per process: a child process with both set gives
    the same digits."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, POULPY_DBG_MULPLAIN_FUSED="1", POULPY_DBG_MULCONST_FUSED="0")
    out = tmp_path / "composed.npz"
    r = subprocess.run([sys.executable, "-c", _KNOB_SCRIPT, root, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    composed = np.load(out)
    for i, (n, rank, a_size, b_size, res_size, ab, rb, off, abo, bbo) in enumerate(PLAIN_GRID):
        ref, hip = mods(n)
        for shared in (False, True):
            got, want = _run_plain(hip, ref, n, rank, a_size, b_size, res_size, ab, rb, off, "into", shared, batch=3, seed=n + off + rank, chunk=2,
                                   abo=abo, bbo=bbo)
            assert np.array_equal(got, want)
            assert np.array_equal(got, composed["p%d_%d" % (i, shared)]), (n, a_size, b_size, shared)
        rng = np.random.default_rng(n)
        re = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
        im = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
        got, want = _run_const(hip, ref, n, rank, a_size, res_size, ab, ab, off, "into", re, im, batch=3, seed=n + 5)
        assert np.array_equal(got, want) and np.array_equal(got, composed["c%d" % i]), (n, a_size)


def test_glwe_mul_plain_n65536_bench_shape(mods):
    """poulpy-bench's shape: the plaintext has the ciphertext's layout, cnv_offset = 0; per-ciphertext plaintexts, assign form."""
    n = 65536
    ref, hip = mods(n)
    got, want = _run_plain(hip, ref, n, 1, 16, 16, 16, 12, 12, 0, "assign", False, batch=3, seed=1617)
    assert np.array_equal(got, want)


def _run_const(hip, ref, n, rank, a_size, res_size, ab, rb, off, mode, re, im, batch, seed, chunk=0, pool=None, a_fill=None):
    """a_fill(t, data, rng): overwrite input t's digits in place (tests/unnormalized.py)"""
    from poulpy_amd.hal import GlweMulConstParams
    rng = seeded(seed)
    cols = rank + 1
    assign = mode == "assign"
    if assign:
        a_size, ab = res_size, rb
    pool = pool or batch
    a_p = np.stack([VecZnx(n, cols, a_size).fill_uniform(ab, rng).data for _ in range(pool)])
    if a_fill is not None:
        for t in range(pool):
            a_fill(t, a_p[t], rng)
    want_p = np.empty((pool, res_size, cols, n), dtype=np.int64)
    for t in range(pool):
        if assign:
            r = VecZnx(n, cols, res_size, a_p[t].copy())
            po.ckks_mul_pt_const_assign(ref, off, r, rb, re, im)
        else:
            r = VecZnx(n, cols, res_size)
            po.ckks_mul_pt_const_into(ref, off, r, rb, VecZnx(n, cols, a_size, a_p[t].copy()), ab, re, im)
        want_p[t] = r.data
    idx = np.arange(batch) % pool
    a_all = np.ascontiguousarray(a_p[idx])
    with on_device(hip) as dev:
        d_a = dev.upload(a_all)
        if assign:
            d_r = d_a
        else:
            d_r = dev.alloc(batch * res_size * cols * n * 8)
        p = GlweMulConstParams(rank=rank, a_size=a_size, a_base2k=ab, res_size=res_size, res_base2k=rb, cnv_offset=off)
        with on_device(hip, chunk=chunk):
            b_size = len(re) if re is not None else (len(im) if im is not None else 0)
            hip.glwe_mul_const_batched(d_r.ptr, None if assign else d_a.ptr, re, im, p, mode, batch, b_size=b_size)
            hip.sync()
        got = d_r.download(np.int64, batch * res_size * cols * n).reshape(batch, res_size, cols, n)
    return got, want_p[idx]


CONST_GRID = [
    (256, 1, 4, 4, 12, 12, 24),    # hi = 1, lo = 0
    (256, 2, 3, 5, 13, 13, 7),     # hi = 0, lo < 0; the assign form truncates res_big to res_size limbs
    (1024, 1, 5, 4, 12, 16, 40),   # cross-base: the per-op composition
    (4096, 2, 6, 6, 12, 12, 0),    # cnv_offset 0
    (4096, 1, 8, 8, 12, 12, 31),   # cnv_offset >= base2k, not a multiple: positive sub-base2k res_offset (lsh > 0)
]


@pytest.mark.parametrize("arms", ["re", "im", "both", "none"])
@pytest.mark.parametrize("mode", ["into", "assign"])
@pytest.mark.parametrize("case", CONST_GRID)
def test_glwe_mul_const_batched(mods, case, mode, arms):
    n, rank, a_size, res_size, ab, rb, off = case
    if mode == "assign" and rb != ab:
        pytest.skip("the assign form has one base2k (operations/glwe.rs:111)")
    ref, hip = mods(n)
    rng = seeded(n + off)
    re = rng.integers(-(1 << 40), 1 << 40, 3, dtype=np.int64) if arms in ("re", "both") else None
    im = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64) if arms in ("im", "both") else None
    hip.dispatch_notes(reset=True)
    got, want = _run_const(hip, ref, n, rank, a_size, res_size, ab, rb, off, mode, re, im, batch=5, seed=n + rank + off, chunk=2)
    assert np.array_equal(got, want), (case, mode, arms)
    if ab == rb and arms != "none":
        assert "k_mul_const_nz" in hip.dispatch_notes()


def test_glwe_mul_const_n65536_two_waves(mods):
    """N = 2^16, rank 1, 16 limbs, base2k 12, a 3-digit complex constant, 64 ciphertexts from a pool of 4, second wave by set_chunk."""
    n = 65536
    ref, hip = mods(n)
    rng = seeded(2024)
    re = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
    im = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
    hip.dispatch_notes(reset=True)
    got, want = _run_const(hip, ref, n, 1, 16, 16, 12, 12, 3 * 12, "into", re, im, batch=64, seed=2025, chunk=40, pool=4)
    assert np.array_equal(got, want)
    assert "k_mul_const_nz" in hip.dispatch_notes()


def test_refusals(mods):
    """Every refusal is a status (PoulpyHipError), before anything touches the device."""
    from poulpy_amd.hal import GlweMulConstParams, GlweTensorParams, PoulpyHipError
    n = 256
    _, hip = mods(n)
    cols, size = 2, 3
    with on_device(hip) as dev:
        d_a = dev.alloc(n * cols * size * 8, poison=False)
        d_r = dev.alloc(n * cols * size * 8, poison=False)
        d_pt = dev.alloc(n * size * 8, poison=False)
        host = np.zeros((size, cols, n), dtype=np.int64)
        good = dict(rank=1, a_size=size, b_size=size, ab_base2k=12, a_effective_k=36, b_effective_k=36, res_size=size, res_base2k=12, cnv_offset=12)
        bad = [dict(rank=0), dict(a_size=0), dict(ab_base2k=0), dict(res_base2k=64), dict(a_effective_k=40), dict(b_effective_k=20),
               dict(cnv_offset=12 * 12)]
        for d in bad:
            with pytest.raises(PoulpyHipError):
                hip.glwe_mul_plain_batched(d_r.ptr, d_a.ptr, d_pt.ptr, False, GlweTensorParams(**{**good, **d}), "into", 1)
        p = GlweTensorParams(**good)
        for (r, a, pt, mode) in ((host.ctypes.data, d_a.ptr, d_pt.ptr, "into"), (d_r.ptr, host.ctypes.data, d_pt.ptr, "into"),
                                 (d_r.ptr, d_a.ptr, host.ctypes.data, "into"), (d_r.ptr, d_r.ptr, d_pt.ptr, "into"), (d_r.ptr, None, d_r.ptr, "assign"),
                                 (d_r.ptr, d_a.ptr, d_pt.ptr, "assign")):
            with pytest.raises(PoulpyHipError):
                hip.glwe_mul_plain_batched(r, a, pt, False, p, mode, 1)
        hip.glwe_mul_plain_batched(d_r.ptr, d_a.ptr, d_pt.ptr, False, p, "into", 0)   # batch 0: a no-op
        cgood = dict(rank=1, a_size=size, a_base2k=12, res_size=size, res_base2k=12, cnv_offset=12)
        b = np.array([3, -2], dtype=np.int64)
        for d in (dict(rank=0), dict(res_size=0), dict(a_base2k=64), dict(cnv_offset=12 * 10)):
            with pytest.raises(PoulpyHipError):
                hip.glwe_mul_const_batched(d_r.ptr, d_a.ptr, b, None, GlweMulConstParams(**{**cgood, **d}), "into", 1)
        cp = GlweMulConstParams(**cgood)
        for (r, a, mode) in ((host.ctypes.data, d_a.ptr, "into"), (d_r.ptr, host.ctypes.data, "into"), (d_r.ptr, d_r.ptr, "into"),
                             (d_r.ptr, d_a.ptr, "assign")):
            with pytest.raises(PoulpyHipError):
                hip.glwe_mul_const_batched(r, a, b, None, cp, mode, 1)


@pytest.mark.parametrize("n,b_size,off", [(65536, 3, 36), (4096, 8, 0), (1024, 3, 31)])
def test_rounding_margin_of_the_plaintext_paths(mods, n, b_size, off):
    """The rounding margin (max |x - round(x)| of the inverse transforms) stays below 0.05 on the pipeline path and on the per-op path."""
    from poulpy_amd.hal import GlweTensorParams
    _, hip = mods(n)
    rng = seeded(n + b_size)
    cols, size, k, batch = 2, 16 if n == 65536 else 8, 12, 4
    a = np.stack([VecZnx(n, cols, size).fill_uniform(k, rng).data for _ in range(batch)])
    pt = VecZnx(n, 1, b_size).fill_uniform(k, rng).data
    with on_device(hip) as dev:
        d_a = dev.upload(a)
        d_pt = dev.alloc(pt.nbytes, poison=False).upload(np.ascontiguousarray(pt))
        d_r = dev.alloc(a.nbytes, poison=False)
        p = GlweTensorParams(rank=1, a_size=size, b_size=b_size, ab_base2k=k, a_effective_k=size * k, b_effective_k=b_size * k, res_size=size,
                             res_base2k=k, cnv_offset=off)
        margin = hip.rounding_margin_of(lambda: hip.glwe_mul_plain_batched(d_r.ptr, d_a.ptr, d_pt.ptr, True, p, "into", batch))
    assert 0.0 < margin < 0.05, margin
