"""GPU parity on UN-NORMALIZED inputs: digits wider than base2k, as a ciphertext holds them after additions without a normalize
(poulpy-core api/operations.rs: glwe_add_into / _sub / _negate never normalize).  The reference computes the right answer from any i64
limbs as long as its f64 rounding stays exact, and the backend must give the same bits.  Several device paths keep 16- or 32-bit copies
of digits that are normalized when the input is (the spectral automorphism's body operand and pass 1's side copy, raising a `wide` flag
otherwise; the blind rotation's and the tensor's accumulators, which come out of a normalizing tail).  Every other batched test draws
normalized digits, so a path that truncated or mis-flagged a wide input would pass the rest of the suite.

Inputs come from tests/unnormalized.py (classes 1-4, each checked for the property it claims).  Every case compares every i64 limb with
the C oracle.  Exactness guard for the FFT-based cases: the device's and the oracle's rounding margins stay below STRUCTURED_MARGIN_MAX
(as tests/test_gpu_structured.py), and the dsize-1 external products and key switches also equal the exact integer product, so that a
mismatch means a wrong kernel and not two inexact f64 results.  The margins reached are printed (`-s`)."""
import os
import sys

import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import unnormalized as un
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded
from tests.test_gpu_cnv import _run_mul_relinearize, _run_relinearize, _run_tensor
from tests.test_gpu_mul_plain import _run_const, _run_plain
from tests.test_gpu_parity import _run_blind_rotation, _run_glwe_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

STRUCTURED_MARGIN_MAX = 0.25


def _check_margins(label, gpu_margin, oracle_margin):
    print(f"[margin] {label}: gpu {gpu_margin:.3g} oracle {oracle_margin:.3g}")
    assert gpu_margin < STRUCTURED_MARGIN_MAX and oracle_margin < STRUCTURED_MARGIN_MAX, (label, gpu_margin, oracle_margin)


def _margins_of(hip, ref, run):
    """Runs `run() -> (got, want)` once more with both margin probes on; the results must agree there too.  -> (gpu, oracle) margins."""
    box = {}

    def checked():
        got, want = run()
        assert np.array_equal(got, want), "differs under the margin probe"
    gpu = hip.rounding_margin_of(lambda: box.__setitem__("oracle", ref.rounding_margin_of(checked)))
    return gpu, box["oracle"]


def _exact_glwe(ks, a, mat, base2k, res_size):
    """The exact result of a dsize-1 external product (ks False) or key switch (ks True) with one base2k: integer products, then a big-int
    normalize (tools/structured.py, oracle/exact.py)."""
    import structured as st
    from oracle.exact import normalize_exact
    if not ks:
        assert a.shape[0] == res_size
        return st.exact_external_product(a, mat, base2k)
    big = st.exact_vmp_big(np.ascontiguousarray(a[:, 1:]), mat)
    big[:a.shape[0], 0] += a[:, 0]
    out = np.empty((res_size, mat.shape[3], a.shape[-1]), dtype=np.int64)
    for c in range(mat.shape[3]):
        out[:, c] = normalize_exact(big[:, c], base2k, res_size)
    return out


def _variants(base2k, smax, index_wave1, batch):
    """Classes 1-3 at base2k: sums of 2^s (s <= smax), one wide ciphertext in the second wave and in wave 0, wide in one place only."""
    v = [un.sums(base2k, s) for s in (1, 2, 4, 6) if s <= smax]
    v += [un.one_wide(index_wave1, base2k, min(4, smax)), un.one_wide(0, base2k, min(4, smax))]
    v += [un.wide_at(w, base2k, min(4, smax), index=(batch - 1 if w == "top" else None)) for w in un.PLACES]
    return v


# (N, limbs, batch, chunk, knob): knob "small-on" / "small-off" (N = 4096, set_small_path), "fused" / "unfused" (set_fusion), None
GLWE_SHAPES = [
    (1024, 3, 4, 2, None), (2048, 3, 4, 2, None),
    (4096, 3, 4, 2, "small-on"), (4096, 3, 4, 2, "small-off"),
    (8192, 4, 4, 2, "fused"), (8192, 4, 4, 2, "unfused"),
    (65536, 8, 3, 2, None),
]


@pytest.mark.parametrize("ks", [False, True], ids=["external_product", "keyswitch"])
@pytest.mark.parametrize("shape", GLWE_SHAPES, ids=lambda s: f"n{s[0]}-{s[4] or 'default'}")
def test_external_product_and_keyswitch_on_unnormalized_input(mods, shape, ks):
    n, limbs, batch, chunk, knob = shape
    ref, hip = mods(n)
    base2k = 12
    smax = 4 if n == 65536 else 6
    variants = _variants(base2k, smax, 2, batch)
    fuse = (False, False) if knob == "unfused" else (True, True)
    case = 0
    with on_device(hip, small_path=knob != "small-off"):
        for j, (rank, dsize) in enumerate(((1, 1), (2, 1), (1, 2), (2, 2))):
            # rank 1, dsize 1: every input variant (N = 2^16: every third); the other pairs: every third one, in turn
            for i in (range(len(variants)) if j == 0 and n < 65536 else range(j % 3, len(variants), 3)):
                fill = variants[i]
                dnum = limbs if dsize == 1 else -(-limbs // 2)
                out = {}
                hip.dispatch_notes(reset=True)
                got, want = _run_glwe_op(hip, ref, ks, n, rank, rank, limbs, base2k, limbs, base2k, dnum, dsize, limbs, base2k, batch=batch,
                                         seed=9000 + case + n, chunk=chunk, fuse=fuse, a_fill=fill, out=out)
                notes = out["notes"]   # (the main call's: the margin-probe rerun may take another path)
                case += 1
                label = (n, knob, "ks" if ks else "ep", rank, dsize, fill.label)
                assert np.array_equal(got, want), label
                _check_margins(label, out["gpu_margin"], out["oracle_margin"])
                if n <= 2048 and not ks and (rank, dsize) == (1, 1):
                    assert "k_small_one" in notes, (label, notes)
                if knob in ("fused", "small-off") or n == 65536:
                    assert "k_mid128" in notes, (label, notes)
                if knob == "unfused" or (knob == "small-on" and (rank, dsize) == (1, 1)):
                    assert "k_mid128" not in notes, (label, notes)   # (small-on: the two-kernel path of device_small.hpp)
                if dsize == 1 and np.abs(out["a"]).max() < (1 << 20) and (n < 65536 or rank == 1):
                    for b in (range(batch) if n < 65536 else (2,)):   # (N = 2^16: the ciphertext of the second wave)
                        exact = _exact_glwe(ks, out["a"][b], out["mat"], base2k, limbs)
                        assert np.array_equal(want[b], exact), (label, b, "oracle != exact")
                    print(f"[exact] {label}: gpu == oracle == exact product")


@pytest.mark.parametrize("mode", ["automorphism", "add", "sub", "sub_negate"])
@pytest.mark.parametrize("n,rank,knob", [(1024, 1, None), (2048, 1, None), (2048, 2, None), (4096, 1, None), (4096, 2, None),
                                         (8192, 1, None), (8192, 1, "unfused"), (8192, 2, None), (65536, 1, None), (65536, 2, None)])
def test_automorphism_family_on_unnormalized_input(mods, n, rank, knob, mode):
    """The paths test_glwe_automorphism_body_as_16_bit_copies_and_wide_inputs leaves out: N <= 2048 (small-ring path), N = 4096, fusion off,
    wide digits in a mask column only (rank 1 fused, N >= 8192, add / sub forms: pass 1's 16-bit side copy of the mask column is then the
    only thing that can raise the wide flag; rank 2: a body-less column), and a wide ciphertext in wave 0 with normalized ones after it
    (the flag raised, consumed and reset per wave).  Every width reaches past 16 bits; Galois elements = 1 mod 4 and = 3 mod 4."""
    ref, hip = mods(n)
    base2k = 12 if n != 4096 else 14
    limbs = 3 if n < 65536 else 4
    fuse = (False, False) if knob == "unfused" else (True, True)
    s = 17 - base2k      # digits up to +-2^16
    fills = [un.sums(base2k, s), un.one_wide(2, base2k, s), un.one_wide(0, base2k, s), un.wide_at("mask", base2k, s), un.wide_at("body", base2k, s)]
    for p in ((5, -5) if n < 65536 else (5,)):
        for fill in fills:
            out = {}
            got, want = _run_glwe_op(hip, ref, True, n, rank, rank, limbs, base2k, limbs, base2k, limbs, 1, limbs, base2k, batch=4 if n < 65536 else 3,
                                     seed=9500 + n + rank + p, chunk=2, fuse=fuse, auto=(p % (2 * n), mode), a_fill=fill, out=out)
            label = (n, rank, knob, mode, p, fill.label)
            assert np.array_equal(got, want), label
            _check_margins(label, out["gpu_margin"], out["oracle_margin"])


def _run_trace(hip, ref, n, rank, size, k, nsteps, batch, seed, fill, chunk=0):
    from poulpy_amd.hal import GlweOpParams
    rng = seeded(seed)
    cols, dnum, key_size = rank + 1, size, size
    gals = [-1] + [pow(5, 1 << i, 2 * n) for i in range(nsteps - 1)]
    with on_device(hip) as dev:
        prs, d_keys = [], []
        for _ in gals:
            pr, ph = prepared_key(ref, hip, MatZnx(n, dnum, rank, cols, key_size).fill_uniform(k, rng))
            prs.append(pr)
            d_keys.append(dev.key(ph))
        cts = np.empty((batch, size, cols, n), dtype=np.int64)
        want = np.empty_like(cts)
        oracle_margin = 0.0
        for b in range(batch):
            ct = VecZnx(n, cols, size).fill_uniform(k, rng)
            fill(b, ct.data, rng)
            cts[b] = ct.data
            oracle_margin = max(oracle_margin, ref.rounding_margin_of(lambda: ref.glwe_trace_assign(ct, k, gals, prs)))
            want[b] = ct.data
        p = GlweOpParams(rank=rank, dnum=dnum, dsize=1, key_size=key_size, key_base2k=k, a_size=size, a_base2k=k, res_size=size, res_base2k=k,
                         rank_out=rank)
        d_res = dev.upload(cts)
        with on_device(hip, chunk=chunk):
            hip.glwe_trace_batched(d_res.ptr, gals, [d.ptr for d in d_keys], p, batch)
            hip.sync()
            got = d_res.download(np.int64, want.size).reshape(want.shape)
            d_res.upload(cts)
            gpu_margin = hip.rounding_margin_of(lambda: hip.glwe_trace_batched(d_res.ptr, gals, [d.ptr for d in d_keys], p, batch))
    return got, want, gpu_margin, oracle_margin


@pytest.mark.parametrize("k", [12, 14])
@pytest.mark.parametrize("n", [512, 8192, 65536])
def test_trace_on_unnormalized_input(mods, n, k):
    """glwe_trace with input digits of 2^15 and more at base2k <= 14: the steps take the 16-bit body operand there (want_rsh), which is
    only right if what reaches them is normalized.  Whole batch wide, and one wide ciphertext in the second wave."""
    ref, hip = mods(n)
    size, nsteps = (3, 3) if n < 65536 else (4, 2)
    s = 16 - k + 1       # digits up to +-2^16
    for fill in (un.sums(k, s), un.one_wide(2, k, s), un.wide_at("body", k, s), un.wide_at("bottom", k, s)):
        got, want, gm, om = _run_trace(hip, ref, n, 1, size, k, nsteps, batch=4 if n < 65536 else 3, seed=n + k, fill=fill, chunk=2)
        label = (n, k, fill.label)
        assert np.array_equal(got, want), label
        _check_margins(label, gm, om)


@pytest.mark.parametrize("mode", ["apply", "square", "add_assign"])
@pytest.mark.parametrize("n", [8192, 65536])
def test_tensor_on_unnormalized_operands(mods, n, mode):
    """glwe_tensor_apply / _square / _add_assign at base2k 12 and 14 (the compact 16-bit tensor of the fused multiply) and 16 (the d16 copies of
    the diagonal terms): one operand wide, then both."""
    ref, hip = mods(n)
    sizes = (4, 3, 5) if n == 8192 else (4, 4, 6)
    for k in (12, 14, 16):
        off = k + 2
        for which in ("a", "both"):
            fa = un.sums(k, 17 - k)      # digits up to +-2^16: beyond the 16-bit copies
            fb = un.one_wide(1, k, 17 - k) if which == "both" else None

            def run():
                return _run_tensor(hip, ref, n, 1, *sizes, k, k, off, mode, batch=3, seed=n + k + len(which), chunk=2, a_fill=fa, b_fill=fb)
            hip.dispatch_notes(reset=True)
            got, want = run()
            notes = hip.dispatch_notes()
            label = (n, mode, k, which)
            assert np.array_equal(got, want), label
            if n == 8192:    # the fused row pass (test_gpu_cnv.py: test_glwe_tensor_apply_fused_row_pass)
                assert "k_mid_cnv" in notes, (label, notes)
            _check_margins(label, *_margins_of(hip, ref, run))


@pytest.mark.parametrize("n", [8192, 65536])
def test_relinearize_and_mul_relinearize_on_unnormalized_input(mods, n):
    ref, hip = mods(n)
    for k in (12, 14, 16):
        limbs = 4
        for mode in ("apply", "square"):
            def run():
                return _run_mul_relinearize(hip, ref, n, 1, limbs, limbs, limbs + 1, k, k, limbs + 1, k, limbs + 1, 1, limbs, k, mode, batch=3,
                                            seed=n + k, chunk=2, a_fill=un.sums(k, 17 - k), b_fill=un.wide_at("top", k, 17 - k))
            got, want = run()
            label = ("mul_relinearize", n, k, mode)
            assert np.array_equal(got, want), label
            _check_margins(label, *_margins_of(hip, ref, run))

        def run_relin():
            return _run_relinearize(hip, ref, n, 1, limbs, k, limbs + 1, k, limbs, 1, limbs, k, batch=3, seed=n + k + 1, chunk=2,
                                    a_fill=un.sums(k, 17 - k))
        got, want = run_relin()
        assert np.array_equal(got, want), ("relinearize", n, k)
        _check_margins(("relinearize", n, k), *_margins_of(hip, ref, run_relin))


@pytest.mark.parametrize("shared", [False, True], ids=["per_ct", "shared"])
@pytest.mark.parametrize("case", [(8192, 1, 8, 3, 8, 12, 12, 31, 0, 0), (4096, 1, 6, 3, 6, 12, 12, 29, 0, 0), (1024, 2, 5, 3, 5, 12, 12, 31, 0, 2)])
def test_mul_plain_on_unnormalized_input(mods, case, shared):
    """a wide ciphertext, then separately a wide plaintext"""
    n, rank, a_size, b_size, res_size, ab, rb, off, abo, bbo = case
    ref, hip = mods(n)
    for (fa, fp) in ((un.sums(ab, 4), None), (None, un.sums(ab, 4)), (un.one_wide(2, ab, 6), None)):
        def run():
            return _run_plain(hip, ref, n, rank, a_size, b_size, res_size, ab, rb, off, "into", shared, batch=4, seed=n + off, chunk=2,
                              abo=abo, bbo=bbo, a_fill=fa, pt_fill=fp)
        got, want = run()
        label = (case, shared, fa and fa.label, fp and fp.label)
        assert np.array_equal(got, want), label
        _check_margins(label, *_margins_of(hip, ref, run))


@pytest.mark.parametrize("n,rank,n_lwe,blk,dnum,bsz,rsz,k,batch", [
    (512, 3, 6, 3, 1, 2, 1, 18, 5),         # the `ref` shape: the one-kernel rotation (k_br_fused asserted)
    (1024, 2, 6, 3, 3, 3, 3, 13, 5),        # rank 2 at N = 1024, N = 2048: the small-ring path (k_br_block asserted); by
    (2048, 1, 8, 4, 2, 2, 2, 14, 4),        #   api_br.hip's conditions, 16-bit accumulator digits between blocks (base2k <= 15)
    (16384, 1, 6, 2, 2, 2, 2, 13, 3),       # the pipeline (k_mid128<.., BR=1> asserted); 16-bit digits between blocks by its conditions (base2k <= 15)
    (16384, 1, 6, 3, 2, 2, 2, 17, 3),       # the pipeline; 32-bit digits between blocks (base2k 17)
])
def test_blind_rotation_on_an_unnormalized_test_vector(mods, n, rank, n_lwe, blk, dnum, bsz, rsz, k, batch):
    """X^b * LUT reaches the first block as any i64; later blocks read the accumulator as 16- or 32-bit digits, which is right only because the
    first block's tail normalizes."""
    ref, hip = mods(n)
    s = 3 if k <= 14 else 1
    for fill in (un.sums(k, s), un.wide_at("top", k, s + 1), un.wide_at("bottom", k, s + 1)):
        out = {}
        hip.dispatch_notes(reset=True)
        got, want = _run_blind_rotation(hip, ref, n, rank, n_lwe, blk, dnum, bsz, rsz, k, batch=batch, seed=n + k + blk, lut_fill=fill, out=out)
        notes = out["notes"]
        label = (n, rank, blk, k, fill.label)
        assert np.array_equal(got, want), label
        if n == 512:
            assert "k_br_fused" in notes, (label, notes)
        elif n <= 2048:
            assert "k_br_block" in notes and "k_br_fused" not in notes, (label, notes)
        else:
            assert "BR=1" in notes, (label, notes)
        _check_margins(label, out["gpu_margin"], out["oracle_margin"])


def test_mul_const_on_unnormalized_input(mods):
    for (n, rank, a_size, res_size, ab, rb, off) in ((256, 1, 4, 4, 12, 12, 24), (4096, 1, 8, 8, 12, 12, 31), (1024, 1, 5, 4, 12, 16, 40)):
        ref, hip = mods(n)
        rng = seeded(n + off)
        re = [int(x) for x in rng.integers(-(1 << 11), 1 << 11, 3)]
        im = [int(x) for x in rng.integers(-(1 << 11), 1 << 11, 3)]
        got, want = _run_const(hip, ref, n, rank, a_size, res_size, ab, rb, off, "into", re, im, batch=4, seed=n + off, chunk=2)
        assert np.array_equal(got, want)
        for fill in (un.sums(ab, 6), un.one_wide(2, ab, 8), un.full_range_fill()):
            got, want = _run_const(hip, ref, n, rank, a_size, res_size, ab, rb, off, "into", re, im, batch=4, seed=n + off, chunk=2, a_fill=fill)
            assert np.array_equal(got, want), (n, fill.label)


@pytest.mark.parametrize("negate", [False, True])
def test_mod_switch_2n_on_full_range_limbs(mods, negate):
    ref, hip = mods(256)
    rng = seeded(77 + negate)
    for (n2, base2k, size) in ((2048, 17, 2), (2048, 12, 2), (1 << 15, 13, 3), (64, 7, 1)):
        batch, n_lwe = 5, 101
        lwe = un.full_range(rng, (batch, size, n_lwe + 1))
        want = np.stack([ref.mod_switch_2n(n2, lwe[b], base2k, negate) for b in range(batch)])
        with on_device(hip) as dev:
            d_l = dev.upload(lwe)
            d_r = dev.alloc(want.nbytes, poison=False)
            hip.lwe_mod_switch_2n_batched(d_r.ptr, d_l.ptr, n_lwe, size, base2k, n2, negate, batch)
            hip.sync()
            got = d_r.download(np.int64, want.size).reshape(want.shape)
        assert np.array_equal(got, want), (n2, base2k, size, negate)


@pytest.mark.parametrize("n,n_lwe", [(256, 100), (4096, 77)])
def test_sample_extract_on_full_range_limbs(mods, n, n_lwe):
    ref, hip = mods(n)
    rng = seeded(n + 5)
    for cols, a_size, res_size, batch in ((2, 3, 3, 5), (3, 2, 4, 2)):
        a = un.full_range(rng, (batch, a_size, cols, n))
        want = np.stack([ref.lwe_sample_extract(n_lwe, res_size, VecZnx(n, cols, a_size, a[b].copy())) for b in range(batch)])
        with on_device(hip) as dev:
            d_a = dev.upload(a)
            d_r = dev.alloc(want.nbytes, poison=False)
            hip.lib.pz_memset_d(hip.handle, d_r.ptr, 0x33, want.nbytes)
            hip.lwe_sample_extract_batched(d_r.ptr, n_lwe, res_size, d_a.ptr, cols, a_size, batch)
            hip.sync()
            got = d_r.download(np.int64, want.size).reshape(want.shape)
        assert np.array_equal(got, want), (n, cols, a_size, res_size)


@pytest.mark.parametrize("n", [32, 65536])
def test_vec_znx_limbwise_family_on_full_range_limbs(mods, n):
    """add / sub / negate / copy with INT64_MIN, INT64_MAX and +-2^62 among the operands: the reference's wrapping arithmetic"""
    ref, hip = mods(n)
    rng = seeded(6100 + n)
    a = VecZnx(n, 2, 3, un.full_range(rng, (3, 2, n)))
    b = VecZnx(n, 3, 2, un.full_range(rng, (2, 3, n)))
    b.data[0, 2, :un.EDGES.size] = un.EDGES[::-1]
    for name in ("vec_znx_add_into", "vec_znx_sub"):
        r1 = VecZnx(n, 2, 3)
        r2 = r1.copy()
        getattr(ref, name)(r1, 1, a, 0, b, 2)
        getattr(hip, name)(r2, 1, a, 0, b, 2)
        assert np.array_equal(r1.data, r2.data), name
    for name in ("vec_znx_add_assign", "vec_znx_sub_assign", "vec_znx_sub_negate_assign", "vec_znx_negate", "vec_znx_copy"):
        r1 = VecZnx(n, 2, 3, un.full_range(rng, (3, 2, n)))
        r2 = r1.copy()
        getattr(ref, name)(r1, 0, a, 1)
        getattr(hip, name)(r2, 0, a, 1)
        assert np.array_equal(r1.data, r2.data), name


def _margins_around(hip, ref, check):
    """Runs the parity check `check()` once more with both margin probes on (its assertions hold there too).  -> (gpu, oracle) margins."""
    box = {}
    gpu = hip.rounding_margin_of(lambda: box.__setitem__("oracle", ref.rounding_margin_of(check)))
    return gpu, box["oracle"]


def _parity_and_margins(hip, ref, label, check):
    check()
    _check_margins(label, *_margins_around(hip, ref, check))


@pytest.mark.parametrize("s", [2, 4])
def test_composites_on_unnormalized_input(mods, s):
    """The loops over GLWE products, one shape each (the parity tests of test_gpu_parity.py with wide input digits): ggsw_external_product,
    ggsw_expand_row (five-kernel path and the fused pipeline), ggsw_from_gglwe, glwe_pack (five-kernel path and the fused automorphism
    pipeline)."""
    from tests import test_gpu_parity as tp
    _parity_and_margins(mods(256)[1], mods(256)[0], ("ggsw_external_product", s), lambda: tp.test_ggsw_external_product(mods, fill=un.sums(13, s)))
    for args in ((256, 1, 3, 4, 4, 4, 13, 1, 1), (4096, 1, 2, 4, 4, 4, 14, 1, 3)):
        ref, hip = mods(args[0])
        _parity_and_margins(hip, ref, ("ggsw_expand_row", args[0], s),
                            lambda: tp.test_ggsw_expand_row_batched(mods, *args, fill=un.sums(args[6], s)))
    ref, hip = mods(4096)
    _parity_and_margins(hip, ref, ("ggsw_from_gglwe", s), lambda: tp.test_ggsw_from_gglwe_batched(mods, 4096, 2, 2, fill=un.sums(13, s)))
    for args in ((64, 1, 3, 0, [0, 5, 17, 32, 33, 63], 3), (4096, 1, 3, 9, [0, 512, 1024, 2048, 3584], 2)):
        ref, hip = mods(args[0])
        _parity_and_margins(hip, ref, ("glwe_pack", args[0], s), lambda: tp.test_glwe_pack_batched(mods, *args, fill=un.one_wide(1, 13, s)))


@pytest.mark.parametrize("fuse", [True, False], ids=["one-kernel", "composed"])
def test_extended_blind_rotation_on_unnormalized_test_vectors(mods, fuse):
    from tests import test_gpu_parity as tp
    n = 512
    ref, hip = mods(n)
    _parity_and_margins(hip, ref, ("extended blind rotation", fuse),
                        lambda: tp.test_blind_rotation_extended(mods, n, 2, 8, 4, 2, 3, 2, 3, 3, fuse, fill=un.sums(13, 3)))


@pytest.mark.parametrize("s", [3, 6])
def test_lwe_conversions_on_unnormalized_input(mods, s):
    """glwe_from_lwe (embedding + key switch) with wide LWE limbs, lwe_from_glwe (key switch + extraction) with wide GLWE digits.  Both run an
    FFT product after the embedding, so they take class 1 rather than full-range limbs (those would leave f64's exact range)."""
    from tests import test_gpu_lwe as tl
    for args in ((256, 100, 3, 12, 12, 1), (4096, 700, 2, 17, 12, 1)):
        ref, hip = mods(args[0])
        _parity_and_margins(hip, ref, ("glwe_from_lwe", args, s), lambda: tl.test_glwe_from_lwe(mods, *args, fill=un.sums(args[3], s)))
    for args in ((256, 1, 0, 100), (4096, 2, 4095, 33)):
        ref, hip = mods(args[0])
        _parity_and_margins(hip, ref, ("lwe_from_glwe", args, s), lambda: tl.test_lwe_from_glwe(mods, *args, fill=un.sums(12, s)))
