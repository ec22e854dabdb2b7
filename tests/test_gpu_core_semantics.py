"""The encrypt / operate / decrypt procedures of tests/core_cases.py through the batched device entry points.

Every case runs a batch of 3 ciphertexts, each with its own plaintext, so that a mixed-up batch index shows; it checks the device output
against the oracle bit for bit, then decrypts every output under the secret key (tests/fhe_sk.py) against its own plaintext and the
reference's noise bound.  The negative controls go through the same calls: device == oracle, and the decryption fails.  The shapes are
the routes of tests/test_gpu_unnormalized.py (small-ring kernel, N = 4096 small path on / off, N = 8192 fused / unfused, N = 2^16 at the
headline shape and a 16-limb automorphism) with their dispatch notes, and both sides of the spectral automorphism's 16-bit body gate.
noise_have / noise_want are printed (`-s`)."""
import numpy as np
import pytest

from tests import core_cases as cs
from tests import fhe_sk as fs
from tests.device import mods, on_device  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH = 3


def _device(hip, c, in_place=False, fuse=(True, True), chunk=0):
    """One batched call on the case's ciphertexts -> (outputs, dispatch notes)."""
    from poulpy_amd.hal import GlweOpParams
    rows, cols_in, ksz, cols_out, n = c.key.shape
    ph = cs.prepare(hip, c.key)
    a_all = np.ascontiguousarray(c.a)
    shape = (a_all.shape[0], c.res_size, cols_out, n)
    nbytes = int(np.prod(shape)) * 8
    p = GlweOpParams(rank=c.rank, dnum=rows, dsize=c.dsize, key_size=ksz, key_base2k=c.key_base2k, a_size=a_all.shape[1],
                     a_base2k=c.a_base2k, res_size=c.res_size, res_base2k=c.res_base2k, rank_out=c.rank_out)
    with on_device(hip, chunk=chunk, fuse=fuse) as dev:
        d_a, d_key = dev.upload(a_all), dev.key(ph)
        if in_place:
            assert a_all.shape == shape
            d_res = d_a
        else:
            d_res = dev.alloc(nbytes)
        hip.dispatch_notes(reset=True)
        if c.op == "auto":
            hip.glwe_automorphism_batched(d_res.ptr, d_a.ptr, d_key.ptr, p, c.p % (2 * n), c.mode, len(a_all))
        elif c.op == "ks":
            hip.glwe_keyswitch_batched(d_res.ptr, d_a.ptr, d_key.ptr, p, len(a_all))
        else:
            hip.glwe_external_product_batched(d_res.ptr, d_a.ptr, d_key.ptr, p, len(a_all))
        hip.sync()
        got = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
        notes = hip.dispatch_notes()
    return got, notes


def _run(ref, hip, label, c, in_place=False, fail=False, **kw):
    got, notes = _device(hip, c, in_place=in_place, **kw)
    want = cs.run_oracle(ref, c)
    assert np.array_equal(got, want), (label, "device != oracle")
    cs.check(label, c, got, fail=fail)
    return notes


@pytest.mark.parametrize("kind", ["ep", "ep_assign", "ks", "ks_assign", "auto", "auto_assign"])
def test_reference_procedures_on_device(mods, kind):
    """The reference's own loops (N = 256, base2k 17) through the batched entry points, in place for the assign forms."""
    ref, hip = mods(cs.N)
    for label, c, in_place in cs.reference_cases(kind, batch=BATCH):
        _run(ref, hip, label, c, in_place=in_place)


def test_negative_controls_fail_on_device(mods):
    ref, hip = mods(cs.N)
    for label, c, in_place in cs.control_cases(batch=BATCH):
        _run(ref, hip, label, c, in_place=in_place, fail=True)


def _shape_case(op, n, rank, limbs, base2k, seed, mode="automorphism", p=cs.P_AUTO):
    """One base2k for input, key and output; k = limbs base2k, dnum = limbs, dsize 1 (the routes' shapes)."""
    k = limbs * base2k
    if op == "ep":
        return cs.external_product_case(n, rank, 1, limbs, base2k, base2k, base2k, k, k, k, base2k, BATCH, seed)
    if op == "ks":
        return cs.keyswitch_case(n, rank, rank, 1, limbs, base2k, base2k, base2k, k, k, k, BATCH, seed)
    assert op == "auto"
    return cs.automorphism_case(n, rank, 1, limbs, base2k, base2k, base2k, k, k, k, 1, BATCH, seed, mode=mode, p=p)


# (N, limbs, base2k, knob): the routes of tests/test_gpu_unnormalized.py GLWE_SHAPES
SHAPES = [(1024, 3, 12, None), (2048, 3, 12, None), (4096, 3, 12, "small-on"), (4096, 3, 12, "small-off"), (8192, 4, 12, "fused"),
          (8192, 4, 12, "unfused"), (65536, 8, 12, None)]
BODY16 = "spectral tail: 16-bit body operand"
P_SPECTRAL = 5   # = 1 mod 4: the fused pipeline folds the permutation into the middle kernel (k_mid128<.., PERM=1>) and the spectral tail


@pytest.mark.parametrize("op,mode", [("ep", None), ("ks", None), ("auto", "automorphism"), ("auto", "add")])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}-{s[3] or 'default'}")
def test_routes_decrypt(mods, shape, op, mode):
    n, limbs, base2k, knob = shape
    ref, hip = mods(n)
    fuse = (False, False) if knob == "unfused" else (True, True)
    # the spectral automorphism from N = 4096 on the fused pipeline; its 16-bit body operand where the tail's plan has that form (N >= 8192 here)
    perm = op == "auto" and knob not in ("unfused", "small-on") and n >= 4096
    body16 = perm and n >= 8192
    with on_device(hip, small_path=knob != "small-off"):
        for in_place in (False, True):
            c = _shape_case(op, n, 1, limbs, base2k, seed=n + limbs + int(in_place) + 7 * len(mode or op), mode=mode or "automorphism",
                            p=P_SPECTRAL)
            label = (n, knob, op, mode, "in place" if in_place else "out of place")
            notes = _run(ref, hip, label, c, in_place=in_place, fuse=fuse, chunk=2)
            if n <= 2048 and op == "ep":
                assert "k_small_one" in notes, (label, notes)
            if knob in ("fused", "small-off") or n == 65536:
                assert "k_mid128" in notes, (label, notes)
            if knob == "unfused" or (knob == "small-on" and op != "auto"):
                assert "k_mid128" not in notes, (label, notes)
            assert ("PERM=1" in notes) == perm and (BODY16 in notes) == body16, (label, notes)


@pytest.mark.parametrize("mode", ["automorphism", "add"])
def test_automorphism_16_limbs_n65536(mods, mode):
    """configs[4] shape: N = 2^16, 16 limbs, base2k 12, on the spectral path."""
    ref, hip = mods(65536)
    c = _shape_case("auto", 65536, 1, 16, 12, seed=1616, mode=mode, p=P_SPECTRAL)
    notes = _run(ref, hip, (65536, 16, mode), c)
    assert "k_mid128" in notes and "PERM=1" in notes and BODY16 in notes, notes


@pytest.mark.parametrize("key_base2k", [14, 15, 16, 17])
@pytest.mark.parametrize("mode", ["automorphism", "add"])
def test_automorphism_body_operand_gate(mods, key_base2k, mode):
    """Both sides of the spectral tail's 16-bit body operand gate (api_glwe.hip spectral_body16: key_base2k <= 16, <= 15 for the add
    forms): the note names the side taken, and both sides decrypt."""
    ref, hip = mods(8192)
    c = _shape_case("auto", 8192, 1, 3, key_base2k, seed=800 + key_base2k, mode=mode, p=P_SPECTRAL)
    notes = _run(ref, hip, (8192, key_base2k, mode), c)
    assert "PERM=1" in notes, notes
    assert (BODY16 in notes) == (key_base2k <= (15 if mode == "add" else 16)), (key_base2k, mode, notes)


def test_headline_control_fails_on_device(mods):
    """At the headline shape too: an automorphism key for p instead of p^-1 gives device == oracle and a failed decryption."""
    ref, hip = mods(65536)
    k = 8 * 12
    c = cs.automorphism_case(65536, 1, 1, 8, 12, 12, 12, k, k, k, 1, BATCH, 4242, encrypt_for=cs.P_AUTO % (2 * 65536))
    _run(ref, hip, "headline: automorphism key for p", c, fail=True)
    assert fs.galois_inv(cs.P_AUTO, 65536) != cs.P_AUTO % (2 * 65536)
