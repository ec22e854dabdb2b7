"""The encrypt / trace / decrypt and encrypt / pack / decrypt procedures of tests/trace_cases.py through the batched device entry points
(pz_glwe_trace_batched, pz_glwe_pack_batched, pz_glwe_pack_bases_batched).

Every case runs a batch of 3 ciphertexts (3 sets of ciphertexts for the packing), each with its own plaintext, under one real
automorphism key per Galois element; the packing's result buffer is pre-filled with 0x5A (the trace works in place); the device output
is compared with the oracle bit for bit, then decrypted under the secret key (tests/fhe_sk.py) against the definition applied to the
plaintext and the reference's noise formula.  The negative controls go through the same calls: device == oracle, and the decryption
fails.  Shapes: the reference's own and tests/trace_cases.py ROUTES (N = 512 full trace, N = 4096, N = 8192 fused and unfused, N = 2^16
where the one-bit shift rides on the spectral tail, the result in another base than the keys; the packing dense, sparse, rank 2,
on the fused pipeline and in the reference's two bases).  noise_have / noise_want are printed (`-s`)."""
import numpy as np
import pytest

from tests import trace_cases as tc
from tests.core_cases import prepare
from tests.device import mods, on_device  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH = 3


def _device(hip, c, fuse=(True, True)):
    """One batched call on the case's ciphertexts -> (outputs, dispatch notes)."""
    from poulpy_amd.hal import GlweOpParams
    n, cols = c.n, c.rank + 1
    rows, _, ksz, _, _ = c.keys[0].shape
    gals = [tc._gal(g, n) for g in c.gals]
    with on_device(hip) as dev:
        d_keys = [dev.key(prepare(hip, key)) for key in c.keys]
        hip.sync()
        one_base = c.base2k == c.key_base2k
        with on_device(hip, fuse=fuse):
            hip.dispatch_notes(reset=True)
            if c.op == "trace":
                batch, size = c.a.shape[0], c.a.shape[1]
                p = GlweOpParams(rank=c.rank, dnum=rows, dsize=1, key_size=ksz, key_base2k=c.key_base2k, a_size=size if one_base else c.conv_size,
                                 a_base2k=c.key_base2k, res_size=size, res_base2k=c.base2k, rank_out=c.rank)
                d_res = dev.upload(c.a)
                hip.glwe_trace_batched(d_res.ptr, gals, [d.ptr for d in d_keys], p, batch)
                shape = c.a.shape
            else:
                batch, size = len(c.want), c.size
                p = GlweOpParams(rank=c.rank, dnum=rows, dsize=1, key_size=ksz, key_base2k=c.key_base2k, a_size=size, a_base2k=c.base2k, res_size=size,
                                 res_base2k=c.base2k, rank_out=c.rank)
                shape = (batch, size, cols, n)
                d_cts = [dev.upload(c.a[j]) for j in c.indices]
                d_res = dev.alloc(int(np.prod(shape)) * 8)
                nbytes = hip.glwe_pack_tmp_bytes(p, batch) if one_base else hip.glwe_pack_bases_tmp_bytes(p, c.conv_size, batch)
                d_tmp = dev.alloc(nbytes)
                if one_base:
                    hip.glwe_pack_batched(d_res.ptr, c.indices, [d.ptr for d in d_cts], c.log_gap_out, gals, [k.ptr for k in d_keys], p, d_tmp.ptr,
                                          nbytes, batch)
                else:
                    hip.glwe_pack_bases_batched(d_res.ptr, c.indices, [d.ptr for d in d_cts], c.log_gap_out, gals, [k.ptr for k in d_keys], p,
                                                c.conv_size, d_tmp.ptr, nbytes, batch)
            hip.sync()
            got = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
            notes = hip.dispatch_notes()
    return got, notes


def _run(ref, hip, label, c, fail=False, **kw):
    got, notes = _device(hip, c, **kw)
    want = tc.run_oracle(ref, c)
    assert np.array_equal(got, want), (label, "device != oracle")
    tc.check(label, c, got, fail=fail)
    return notes


@pytest.mark.parametrize("kind", ["trace", "pack"])
def test_reference_procedures_on_device(mods, kind):
    for label, c in tc.reference_cases(kind, batch=BATCH):
        ref, hip = mods(c.n)
        _run(ref, hip, label, c)


def test_negative_controls_fail_on_device(mods):
    for label, c in tc.control_cases(batch=BATCH):
        ref, hip = mods(c.n)
        _run(ref, hip, label, c, fail=True)


@pytest.mark.parametrize("name", list(tc.ROUTES))
def test_routes_decrypt(mods, name):
    c, k = tc.route_case(name, batch=BATCH)
    ref, hip = mods(c.n)
    notes = _run(ref, hip, name, c, fuse=k.fuse)
    print(f"[notes] {name}: {notes}")
    if name in ("trace-n8192-fused", "trace-n65536-first4"):    # the spectral automorphism-add with the 16-bit body operand (base2k 12)
        assert "k_mid128" in notes and "PERM=1" in notes and "spectral tail: 16-bit body operand" in notes, (name, notes)
    if name == "trace-n8192-unfused":
        assert "k_mid128" not in notes, (name, notes)


def test_headline_control_fails_on_device(mods):
    """At N = 2^16 too: trace keys made for g instead of g^-1 give device == oracle and a failed decryption."""
    _, kw, _ = tc.ROUTES["trace-n65536-first4"]
    c = tc.trace_case(batch=BATCH, **dict(kw, for_g=True, seed=65537))
    ref, hip = mods(c.n)
    _run(ref, hip, "n65536: trace keys for g", c, fail=True)
