"""The encrypt / multiply / decrypt procedures of tests/tensor_cases.py through the batched device entry points
(pz_glwe_tensor_apply_batched, pz_glwe_tensor_relinearize_batched, pz_glwe_tensor_mul_relinearize_batched).

Every case runs a batch of 3 message pairs of their own under a real tensor key; the result buffers are pre-filled with 0x5A; the device
output is compared with the oracle bit for bit, then decrypted under the secret key (tests/fhe_sk.py) against the exact product of the
messages and the reference's bound.  The negative controls go through the same calls: device == oracle, and the decryption fails.
The square form is also run as apply(a, a) on the device and must agree bit for bit, and add_assign as accumulator + apply.  Shapes:
the reference's own (N = 256, base2k 17, the per-op composition) and tests/tensor_cases.py ROUTES (the fused row pass k_mid_cnv at
N = 8192, two bases on the same ring, the relinearization fused and unfused at N = 4096, the one-call multiply with the tensor as 16-bit
digits and as i64, BASELINE configs[4] once per form), with their dispatch notes.  noise_have / noise_want are printed (`-s`)."""
import os

import numpy as np
import pytest

from tests import tensor_cases as tc
from tests.core_cases import prepare
from tests.device import mods, on_device  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH = 3


def _device(hip, c, kind, mode=None, chunk=0, fuse=(True, True), pin=False):
    """The case's batch through the entry points of `kind` -> ({"tensor": ..., "relin": ...} as tc.run_oracle, dispatch notes)."""
    from poulpy_amd.hal import GlweOpParams, GlweTensorParams
    mode = mode or c.mode
    square = mode == "square"
    n, cols = c.n, c.rank + 1
    pairs = c.rank * (c.rank + 1) // 2
    tcols = cols + pairs
    batch, a_size = c.a.shape[0], c.a.shape[1]
    b_all = c.a if c.b is None else c.b
    out = {}
    d_key = None
    with on_device(hip) as dev:
        d_a = dev.upload(c.a)
        d_b = d_a if c.b is None else dev.upload(c.b)
        t_shape = (batch, c.res_size, tcols, n)
        tp = GlweTensorParams(rank=c.rank, a_size=a_size, b_size=b_all.shape[1], ab_base2k=c.in_base2k, a_effective_k=c.a_k,
                              b_effective_k=c.b_k, res_size=c.res_size, res_base2k=c.res_base2k, cnv_offset=c.cnv_offset)
        if c.key is not None and kind != "apply":
            rows, pr, ksz, _, _ = c.key.shape
            assert pr == pairs
            ph = prepare(hip, c.key)
            d_key = dev.key(ph)
            rp = GlweOpParams(rank=c.rank, dnum=rows, dsize=c.dsize, key_size=ksz, key_base2k=c.key_base2k, a_size=c.res_size,
                              a_base2k=c.res_base2k, res_size=c.relin[0], res_base2k=c.relin[1], rank_out=c.rank)
            r_shape = (batch, c.relin[0], cols, n)
            d_r = dev.alloc(int(np.prod(r_shape)) * 8)
        with on_device(hip, chunk=chunk, fuse=fuse) as pinned:
            hip.dispatch_notes(reset=True)
            if pin:
                pinned.pin(d_key, rows, pairs, cols, ksz)
            if kind == "one_call":
                hip.glwe_tensor_mul_relinearize_batched(d_r.ptr, d_a.ptr, None if square else d_b.ptr, d_key.ptr, tp, rp, mode, batch)
            else:
                d_t = dev.upload(c.acc) if mode == "add_assign" else dev.alloc(int(np.prod(t_shape)) * 8)
                hip.glwe_tensor_apply_batched(d_t.ptr, d_a.ptr, None if square else d_b.ptr, tp, mode, batch)
                if kind == "two_calls" and d_key is not None:
                    hip.glwe_tensor_relinearize_batched(d_r.ptr, d_t.ptr, d_key.ptr, rp, batch)
                hip.sync()
                out["tensor"] = d_t.download(np.int64, int(np.prod(t_shape))).reshape(t_shape)
            hip.sync()
            if d_key is not None:
                out["relin"] = d_r.download(np.int64, int(np.prod(r_shape))).reshape(r_shape)
            notes = hip.dispatch_notes()
    return out, notes


def _run(ref, hip, label, c, kind, fail=False, **kw):
    got, notes = _device(hip, c, kind, **kw)
    want = tc.run_oracle(ref, c)
    assert got.keys() == want.keys(), (label, list(got), list(want))
    for stage in want:
        assert np.array_equal(got[stage], want[stage]), (label, stage, "device != oracle")
    if c.mode in ("square", "add_assign"):
        # the device's own apply: square == apply(a, a), add_assign == accumulator + apply, bit for bit (glwe_tensor.rs:404, :420, :269)
        other, _ = _device(hip, c, kind, mode="apply", **kw)
        for stage in got:
            if c.mode == "square":
                assert np.array_equal(got[stage], other[stage]), (label, stage, "square != apply(a, a) on the device")
            elif stage == "tensor":
                assert np.array_equal(got[stage], c.acc + other[stage]), (label, "add_assign != acc + apply on the device")
    tc.check(label, c, got, fail=fail)
    return notes


@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("kind", tc.MODES)
def test_reference_procedures_on_device(mods, kind, rank):
    """The reference's loops (N = 256, base2k 17) through the per-op composition: res_offset in {0, 1, in_base2k - 1, in_base2k, scale - 1}
    (every one runs on the oracle in tests/test_tensor_semantics.py, rank 3 too)."""
    ref, hip = mods(tc.N)
    for label, c in tc.reference_cases(kind, batch=BATCH, ranks=(rank,), offsets=tc.DEVICE_OFFSETS):
        _run(ref, hip, label, c, "two_calls")


def test_negative_controls_fail_on_device(mods):
    ref, hip = mods(tc.N)
    for label, c in tc.control_cases(batch=BATCH):
        _run(ref, hip, label, c, "two_calls", fail=True)


@pytest.mark.parametrize("name", list(tc.ROUTES))
def test_routes_decrypt(mods, name):
    c, k = tc.route_case(name, batch=BATCH)
    ref, hip = mods(c.n)
    notes = _run(ref, hip, name, c, k.kind, chunk=k.chunk, fuse=k.fuse, pin=k.pin)
    if k.mid_cnv is not None and os.environ.get("POULPY_DBG_TENSOR_FUSED") != "0" and os.environ.get("POULPY_DBG_TENSOR_COMBINE") != "0":
        assert ("k_mid_cnv" in notes) == k.mid_cnv, (name, notes)
    if k.t16 is not None and os.environ.get("POULPY_DBG_TENSOR_FUSED") != "0" and os.environ.get("POULPY_DBG_TENSOR_COMBINE") != "0":
        assert (tc.NOTE_T16 in notes) == k.t16, (name, notes)       # both sides of the gate: base2k 14 against 15


@pytest.mark.parametrize("label", list(tc.LARGE_CONTROLS))
def test_large_controls_fail_on_device(mods, label):
    """At the N = 8192 one-call multiply too: exchanged pair columns of the tensor key, and cnv_offset read one bit off, give
    device == oracle and a failed decryption."""
    c = tc.tensor_case(batch=BATCH, **tc.LARGE_CONTROLS[label])
    ref, hip = mods(c.n)
    notes = _run(ref, hip, label, c, "one_call", fail=True, chunk=2)
    assert tc.NOTE_T16 in notes, notes


# ---- plaintext and constant products (pz_glwe_mul_plain_batched, pz_glwe_mul_const_batched) ----
def _device_plain(hip, c, chunk=2):
    from poulpy_amd.hal import GlweMulConstParams, GlweTensorParams
    n, cols = c.n, c.rank + 1
    batch, a_size = c.a.shape[0], c.a.shape[1]
    assign = c.mode == "assign"
    shape = (batch, c.res_size, cols, n)
    nbytes = int(np.prod(shape)) * 8
    with on_device(hip) as dev:
        d_a = dev.upload(c.a)
        if assign:
            assert c.a.shape == shape
            d_r = d_a
        else:
            d_r = dev.alloc(nbytes)
        with on_device(hip, chunk=chunk):
            hip.dispatch_notes(reset=True)
            if c.op == "plain":
                pt = np.ascontiguousarray(c.pt)
                d_pt = dev.upload(pt)
                p = GlweTensorParams(rank=c.rank, a_size=a_size, b_size=pt.shape[1], ab_base2k=c.ab, a_effective_k=c.a_k, b_effective_k=c.b_k,
                                     res_size=c.res_size, res_base2k=c.rb, cnv_offset=c.cnv_offset)
                hip.glwe_mul_plain_batched(d_r.ptr, None if assign else d_a.ptr, d_pt.ptr, c.shared, p, c.mode, batch)
            else:
                p = GlweMulConstParams(rank=c.rank, a_size=a_size, a_base2k=c.ab, res_size=c.res_size, res_base2k=c.rb, cnv_offset=c.cnv_offset)
                hip.glwe_mul_const_batched(d_r.ptr, None if assign else d_a.ptr, c.re, c.im, p, c.mode, batch, b_size=3)
            hip.sync()
            got = d_r.download(np.int64, int(np.prod(shape))).reshape(shape)
            notes = hip.dispatch_notes()
    return got, notes


def _run_plain(ref, hip, label, c, fail=False):
    got, notes = _device_plain(hip, c)
    assert np.array_equal(got, tc.run_plain_oracle(ref, c)), (label, "device != oracle")
    tc.check_plain(label, c, got, fail=fail)
    return notes


@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("kind", ["plain", "const"])
def test_plain_reference_procedures_on_device(mods, kind, rank):
    ref, hip = mods(tc.N)
    for label, c in tc.plain_reference_cases(kind, batch=BATCH, ranks=(rank,), offsets=tc.DEVICE_OFFSETS):
        _run_plain(ref, hip, label, c)


def test_plain_negative_controls_fail_on_device(mods):
    ref, hip = mods(tc.N)
    for label, c in tc.plain_control_cases(batch=BATCH):
        _run_plain(ref, hip, label, c, fail=True)


@pytest.mark.parametrize("name", list(tc.PLAIN_ROUTES))
def test_plain_routes_decrypt(mods, name):
    c = tc.plain_route_case(name, batch=BATCH)
    ref, hip = mods(c.n)
    notes = _run_plain(ref, hip, name, c)
    if c.op == "const" and c.ab == c.rb:
        assert "k_mul_const_nz" in notes, (name, notes)       # as tests/test_gpu_mul_plain.py::test_glwe_mul_const_batched
    if c.op == "plain" and "mid-cnv" in name:
        assert "k_mid_cnv" in notes, (name, notes)
    print(f"[notes] {name}: {notes}")
