"""GPU: pz_glwe_tensor_dot_relinearize_batched and the plan built on it (poulpy_amd/ckks.py plan_dot_product_ct), bit for bit against the
oracle (tests/ckks_dot_oracle.py) - no tolerance anywhere.  Shapes and sizes of tests/test_gpu_ckks_mul.py: N = 256 at base2k 12, ranks 1 and
2 (the i64 accumulated tensor) and N = 8192, rank 1 (the pipeline: the 16-bit accumulated tensor up to 5 pairs, the i64 one beyond); batch 5
in waves of 2, so that the wave loop, its remainder and the reuse of the workspace all run.  One case is decrypted under a real key."""
import os
import subprocess
import sys

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import Ct
from poulpy_amd.layouts import VecZnx
from tests import ckks_dot_cases as dcases
from tests import ckks_dot_oracle as do
from tests import ckks_mul_cases as cases
from tests import ckks_mul_oracle as mo
from tests import fhe_sk as fs
from tests.core_cases import prepare
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded
from tests.test_gpu_ckks_mul import B, BATCH, CHUNK, FUSED, GRAPHS, Setup, _down, _rand, _vec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 1), (256, 2), (8192, 1)]
NOTE_T16 = "glwe_tensor_dot_relinearize: 16-bit accumulated tensor"
NOTE_I64 = "glwe_tensor_dot_relinearize: i64 accumulated tensor"
T16_MAX_PAIRS = 5          # at base2k 12: 5 x 3 x 2^11 = 30 720 <= 2^15 - 1 (poulpy_amd/csrc/dot_form.hpp)
CONT = 6                   # limbs of the operand containers: 4 (a) / 3 (b) in use, garbage in the rest


def _check_route(s, notes, npairs):
    """the 16-bit form on the pipeline shape up to the bound, the i64 form everywhere else; with the fused tensoring switched off the
    one-call product is not compact anywhere (as tests/test_gpu_ckks_mul.py relaxes its own route assertion)"""
    assert (NOTE_T16 in notes) != (NOTE_I64 in notes), notes
    if FUSED:
        assert (NOTE_T16 in notes) == (s.n == 8192 and npairs <= T16_MAX_PAIRS), (s.n, npairs, notes)
    else:
        assert NOTE_I64 in notes, notes


def _oracle_prefixes(s, a_ops, b_ops):
    """a_ops / b_ops: per pair an array (batch, CONT, cols, n).  -> per pair count 1 .. npairs the oracle's result (batch, size, cols, n), and the
    accumulated tensors of the full count: ONE glwe_tensor_apply / _add_assign per pair and ciphertext, a relinearization per prefix"""
    tp, _ = s.params()
    npairs, batch = len(a_ops), a_ops[0].shape[0]
    want = np.zeros((npairs, batch, s.size, s.cols, s.n), dtype=np.int64)
    tensors = []
    for t in range(batch):
        acc = VecZnx(s.n, s.cols * (s.cols + 1) // 2, s.t_size)
        for i in range(npairs):
            s.ref.glwe_tensor_apply(s.off, acc, B, mo.compact(_vec(a_ops[i][t]), s.a_size), int(tp.a_effective_k),
                                    mo.compact(_vec(b_ops[i][t]), s.b_size), int(tp.b_effective_k), B, add_assign=i > 0)
            out = VecZnx(s.n, s.cols, s.size)
            s.ref.glwe_tensor_relinearize(out, B, acc, B, s.tsk.pmat, s.tsk.dsize, s.tsk.base2k)
            want[i, t] = out.data
        tensors.append(acc.data.copy())
    return want, np.stack(tensors)


def _dot(s, dev, d_res, a_ptrs, b_ptrs, batch=BATCH, a_strides=None, b_strides=None):
    tp, rp = s.params()
    n = len(a_ptrs)
    s.hip.glwe_tensor_dot_relinearize_batched(getattr(d_res, "ptr", d_res), [getattr(p, "ptr", p) for p in a_ptrs], [getattr(p, "ptr", p) for p in b_ptrs],
                                              dev.key_buf.ptr, tp, rp, batch, a_strides=[CONT] * n if a_strides is None else a_strides,
                                              b_strides=[CONT] * n if b_strides is None else b_strides)


_SHARED = {}


def _three_pairs(mods, n, rank):
    """three pairs per shape, computed once and left unchanged: operands in 6-limb containers with garbage in the unused limbs; pair 2 reuses
    pair 0's a operand (one pointer in two pairs)"""
    if (n, rank) not in _SHARED:
        s = Setup(mods, n, rank, 1100 + rank)
        a0, a1 = (_rand(s.rng, (BATCH, CONT, s.cols, n)) for _ in range(2))
        b0, b1, b2 = (_rand(s.rng, (BATCH, CONT, s.cols, n)) for _ in range(3))
        want, _ = _oracle_prefixes(s, [a0, a1, a0], [b0, b1, b2])
        _SHARED[(n, rank)] = (s, (a0, a1), (b0, b1, b2), want)
    return _SHARED[(n, rank)]


@pytest.mark.parametrize("n,rank", SHAPES)
def test_one_two_and_three_pairs_equal_the_per_op_composition_and_the_oracle(mods, n, rank):
    """npairs 1, 2, 3: device == npairs x pz_glwe_tensor_apply_batched (apply, then add_assign) on a caller-owned i64 tensor batch +
    pz_glwe_tensor_relinearize_batched on compacted copies == the oracle; the route note says which form ran"""
    s, (a0, a1), (b0, b1, b2), want = _three_pairs(mods, n, rank)
    tp, rp = s.params()
    shape = want.shape[1:]
    with on_device(s.hip, chunk=CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a = [dev.upload(a0), dev.upload(a1)]
        d_b = [dev.upload(b0), dev.upload(b1), dev.upload(b2)]
        d_ac = [dev.upload(x[:, :s.a_size]) for x in (a0, a1)]
        d_bc = [dev.upload(x[:, :s.b_size]) for x in (b0, b1, b2)]
        d_t = dev.alloc(BATCH * s.t_size * (s.cols * (s.cols + 1) // 2) * n * 8)
        for npairs in (1, 2, 3):
            pa, pb = [d_a[0], d_a[1], d_a[0]][:npairs], d_b[:npairs]
            d_r, d_rc = dev.alloc(want[0].nbytes), dev.alloc(want[0].nbytes)
            s.hip.dispatch_notes(reset=True)
            _dot(s, dev, d_r, pa, pb)
            s.hip.sync()
            _check_route(s, s.hip.dispatch_notes(), npairs)
            for i in range(npairs):
                s.hip.glwe_tensor_apply_batched(d_t.ptr, [d_ac[0], d_ac[1], d_ac[0]][i].ptr, d_bc[i].ptr, tp, "apply" if i == 0 else "add_assign", BATCH)
            s.hip.glwe_tensor_relinearize_batched(d_rc.ptr, d_t.ptr, dev.key_buf.ptr, rp, BATCH)
            s.hip.sync()
            got, old = _down(d_r, shape), _down(d_rc, shape)
            assert np.array_equal(got, old), ("one call != the per-op composition", npairs)
            assert np.array_equal(got, want[npairs - 1]), ("device != oracle", npairs)
            dev.free(d_r)
            dev.free(d_rc)
        # one pair is the existing one-call product
        d_r, d_rc = dev.alloc(want[0].nbytes), dev.alloc(want[0].nbytes)
        _dot(s, dev, d_r, d_a[:1], d_b[:1])
        s.hip.glwe_tensor_mul_relinearize_acc_batched(d_rc.ptr, d_a[0].ptr, d_b[0].ptr, dev.key_buf.ptr, tp, rp, "apply", BATCH, a_stride=CONT, b_stride=CONT)
        s.hip.sync()
        assert np.array_equal(_down(d_r, shape), _down(d_rc, shape))


def test_sixteen_bit_bound_with_every_pair_identical(mods):
    """N = 8192, batch 3, the largest pair count the form function admits at base2k 12 with ALL pairs identical: every accumulated value is
    npairs x one product's.  The oracle's accumulated tensor shows that the case reaches the range (some |value| >= npairs (2^(B-1) - 8)) and
    that the bound is tight (with one pair more its largest value would leave int16).  One pair more: the i64 form, still bit-exact."""
    n, rank, batch = 8192, 1, 3
    s = Setup(mods, n, rank, 1200)
    a = _rand(s.rng, (batch, CONT, s.cols, n))
    b = _rand(s.rng, (batch, CONT, s.cols, n))
    npairs = T16_MAX_PAIRS
    want, tensors = _oracle_prefixes(s, [a] * (npairs + 1), [b] * (npairs + 1))
    _, one = _oracle_prefixes(s, [a], [b])
    assert np.array_equal(tensors, (npairs + 1) * one)
    peak = int(np.abs(npairs * one).max())
    print(f"[t16 bound] largest accumulated |value| at {npairs} pairs: {peak}; at {npairs + 1}: {int(np.abs(tensors).max())}")
    assert peak >= npairs * ((1 << (B - 1)) - 8) and peak <= 32767, peak
    assert int(np.abs(tensors).max()) > 32767, "one pair more would still fit int16: the case does not reach the bound"
    shape = want.shape[1:]
    with on_device(s.hip, chunk=CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a, d_b = dev.upload(a), dev.upload(b)
        for k in (npairs, npairs + 1):
            d_r = dev.alloc(want[0].nbytes)
            s.hip.dispatch_notes(reset=True)
            _dot(s, dev, d_r, [d_a] * k, [d_b] * k, batch=batch)
            s.hip.sync()
            _check_route(s, s.hip.dispatch_notes(), k)
            assert np.array_equal(_down(d_r, shape), want[k - 1]), ("device != oracle", k)
            dev.free(d_r)


def test_alias_and_argument_refusals_leave_res_untouched(mods):
    from poulpy_amd.hal import PoulpyHipError
    s, (a0, a1), (b0, b1, b2), want = _three_pairs(mods, 256, 1)
    shape = want.shape[1:]
    with on_device(s.hip, chunk=CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a0, d_b0, d_b1 = dev.upload(a0), dev.upload(b0), dev.upload(b1)
        big = _rand(s.rng, (BATCH + 1, CONT, s.cols, 256))
        d_big = dev.upload(big)
        ct = CONT * s.cols * 256 * 8
        # res inside operand i > 0 (either side): PZ_ERR_ALIAS, the operand keeps its bytes
        for label, pa, pb in (("res overlaps a[1]", [d_a0.ptr, d_big.ptr], [d_b0.ptr, d_b1.ptr]), ("res overlaps b[2]", [d_a0.ptr] * 3, [d_b0.ptr, d_b1.ptr, d_big.ptr])):
            with pytest.raises(PoulpyHipError, match=r"\[-4\]"):
                _dot(s, dev, d_big.ptr.value + ct // 2, pa, pb)
            s.hip.sync()
            assert np.array_equal(_down(d_big, big.shape), big), label
        for label, pa, pb, kw in (("stride below the size", [d_a0, d_a0], [d_b0, d_b1], dict(a_strides=[CONT, s.a_size - 1])),
                                  ("b stride below the size", [d_a0, d_a0], [d_b0, d_b1], dict(b_strides=[s.b_size - 1, CONT])),
                                  ("no pair", [], [], {}),
                                  ("65 pairs", [d_a0] * 65, [d_b0] * 65, {})):
            d_r = dev.alloc(want[0].nbytes)
            with pytest.raises(PoulpyHipError, match=r"\[-1\]"):
                _dot(s, dev, d_r, pa, pb, **kw)
            s.hip.sync()
            assert np.all(_down(d_r, shape) == 0x5A5A5A5A5A5A5A5A), label
            dev.free(d_r)
        # 64 pairs are taken (the same pair 64 times: 64 x one product's tensor)
        tp, rp = s.params()
        assert s.hip.glwe_tensor_dot_relinearize_workspace_bytes(tp, rp, 64, BATCH) > 0
        assert s.hip.glwe_tensor_dot_relinearize_workspace_bytes(tp, rp, 0, BATCH) == 0 == s.hip.glwe_tensor_dot_relinearize_workspace_bytes(tp, rp, 65, BATCH)


@pytest.mark.parametrize("n,rank", [(256, 1), (8192, 1)])
def test_replayed_in_a_graph_with_new_contents_and_a_new_graph_for_a_new_pointer(mods, n, rank):
    """second and third call with new contents behind the same pointers (the batch rolled: the oracle's results roll with it), bit-exact; with
    another pointer for pair 2's a the call runs plainly once and is captured as a graph of its own"""
    s, (a0, a1), (b0, b1, b2), want = _three_pairs(mods, n, rank)
    w3, shape = want[2], want.shape[1:]
    with on_device(s.hip, chunk=CHUNK, graphs=True) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a0, d_a1, d_a2 = dev.alloc(a0.nbytes), dev.alloc(a0.nbytes), dev.alloc(a0.nbytes)
        d_b = [dev.alloc(a0.nbytes) for _ in range(3)]
        d_r = dev.alloc(w3.nbytes)
        counts = [s.hip.graph_launches()]
        for it in range(5):
            r = it % BATCH
            d_a0.upload(np.roll(a0, r, axis=0)), d_a1.upload(np.roll(a1, r, axis=0)), d_a2.upload(np.roll(a0, r, axis=0))
            for d, x in zip(d_b, (b0, b1, b2)):
                d.upload(np.roll(x, r, axis=0))
            d_r.upload(_rand(s.rng, shape))
            _dot(s, dev, d_r, [d_a0, d_a1, d_a0 if it < 3 else d_a2], d_b)
            s.hip.sync()
            assert np.array_equal(_down(d_r, shape), np.roll(w3, r, axis=0)), ("call", it)
            counts.append(s.hip.graph_launches())
        if GRAPHS:
            steps = [y - x for x, y in zip(counts, counts[1:])]
            assert steps == [0, 1, 1, 0, 1], steps   # plain, captured + launched, replayed | the new pointer: plain, then a graph of its own


CANARY_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_ckks_dot as t
from oracle.ref import RefModule
from poulpy_amd.hal import Module
from tests.device import on_device
cache = {}
def mods(n):
    if n not in cache:
        cache[n] = (RefModule(n), Module(n))
    return cache[n]
for n, rank, counts in ((256, 2, (3,)), (8192, 1, (3, 6))):
    s = t.Setup(mods, n, rank, 1300 + rank)
    s.hip = Module(n)          # a module that has run nothing else: its workspace is this call's
    batch = 3
    a = t._rand(s.rng, (batch, t.CONT, s.cols, n))
    b = t._rand(s.rng, (batch, t.CONT, s.cols, n))
    want, _ = t._oracle_prefixes(s, [a] * max(counts), [b] * max(counts))
    tp, rp = s.params()
    with on_device(s.hip, chunk=t.CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a, d_b = dev.upload(a), dev.upload(b)
        for k in counts:
            ws = s.hip.glwe_tensor_dot_relinearize_workspace_bytes(tp, rp, k, batch)
            d_r = dev.alloc(want[0].nbytes)
            t._dot(s, dev, d_r, [d_a] * k, [d_b] * k, batch=batch)
            s.hip.sync()
            assert np.array_equal(t._down(d_r, want.shape[1:]), want[k - 1]), (n, k)
            # the module's main workspace is allocated at 9 / 8 of what a call reserves: never beyond what the query reports
            assert 0 < s.hip.workspace_bytes() <= ws + ws // 8, (n, k, ws, s.hip.workspace_bytes())
print("guarded run ok", flush=True)
"""


def test_workspace_query_and_guards():
    """a fresh module under POULPY_DBG_CANARY: every workspace segment of the call - the accumulated tensor, the term tensors, the carves of
    the tensoring and of the relinearization - keeps its guard, in both forms; the module's workspace stays within _workspace_bytes"""
    env = dict(os.environ, POULPY_DBG_CANARY="1")
    out = subprocess.run([sys.executable, "-c", CANARY_CHILD % ROOT], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "WORKSPACE OVERRUN" not in out.stderr and "guarded run ok" in out.stdout


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", SHAPES)
def test_every_scenario_through_the_plan_on_device(mods, n, rank):
    """DotCtPlan.launch on a batch in waves of 2 == the literal restatement of ckks_dot_product_ct on the oracle, digits and metadata: the
    fast branch aligned, with either side rescaled, into a narrower output and from larger containers, and the fallback"""
    limbs, cols = 5, rank + 1
    ref, hip = mods(n)
    rng = seeded(1400 + rank)
    mat = cases.random_tensor_key(rng, n, B, rank, limbs, limbs + 1)
    pr, ph = prepared_key(ref, hip, mat)
    tsk, tsk_meta = mo.Tsk(pr, 1, B), (limbs, 1, limbs + 1, B)
    batch = 3 if n == 8192 else BATCH
    bad = []
    with on_device(hip, chunk=CHUNK) as dev:
        d_k = dev.key(ph)
        for label, branch, dsize, a_list, b_list in dcases.dot_scenarios(B, cols, limbs):
            plan = ckks.plan_dot_product_ct(Ct(B, dsize, 0, 0, cols), a_list, b_list)
            assert plan.branch == branch, label
            ha = [[cases.fill_ct(rng, n, x) for x in a_list] for _ in range(batch)]
            hb = [[cases.fill_ct(rng, n, x) for x in b_list] for _ in range(batch)]
            want, meta = [], None
            for t in range(batch):
                d = Ct(B, dsize, 0, 0, cols, VecZnx(n, cols, dsize))
                do.ckks_dot_product_ct(ref, d, ha[t], hb[t], tsk)
                want.append(d.data.data)
                meta = (d.log_delta, d.log_budget)
            want = np.stack(want)
            bufs_a = [dev.upload(np.stack([ha[t][i].data.data for t in range(batch)])) for i in range(len(a_list))]
            bufs_b = [dev.upload(np.stack([hb[t][i].data.data for t in range(batch)])) for i in range(len(b_list))]
            g_a = [Ct(B, x.size, x.log_delta, x.log_budget, cols, bufs_a[i].ptr) for i, x in enumerate(a_list)]
            g_b = [Ct(B, x.size, x.log_delta, x.log_budget, cols, bufs_b[i].ptr) for i, x in enumerate(b_list)]
            d_d = dev.alloc(want.nbytes)
            nbytes = plan.scratch_bytes(batch, n)
            d_tmp = dev.alloc(nbytes) if nbytes else None
            dd = Ct(B, dsize, 0, 0, cols, d_d.ptr)
            hip.dispatch_notes(reset=True)
            plan.launch(hip, dd, batch, g_a, g_b, tsk_ptr=d_k.ptr, tsk=tsk_meta, tmp=None if d_tmp is None else d_tmp.ptr)
            hip.sync()
            notes = hip.dispatch_notes()
            if branch == "fast" and FUSED:
                assert ((NOTE_T16 if n == 8192 else NOTE_I64) in notes), (label, notes)
            if not np.array_equal(_down(d_d, want.shape), want) or (dd.log_delta, dd.log_budget) != meta:
                bad.append(label)
            for buf in bufs_a + bufs_b + [d_d] + ([d_tmp] if d_tmp is not None else []):
                dev.free(buf)
    assert not bad, bad


# ---- one decrypted case --------------------------------------------------------------------------------------------------------------------
def test_three_pairs_decrypt_to_the_sum_of_products_with_a_control(mods):
    """c0 c1 + c2 c3 + c0 c3 at N = 256 under a real tensor key, every ciphertext of the batch the same messages under its own encryption
    noise: device == oracle bit for bit, the result decrypts to the exact sum within check_decrypt's bounds; with one pair dropped it does not"""
    n, rank, batch = 256, 1, 3
    ref, hip = mods(n)
    c = cases.decrypt_case(n, rank, 1500, s=18)
    pr, ph = prepare(ref, c.key), prepare(hip, c.key)
    tsk = mo.Tsk(pr, 1, c.B)
    E, s, size, cols = c.E, c.s, c.size, c.cols
    ms = c.ms
    pairs = [(0, 1), (2, 3), (0, 3)]
    fresh = lambda data=None: Ct(c.B, size, cases.D, E - cases.D, cols, data)                   # noqa: E731
    plan = ckks.plan_dot_product_ct(Ct(c.B, size, 0, 0, cols), [fresh() for _ in pairs], [fresh() for _ in pairs])
    assert plan.branch == "fast" and not plan.rescales and plan.cnv_offset == E
    bits = E - 2 * s                                                                            # a b stands at 2^-(E - 2 s)
    want_int = sum(fs.mul_msg(ms[i], ms[j]) for i, j in pairs)
    enc = [np.stack([cases._encrypt(c.sk, m, s, c.B, E, size, c.rng) for _ in range(batch)]) for m in ms]
    want, short = [], []
    for t in range(batch):
        a_list = [fresh(_vec(enc[i][t])) for i, _ in pairs]
        b_list = [fresh(_vec(enc[j][t])) for _, j in pairs]
        d = Ct(c.B, size, 0, 0, cols, VecZnx(n, cols, size))
        do.ckks_dot_product_ct(ref, d, a_list, b_list, tsk)
        want.append(d.data.data)
        d2 = Ct(c.B, size, 0, 0, cols, VecZnx(n, cols, size))
        do.ckks_dot_product_ct(ref, d2, a_list[:2], b_list[:2], tsk)
        short.append(d2.data.data)
    want = np.stack(want)
    with on_device(hip, chunk=2) as dev:
        d_k = dev.key(ph)
        bufs = [dev.upload(x) for x in enc]
        d_d = dev.alloc(want.nbytes)
        dd = Ct(c.B, size, 0, 0, cols, d_d.ptr)
        plan.launch(hip, dd, batch, [fresh(bufs[i].ptr) for i, _ in pairs], [fresh(bufs[j].ptr) for _, j in pairs], tsk_ptr=d_k.ptr, tsk=c.tsk)
        hip.sync()
        got = _down(d_d, want.shape)
    assert np.array_equal(got, want), "device != oracle"
    assert (dd.log_delta, dd.log_budget) == (cases.D, E - 2 * cases.D)
    for t in range(batch):
        cases.check_decrypt(f"c0 c1 + c2 c3 + c0 c3 [{t}]", c, got[t], want_int, bits, plan.cnv_offset)
        cases.check_decrypt(f"one pair dropped [{t}]", c, short[t], want_int, bits, plan.cnv_offset, fail=True)
