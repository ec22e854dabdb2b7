"""GPU: pz_glwe_tensor_mul_relinearize_acc_batched and the plans built on it (poulpy_amd/ckks.py: mul_into / mul_assign / square_into /
square_assign, mul_add_ct / mul_sub_ct, mul_many, compact_limbs_copy), bit for bit against the oracle (tests/ckks_mul_oracle.py) - no
tolerance anywhere.  Shapes: N = 256 at base2k 12, ranks 1 and 2 (the per-op composition with the i64 tensor) and N = 8192 at base2k 12,
rank 1 with the sizes of tests/test_gpu_ckks_linear.py's chain (the pipeline with the 16-bit tensor); batch 5 in waves of 2, so that the
wave loop, its remainder and the reuse of the workspace product all run.  One chain is decrypted under a real key."""
import os
import subprocess
import sys

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH_ACC, LSH_TERM, PLAIN, Ct
from poulpy_amd.layouts import VecZnx
from tests import ckks_mul_cases as cases
from tests import ckks_mul_oracle as mo
from tests import shift_oracle as so
from tests import tensor_cases as tc
from tests.core_cases import prepare
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = os.environ.get("POULPY_DBG_GRAPHS") != "0" and os.environ.get("POULPY_DBG_CANARY") != "1"
FUSED = os.environ.get("POULPY_DBG_TENSOR_FUSED") != "0" and os.environ.get("POULPY_DBG_TENSOR_COMBINE") != "0"
B, BATCH, CHUNK = 12, 5, 2
# (n, rank): the five-kernel route at N = 256, the pipeline with the 16-bit tensor at N = 8192
SHAPES = [(256, 1), (256, 2), (8192, 1)]


def _down(buf, shape):
    return buf.download(np.int64, int(np.prod(shape))).reshape(shape)


def _rand(rng, shape, normalized=True):
    h = 1 << (B - 1 if normalized else B + 3)
    return rng.integers(-h, h, shape, dtype=np.int64)


def _vec(x):
    return VecZnx(x.shape[2], x.shape[1], x.shape[0], np.ascontiguousarray(x))


class Setup:
    """a ring, a rank and a random tensor key prepared for the oracle and the device; sizes after test_ckks_chain_multiply_rescale_add_add_pt_on_device"""

    def __init__(self, mods, n, rank, seed):
        from poulpy_amd.hal import GlweOpParams, GlweTensorParams
        self.n, self.rank, self.cols = n, rank, rank + 1
        self.ref, self.hip = mods(n)
        self.rng = seeded(seed)
        self.a_size, self.b_size, self.t_size, self.off, self.key_size, self.dnum, self.size = 4, 3, 5, 5, 5, 5, 4
        mat = cases.random_tensor_key(self.rng, n, B, rank, self.dnum, self.key_size)
        self.pr, self.ph = prepared_key(self.ref, self.hip, mat)
        self.tsk = mo.Tsk(self.pr, 1, B)
        self.GlweOpParams, self.GlweTensorParams = GlweOpParams, GlweTensorParams

    def params(self, square=False):
        bs = self.a_size if square else self.b_size
        tp = self.GlweTensorParams(rank=self.rank, a_size=self.a_size, b_size=bs, ab_base2k=B, a_effective_k=B * self.a_size - 3,
                                   b_effective_k=B * bs - (3 if square else 0), res_size=self.t_size, res_base2k=B, cnv_offset=self.off)
        rp = self.GlweOpParams(rank=self.rank, dnum=self.dnum, dsize=1, key_size=self.key_size, key_base2k=B, a_size=self.t_size, a_base2k=B,
                               res_size=self.size, res_base2k=B, rank_out=self.rank)
        return tp, rp

    def product(self, a, b, square):
        """the oracle's product of one ciphertext pair: the first a_size / b_size limbs of the containers a, b"""
        out = VecZnx(self.n, self.cols, self.size)
        bs = self.a_size if square else self.b_size
        mo.product(self.ref, self.off, out, B, mo.compact(_vec(a), self.a_size), B * self.a_size - 3,
                   None if square else mo.compact(_vec(b), bs), B * bs, self.t_size, self.tsk)
        return out

    def check_route(self, notes):
        if FUSED:
            assert (tc.NOTE_T16 in notes) == (self.n == 8192), (self.n, notes)


def _entry(s, dev, d_res, d_a, d_b, mode, **kw):
    tp, rp = s.params(mode == "square")
    s.hip.glwe_tensor_mul_relinearize_acc_batched(d_res.ptr if hasattr(d_res, "ptr") else d_res, d_a.ptr if hasattr(d_a, "ptr") else d_a,
                                                  None if d_b is None else d_b.ptr, dev.key_buf.ptr, tp, rp, mode, BATCH, **kw)


@pytest.mark.parametrize("mode", ["apply", "square"])
@pytest.mark.parametrize("n,rank", SHAPES)
def test_strided_operands_equal_the_existing_call_on_compacted_copies(mods, n, rank, mode):
    """containers of 6 limbs with 4 (3 for b) used, the unused limbs full of garbage: the digits of pz_glwe_tensor_mul_relinearize_batched on
    compacted copies, and of the oracle"""
    s = Setup(mods, n, rank, 100 + rank)
    square = mode == "square"
    a = _rand(s.rng, (BATCH, 6, s.cols, n))
    b = _rand(s.rng, (BATCH, 6, s.cols, n))
    want = np.stack([s.product(a[t], b[t], square).data for t in range(BATCH)])
    shape = want.shape
    with on_device(s.hip, chunk=CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a, d_b = dev.upload(a), dev.upload(b)
        d_ac, d_bc = dev.upload(a[:, :s.a_size]), dev.upload(b[:, :s.b_size])
        d_r, d_rc = dev.alloc(want.nbytes), dev.alloc(want.nbytes)
        s.hip.dispatch_notes(reset=True)
        _entry(s, dev, d_r, d_a, None if square else d_b, mode, a_stride=6, b_stride=6)
        s.hip.sync()
        s.check_route(s.hip.dispatch_notes())
        tp, rp = s.params(square)
        s.hip.glwe_tensor_mul_relinearize_batched(d_rc.ptr, d_ac.ptr, None if square else d_bc.ptr, dev.key_buf.ptr, tp, rp, mode, BATCH)
        s.hip.sync()
        got, old = _down(d_r, shape), _down(d_rc, shape)
    assert np.array_equal(got, old), "strided != the existing call on compacted copies"
    assert np.array_equal(got, want), "device != oracle"


@pytest.mark.parametrize("n,rank", SHAPES)
def test_in_place_forms_and_alias_refusals(mods, n, rank):
    """res == a, res == b, res == a == b (square) at equal strides give the out-of-place digits; a partial overlap, or res == a at another
    stride, is PZ_ERR_ALIAS and res stays as it was"""
    from poulpy_amd.hal import PoulpyHipError
    s = Setup(mods, n, rank, 200 + rank)
    # the operand that is res sits in a container of res's size (4 limbs); b uses 3 of them
    a = _rand(s.rng, (BATCH, s.size, s.cols, n))
    b = _rand(s.rng, (BATCH, s.size, s.cols, n))
    want = np.stack([s.product(a[t], b[t], False).data for t in range(BATCH)])
    want_sq = np.stack([s.product(a[t], None, True).data for t in range(BATCH)])
    shape = want.shape
    with on_device(s.hip, chunk=CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        for label, alias, mode, w in (("res == a", "a", "apply", want), ("res == b", "b", "apply", want), ("res == a == b", "a", "square", want_sq)):
            d_a, d_b = dev.upload(a), dev.upload(b)
            d_r = d_a if alias == "a" else d_b
            _entry(s, dev, d_r, d_a, None if mode == "square" else d_b, mode, a_stride=s.size, b_stride=s.size)
            s.hip.sync()
            assert np.array_equal(_down(d_r, shape), w), label
            dev.free(d_a)
            dev.free(d_b)
        # refusals: nothing is launched, res keeps its bytes
        big = _rand(s.rng, (BATCH + 1, 6, s.cols, n))
        d_big, d_b = dev.upload(big), dev.upload(b)
        ct4 = s.size * s.cols * n * 8
        for label, res_ptr, a_ptr, kw in (("res == a at another stride", d_big.ptr, d_big.ptr, dict(a_stride=6, b_stride=s.size)),
                                          ("partial overlap", d_big.ptr.value + ct4, d_big.ptr, dict(a_stride=s.size, b_stride=s.size)),
                                          ("accumulate with res == a", d_big.ptr, d_big.ptr, dict(a_stride=s.size, b_stride=s.size, accumulate=True))):
            with pytest.raises(PoulpyHipError, match=r"\[-4\]"):
                tp, rp = s.params(False)
                s.hip.glwe_tensor_mul_relinearize_acc_batched(res_ptr, a_ptr, d_b.ptr, dev.key_buf.ptr, tp, rp, "apply", BATCH, **kw)
            s.hip.sync()
            assert np.array_equal(_down(d_big, big.shape), big), label
        for label, kw in (("stride below the size", dict(a_stride=3)), ("plain join with k", dict(accumulate=True, join="plain", k=1)),
                          ("bad sign", dict(accumulate=True, sign=2)), ("bad join", dict(accumulate=True, join=7))):
            d_r = dev.alloc(want.nbytes)
            with pytest.raises(PoulpyHipError, match=r"\[-1\]"):
                _entry(s, dev, d_r, d_big, d_b, "apply", **kw)
            s.hip.sync()
            assert np.all(_down(d_r, shape) == 0x5A5A5A5A5A5A5A5A), label
            dev.free(d_r)


JOINS = [(PLAIN, 0), (LSH_TERM, 7), (LSH_TERM, B + 5), (LSH_ACC, 7), (LSH_ACC, B + 5)]


def _accumulate(s, hip, mode, joins, canary_label=None):
    """every join kind with both signs, normalize 0 and 1 (res starting from un-normalized limbs with normalize 1): device == the oracle's
    product-then-join"""
    square = mode == "square"
    n = s.n
    a = _rand(s.rng, (BATCH, 6, s.cols, n))
    b = _rand(s.rng, (BATCH, s.b_size, s.cols, n))
    prods = [s.product(a[t], b[t], square) for t in range(BATCH)]
    shape = (BATCH, s.size, s.cols, n)
    bad = []
    with on_device(hip, chunk=CHUNK) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a, d_b = dev.upload(a), dev.upload(b)
        for join, k in joins:
            for sign in (1, -1):
                for normalize in (1, 0):
                    r0 = _rand(s.rng, shape, normalized=not normalize)
                    want = r0.copy()
                    for t in range(BATCH):
                        v = _vec(want[t])
                        mo.join(s.ref, B, v, prods[t], join, k, sign, bool(normalize))
                        want[t] = v.data
                    d_r = dev.upload(r0)
                    hip.dispatch_notes(reset=True)
                    _entry(s, dev, d_r, d_a, None if square else d_b, mode, a_stride=6, accumulate=True, join=join, k=k, sign=sign, normalize=normalize)
                    hip.sync()
                    notes = hip.dispatch_notes()
                    assert ("k_glwe_sum" in notes) == bool(normalize) and ("k_glwe_combine" in notes) == (not normalize), notes
                    s.check_route(notes)
                    if not np.array_equal(_down(d_r, shape), want):
                        bad.append((join, k, sign, normalize))
                    dev.free(d_r)
    return bad


@pytest.mark.parametrize("mode", ["apply", "square"])
@pytest.mark.parametrize("n,rank", SHAPES)
def test_accumulate_equals_product_then_join(mods, n, rank, mode):
    s = Setup(mods, n, rank, 300 + rank)
    assert _accumulate(s, s.hip, mode, JOINS) == []


CANARY_CHILD = r"""
import sys
sys.path.insert(0, %r)
from tests import test_gpu_ckks_mul as t
from oracle.ref import RefModule
from poulpy_amd.hal import Module
cache = {}
def mods(n):
    if n not in cache:
        cache[n] = (RefModule(n), Module(n))
    return cache[n]
for n, rank in ((256, 2), (8192, 1)):
    s = t.Setup(mods, n, rank, 400 + rank)
    assert t._accumulate(s, s.hip, "apply", [(t.LSH_TERM, 7), (t.LSH_ACC, 17)]) == []
print("guarded run ok", flush=True)
"""


def test_workspace_guards():
    """the workspace segment of the product, and every other segment of the call, under POULPY_DBG_CANARY"""
    env = dict(os.environ, POULPY_DBG_CANARY="1")
    out = subprocess.run([sys.executable, "-c", CANARY_CHILD % ROOT], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "WORKSPACE OVERRUN" not in out.stderr and "guarded run ok" in out.stdout


@pytest.mark.parametrize("n,rank", [(256, 1), (8192, 1)])
def test_replayed_in_a_graph_with_new_operands_behind_the_same_pointers(mods, n, rank):
    s = Setup(mods, n, rank, 500 + rank)
    shape = (BATCH, s.size, s.cols, n)
    with on_device(s.hip, chunk=CHUNK, graphs=True) as dev:
        dev.key_buf = dev.key(s.ph)
        d_a = dev.alloc(BATCH * 6 * s.cols * n * 8)
        d_b = dev.alloc(BATCH * s.b_size * s.cols * n * 8)
        d_r = dev.alloc(int(np.prod(shape)) * 8)
        before = s.hip.graph_launches()
        for it in range(5):
            a = _rand(s.rng, (BATCH, 6, s.cols, n))
            b = _rand(s.rng, (BATCH, s.b_size, s.cols, n))
            r0 = _rand(s.rng, shape)
            d_a.upload(a), d_b.upload(b), d_r.upload(r0)
            want = r0.copy()
            for t in range(BATCH):
                v = _vec(want[t])
                mo.join(s.ref, B, v, s.product(a[t], b[t], False), LSH_TERM, 9, -1, True)
                want[t] = v.data
            _entry(s, dev, d_r, d_a, d_b, "apply", a_stride=6, accumulate=True, join=LSH_TERM, k=9, sign=-1, normalize=1)
            s.hip.sync()
            assert np.array_equal(_down(d_r, shape), want), ("call", it)
        if GRAPHS:
            assert s.hip.graph_launches() > before, "no call was replayed as a graph"


# ---- the plans -----------------------------------------------------------------------------------------------------------------------------
def _plan_setup(mods, n, rank, seed, limbs):
    ref, hip = mods(n)
    rng = seeded(seed)
    mat = cases.random_tensor_key(rng, n, B, rank, limbs, limbs + 1)
    pr, ph = prepared_key(ref, hip, mat)
    return ref, hip, rng, mo.Tsk(pr, 1, B), ph, (limbs, 1, limbs + 1, B)


def _batch(rng, n, ct):
    """BATCH containers of ct's layout: (host Cts, the stacked array)"""
    hs = [cases.fill_ct(rng, n, ct) for _ in range(BATCH)]
    return hs, np.stack([h.data.data for h in hs])


@pytest.mark.parametrize("n,rank", SHAPES)
def test_mul_square_and_mul_add_plans_on_device(mods, n, rank):
    """every plan of one product, launched on `BATCH` ciphertexts in waves of 2 == run_mul_plan on the oracle, with its metadata"""
    limbs = 5
    ref, hip, rng, tsk, ph, tsk_meta = _plan_setup(mods, n, rank, 600 + rank, limbs)
    cols = rank + 1
    bad = []
    with on_device(hip, chunk=CHUNK) as dev:
        d_k = dev.key(ph)
        for label, dsize, a, b in cases.mul_scenarios(B, cols, limbs):
            forms = [("mul_into", lambda d: ckks.plan_mul_into(d, a, b), dsize, ("a", "b")),
                     ("square_into", lambda d: ckks.plan_square_into(d, a), dsize, ("a",)),
                     ("mul_assign", lambda d: ckks.plan_mul_assign(d, b), None, ("b",)),
                     ("square_assign", lambda d: ckks.plan_square_assign(d), None, ()),
                     ("mul_add_ct", lambda d: ckks.plan_mul_add_ct(d, a, b), dsize, ("a", "b")),
                     ("mul_sub_ct", lambda d: ckks.plan_mul_sub_ct(d, a, b), dsize, ("a", "b"))]
            for name, make, size, uses in forms:
                # the _assign forms: dst is the first operand, in its own container; the composites: dst at a budget that shifts the join
                if size is None:
                    dst0 = Ct(B, a.size, a.log_delta, a.log_budget, cols)
                elif name.startswith("mul_a") or name.startswith("mul_s"):
                    dst0 = Ct(B, size, cases.D, 11, cols)
                else:
                    dst0 = Ct(B, size, 0, 0, cols)
                plan = make(Ct(B, dst0.size, dst0.log_delta, dst0.log_budget, cols))
                hd, d_arr = _batch(rng, n, dst0)
                ha, a_arr = _batch(rng, n, a)
                hb, b_arr = _batch(rng, n, b)
                for t in range(BATCH):
                    oa, ob = (hb[t], None) if plan.which == ("dst", "a") else (ha[t], hb[t])   # mul_assign(dst, b): the plan's "a" is b
                    mo.run_mul_plan(ref, plan, hd[t], oa, ob, tsk)
                want = np.stack([h.data.data for h in hd])
                d_d, d_a, d_b = dev.upload(d_arr), dev.upload(a_arr), dev.upload(b_arr)
                dd = Ct(B, dst0.size, dst0.log_delta, dst0.log_budget, cols, d_d.ptr)
                kw = {}
                if "a" in plan.which:
                    kw["a"] = Ct(B, a.size, a.log_delta, a.log_budget, cols, d_a.ptr)
                if "b" in plan.which:
                    kw["b"] = Ct(B, b.size, b.log_delta, b.log_budget, cols, d_b.ptr)
                if plan.which == ("dst", "a"):                      # mul_assign(dst, b): the plan's "a" is the other operand
                    kw = {"a": Ct(B, b.size, b.log_delta, b.log_budget, cols, d_b.ptr)}
                plan.launch(hip, dd, BATCH, tsk_ptr=d_k.ptr, tsk=tsk_meta, **kw)
                hip.sync()
                got = _down(d_d, want.shape)
                if not np.array_equal(got, want) or (dd.log_delta, dd.log_budget) != (hd[0].log_delta, hd[0].log_budget):
                    bad.append((label, name))
                for buf in (d_d, d_a, d_b):
                    dev.free(buf)
    assert not bad, bad


@pytest.mark.parametrize("n,rank", [(256, 1), (256, 2), (8192, 1)])
def test_mul_many_plans_on_device(mods, n, rank):
    """mul_many at n = 1, 2, 4 and 5 inputs, input 2 one limb short at n = 4: the plan's nodes on the device == the same nodes on the oracle
    == the literal recursion"""
    limbs = 8
    ref, hip, rng, tsk, ph, tsk_meta = _plan_setup(mods, n, rank, 700 + rank, limbs)
    cols = rank + 1
    K = limbs * B
    scen = [("n = %d" % k, limbs, [cases.fresh(B, K, cols) for _ in range(k)]) for k in (1, 2, 4, 5)]
    scen.append(("n = 4, input 2 one limb short", limbs, [cases.fresh(B, K - B + 1 if i == 2 else K, cols) for i in range(4)]))
    batch = 3 if n == 8192 else BATCH
    with on_device(hip, chunk=CHUNK) as dev:
        d_k = dev.key(ph)
        for label, dsize, inputs in scen:
            plan = ckks.plan_mul_many(Ct(B, dsize, 0, 0, cols), inputs)
            hin = [[cases.fill_ct(rng, n, x) for x in inputs] for _ in range(batch)]
            want = []
            for t in range(batch):
                d1 = Ct(B, dsize, 0, 0, cols, VecZnx(n, cols, dsize))
                d2 = Ct(B, dsize, 0, 0, cols, VecZnx(n, cols, dsize))
                mo.run_mul_many_plan(ref, plan, d1, hin[t], tsk)
                mo.ckks_mul_many(ref, d2, hin[t], tsk)
                assert np.array_equal(d1.data.data, d2.data.data) and (d1.log_delta, d1.log_budget) == (d2.log_delta, d2.log_budget), label
                want.append(d1.data.data)
            want = np.stack(want)
            bufs = [dev.upload(np.stack([hin[t][i].data.data for t in range(batch)])) for i in range(len(inputs))]
            d_in = [Ct(B, x.size, x.log_delta, x.log_budget, cols, bufs[i].ptr) for i, x in enumerate(inputs)]
            d_d = dev.alloc(want.nbytes)
            nbytes = plan.scratch_bytes(batch, n)
            d_tmp = dev.alloc(nbytes) if nbytes else None
            dd = Ct(B, dsize, 0, 0, cols, d_d.ptr)
            plan.launch(hip, dd, batch, d_in, tsk_ptr=d_k.ptr, tsk=tsk_meta, tmp=None if d_tmp is None else d_tmp.ptr)
            hip.sync()
            assert np.array_equal(_down(d_d, want.shape), want), label
            assert (dd.log_delta, dd.log_budget) == (plan.log_delta, plan.log_budget)
            for buf in bufs + [d_d] + ([d_tmp] if d_tmp is not None else []):
                dev.free(buf)


def test_compact_limbs_copy_on_device(mods):
    n, cols = 256, 2
    ref, hip = mods(n)
    rng = seeded(800)
    src = Ct(B, 6, 20, 25, cols)                                     # effective_k 45: 4 limbs
    hs, arr = _batch(rng, n, src)
    dst = Ct(B, 4, 0, 0, cols)
    plan = ckks.plan_compact_limbs_copy(dst, src)
    with on_device(hip) as dev:
        d_s, d_d = dev.upload(arr), dev.alloc(BATCH * 4 * cols * n * 8)
        dd = Ct(B, 4, 0, 0, cols, d_d.ptr)
        plan.launch(hip, dd, BATCH, Ct(B, 6, 20, 25, cols, d_s.ptr))
        hip.sync()
        assert np.array_equal(_down(d_d, (BATCH, 4, cols, n)), arr[:, :4]) and (dd.log_delta, dd.log_budget) == (20, 25)


# ---- one decrypted chain -------------------------------------------------------------------------------------------------------------------
def test_square_rescale_mul_add_chain_decrypts(mods):
    """square -> rescale_assign -> mul_add_ct with a third ciphertext at N = 256 under a real key; the rescaled operand (4 of its container's
    6 limbs in use) is passed by stride, with no copy.  Every ciphertext of the batch carries the same messages under its own encryption
    noise; device == oracle bit for bit, and the result decrypts to dst + a^2 c within the host test's bounds."""
    n, rank, batch = 256, 1, 3
    ref, hip = mods(n)
    c = cases.decrypt_case(n, rank, 900, s=18)
    from tests import fhe_sk as fs
    pr, ph = prepare(ref, c.key), prepare(hip, c.key)
    tsk = mo.Tsk(pr, 1, c.B)
    E, s, size, cols = c.E, c.s, c.size, c.cols
    ma, mc, md = c.ms[0], c.ms[1], c.ms[2]
    r = 8
    # metadata of the chain
    a0 = Ct(c.B, size, cases.D, E - cases.D, cols)
    sq = Ct(c.B, size, 0, 0, cols)
    p_sq = ckks.plan_square_into(sq, a0)
    p_sq.apply_meta(sq)
    p_rs = ckks.plan_rescale_assign(sq, r)
    p_rs.apply_meta(sq)
    cc = Ct(c.B, size, cases.D, E - cases.D, cols)
    assert sq.effective_k == E - cases.D - r and -(-sq.effective_k // c.B) == 4 < sq.size
    # a^2 c stands at 2^-(E - 2 s - sc - r) with c = mc 2^sc; dst holds md in the same unit, 5 bits of budget above the product's
    sc = 16
    bits = E - 2 * s - sc - r
    prod_budget = sq.log_budget - cases.D
    dst = Ct(c.B, size, cases.D, prod_budget + 5, cols)
    p_ma = ckks.plan_mul_add_ct(dst, sq, cc)
    assert (p_ma.join, p_ma.k) == (LSH_ACC, 5) and (p_ma.a_size, p_ma.a_stride) == (4, 6)
    a_all = np.stack([cases._encrypt(c.sk, ma, s, c.B, E, size, c.rng) for _ in range(batch)])
    c_all = np.stack([cases._encrypt(c.sk, mc, sc, c.B, E, size, c.rng) for _ in range(batch)])
    e_dst = dst.effective_k
    d_all = np.stack([fs.glwe_encrypt(c.sk, fs.encode(md << (e_dst - bits - 5), c.B, e_dst, size), c.B, E, c.rng) for _ in range(batch)])
    want_int = fs.mul_msg(fs.mul_msg(ma, ma), mc) + md
    want = []
    for t in range(batch):
        h_sq = Ct(c.B, size, 0, 0, cols, VecZnx(n, cols, size))
        mo.run_mul_plan(ref, p_sq, h_sq, Ct(c.B, size, cases.D, E - cases.D, cols, _vec(a_all[t])), None, tsk)
        so.run(ref, p_rs, h_sq)
        p_rs.apply_meta(h_sq)
        h_d = Ct(c.B, size, dst.log_delta, dst.log_budget, cols, _vec(d_all[t].copy()))
        mo.run_mul_plan(ref, p_ma, h_d, h_sq, Ct(c.B, size, cases.D, E - cases.D, cols, _vec(c_all[t])), tsk)
        want.append(h_d.data.data)
    want = np.stack(want)
    with on_device(hip, chunk=2) as dev:
        d_k = dev.key(ph)
        d_a, d_c, d_d = dev.upload(a_all), dev.upload(c_all), dev.upload(d_all)
        d_sq = dev.alloc(a_all.nbytes)
        g_sq = Ct(c.B, size, 0, 0, cols, d_sq.ptr)
        p_sq.launch(hip, g_sq, batch, a=Ct(c.B, size, cases.D, E - cases.D, cols, d_a.ptr), tsk_ptr=d_k.ptr, tsk=c.tsk)
        p_rs.launch(hip, g_sq, batch)
        g_d = Ct(c.B, size, dst.log_delta, dst.log_budget, cols, d_d.ptr)
        p_ma.launch(hip, g_d, batch, a=g_sq, b=Ct(c.B, size, cases.D, E - cases.D, cols, d_c.ptr), tsk_ptr=d_k.ptr, tsk=c.tsk)
        hip.sync()
        got = _down(d_d, want.shape)
    assert np.array_equal(got, want), "device != oracle"
    assert (g_d.log_delta, g_d.log_budget) == (cases.D, prod_budget)
    for t in range(batch):
        cases.check_decrypt(f"square -> rescale -> mul_add [{t}]", c, got[t], want_int, bits, p_ma.cnv_offset)
