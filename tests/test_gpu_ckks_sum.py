"""GPU: pz_glwe_sum_batched and the plans built on it (poulpy_amd/ckks.py: add_many, the products, composites and dot products by plaintext
vectors), every output byte-equal to the restatement of the reference (tests/ckks_sum_oracle.py): poulpy-ckks
leveled/delegates/composite.rs ckks_add_many, ckks_mul_add / mul_sub_pt_vec_znx_into, ckks_dot_product_pt_vec_znx and leveled/default/mul.rs
ckks_mul_pt_vec_znx_into / _assign.  The chains and scenarios are tests/ckks_sum_cases.py's (what the scenarios cover is asserted on the
host, tests/test_ckks_sum_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH_ACC, LSH_TERM, PLAIN, Ct, Pt
from poulpy_amd.layouts import VecZnx
from tests import ckks_sum_cases as cases
from tests import ckks_sum_oracle as so_sum
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64


def _down(buf, shape):
    return buf.download(np.int64, int(np.prod(shape))).reshape(shape)


# ---- the entry point on random chains ---------------------------------------------------------------------------------------------------------
def _chain_case(rng, ref, n, cols, B, res_size, nterms, normalized, batch, inplace=False, acc_shift=None, res_k=None):
    """-> (res0 (batch, res_size, cols, n), [(array (batch | 1, a_size, cols, n) | None for res, join, k, sign, shared)], want)"""
    res0 = np.stack([cases.fill(rng, VecZnx(n, cols, res_size), B, normalized).data for _ in range(batch)])
    shape = cases.random_chain(rng, n, cols, B, res_size, nterms, normalized, VecZnx(n, cols, res_size) if inplace else None, acc_shift, res_k=res_k)
    shared_at = int(rng.integers(1 if inplace else 0, nterms)) if nterms > 1 else -1
    terms = []
    for u, (a, join, k, sign) in enumerate(shape):
        if inplace and u == 0:
            terms.append((None, join, k, sign, False))
            continue
        count = 1 if u == shared_at else batch
        arr = np.stack([cases.fill(rng, VecZnx(n, cols, a.size), B, normalized).data for _ in range(count)])
        terms.append((arr, join, k, sign, u == shared_at))
    want = np.empty_like(res0)
    for t in range(batch):
        res = VecZnx(n, cols, res_size, res0[t].copy())
        chain = [(res if arr is None else VecZnx(n, cols, arr.shape[1], arr[0 if sh else t].copy()), j, k, s) for arr, j, k, s, sh in terms]
        so_sum.sum_chain(ref, B, res, chain)
        want[t] = res.data
    return res0, terms, want


def _run_chain(hip, B, res0, terms):
    batch, res_size, cols, n = res0.shape
    with on_device(hip) as dev:
        d_res = dev.upload(res0)
        call = []
        for arr, join, k, sign, sh in terms:
            ptr = d_res.ptr if arr is None else dev.upload(arr).ptr
            call.append(dict(a=ptr, a_size=res_size if arr is None else arr.shape[1], shared=sh, join=join, k=k, sign=sign))
        hip.glwe_sum_batched(d_res.ptr, cols, res_size, B, call, batch)
        hip.sync()
        return _down(d_res, res0.shape)


@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "unnormalized"])
@pytest.mark.parametrize("B", [12, 17, 50])
def test_sum_batched_random_chains(mods, B, normalized):
    """batch 3 at N = 64 (3 x cols x 32 threads: the last workgroup is partly filled); res_cols 2 and 3; res_size 1, 3, 5; a_size 1 .. 7; 1, 2,
    5 and 64 terms; random joins and signs, shifts 0 .. 3 base2k; one shared operand"""
    ref, hip = mods(N)
    rng = seeded(77 * B + normalized)
    bad, joins, steps_out = [], set(), False
    for cols in (2, 3):
        for res_size in (1, 3, 5):
            for nterms in (1, 2, 5, 64):
                res0, terms, want = _chain_case(rng, ref, N, cols, B, res_size, nterms, normalized, 3)
                got = _run_chain(hip, B, res0, terms)
                if not np.array_equal(got, want):
                    bad.append((cols, res_size, nterms))
                joins |= {(j, k % B == 0) for _, j, k, _, _ in terms}
                steps_out |= any(j == LSH_TERM and k // B >= max(res_size, arr.shape[1]) for arr, j, k, _, _ in terms)
    assert not bad, bad
    assert joins >= {(PLAIN, True), (LSH_TERM, True), (LSH_TERM, False), (LSH_ACC, True), (LSH_ACC, False)} and steps_out


@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "unnormalized"])
def test_term0_may_be_res(mods, normalized):
    """term 0 = res itself, the partial sum a chunked dot product continues from: without a shift it is read limb by limb ahead of the
    store; where a later PZ_JOIN_LSH_ACC shifts it, or its own PZ_JOIN_LSH_TERM by a limb or more, its limbs are staged in LDS"""
    ref, hip = mods(N)
    rng = seeded(311 + normalized)
    bad = []
    for B in (12, 50):
        for res_size in (1, 3, 5):
            for acc_shift, res_k in ((False, None), (True, None), (False, B + 3), (True, 2 * B)):
                res0, terms, want = _chain_case(rng, ref, N, 2, B, res_size, 5, normalized, 3, inplace=True, acc_shift=acc_shift, res_k=res_k)
                assert any(j == LSH_ACC for _, j, _, _, _ in terms[1:]) == acc_shift
                assert terms[0][:3] == ((None, PLAIN, 0) if res_k is None else (None, LSH_TERM, res_k))
                if not np.array_equal(_run_chain(hip, B, res0, terms), want):
                    bad.append((B, res_size, acc_shift, res_k))
    assert not bad, bad


def test_refusals_return_their_code_and_launch_nothing(mods):
    from poulpy_amd import abi
    from poulpy_amd.hal import PoulpyHipError
    n, cols, size, B, batch = N, 2, 3, 12, 2
    ref, hip = mods(n)
    rng = seeded(5)
    r0 = np.stack([cases.fill(rng, VecZnx(n, cols, 40), B, True).data for _ in range(batch)])
    a0 = np.stack([cases.fill(rng, VecZnx(n, cols, 40), B, True).data for _ in range(batch)])
    with on_device(hip) as dev:
        d_r, d_a = dev.upload(r0), dev.upload(a0)
        t = dict(a=d_a.ptr, a_size=size)
        INV, ALIAS, UNS = abi.PZ_ERR_INVALID, abi.PZ_ERR_ALIAS, abi.PZ_ERR_UNSUPPORTED
        bad = [([], {}, INV),                                                     # no term
               ([t] * 5, {"base2k": 61}, INV),                                    # 5 > 2^(63 - 61): ensure_accumulation_fits
               ([t] * 65, {"base2k": 58}, INV),                                   # 65 > 2^(63 - 58) = 32 comes before the 64-term limit
               ([dict(t, a_size=0)], {}, INV), ([dict(t, a_size=4097)], {}, INV),  # sizes
               ([t], {"res_size": 0}, INV), ([t], {"res_size": 4097}, INV), ([t], {"base2k": 64}, INV), ([t], {"base2k": 0}, INV),
               ([t], {"res_cols": 0}, INV), ([t], {"res_cols": 65}, INV),
               ([t, dict(t, join="lsh_term", k=(1 << 40) + 1)], {}, INV),         # shifts
               ([t, dict(t, join="lsh_acc", k=(1 << 40) + 1)], {}, INV),
               ([t, dict(t, join="plain", k=3)], {}, INV),                        # k != 0 on a plain join
               ([t, dict(t, join=7)], {}, INV), ([dict(t, sign=2)], {}, INV), ([dict(t, sign=0)], {}, INV),
               ([dict(t, a=d_a.at(8))], {}, INV),                                 # alignment
               ([t] * 65, {}, UNS),                                               # more than 64 terms
               ([dict(t, a=d_r.at(8 * n))], {}, ALIAS),                           # overlaps res without being res
               ([t, dict(t, a=d_r.ptr)], {}, ALIAS),                              # res itself, but not as term 0
               ([dict(t, a=d_r.ptr, a_size=2)], {}, ALIAS),                       # res with another limb count
               ([dict(t, a=d_r.ptr, shared=True)], {}, ALIAS),                    # res as a shared operand
               # term 0 = res shifted by a later join: staged up to 32 limbs, refused beyond (the header says so)
               ([dict(t, a=d_r.ptr, a_size=33), dict(t, join="lsh_acc", k=B)], {"res_size": 33}, ALIAS)]
        for terms, kw, code in bad:
            with pytest.raises(PoulpyHipError) as e:
                hip.glwe_sum_batched(d_r.ptr, kw.get("res_cols", cols), kw.get("res_size", size), kw.get("base2k", B), terms, batch)
            assert str(e.value).startswith("[%d]" % code), (len(terms), terms and {k: v for k, v in terms[-1].items() if k != "a"}, kw, str(e.value))
        hip.sync()
        assert np.array_equal(_down(d_r, r0.shape), r0)
        # at the limits it runs: 32 staged limbs, shifted by one limb and one bit
        res0 = r0[:, :32].copy()
        want = np.empty_like(res0)
        for b in range(batch):
            res = VecZnx(n, cols, 32, res0[b].copy())
            so_sum.sum_chain(ref, B, res, [(res, PLAIN, 0, 1), (VecZnx(n, cols, size, a0[b, :size].copy()), LSH_ACC, B + 1, -1)])
            want[b] = res.data
        d_r32, d_a3 = dev.upload(res0), dev.upload(a0[:, :size])
        hip.glwe_sum_batched(d_r32.ptr, cols, 32, B, [dict(a=d_r32.ptr, a_size=32), dict(a=d_a3.ptr, a_size=size, join="lsh_acc", k=B + 1, sign=-1)], batch)
        hip.sync()
        assert np.array_equal(_down(d_r32, res0.shape), want)


# ---- the plans -----------------------------------------------------------------------------------------------------------------------------------
def _host_batch(rng, n, ct, batch):
    return [cases.materialize(rng, n, ct) for _ in range(batch)]


def _stack(cts):
    return np.stack([c.data.data for c in cts])


def _dev_ct(ct, buf):
    return Ct(ct.base2k, ct.size, ct.log_delta, ct.log_budget, ct.cols, buf.ptr)


@pytest.mark.parametrize("B", [12, 17])
def test_add_many_both_routes(mods, B):
    """every scenario by ONE pz_glwe_sum_batched and by the chain of pz_glwe_combine_batched calls: the oracle's bytes and metadata"""
    ref, hip = mods(N)
    batch, bad = 3, []
    for i, (label, dst, inputs) in enumerate(cases.add_many_scenarios(B)):
        rng = seeded(B * 53 + i)
        ins = [_host_batch(rng, N, x, batch) for x in inputs]
        d0 = _host_batch(rng, N, dst, batch)
        want = []
        for t in range(batch):
            w = cases.clone(d0[t])
            so_sum.ckks_add_many(ref, w, [x[t] for x in ins])
            want.append(w)
        for route in ("sum", "chain"):
            with on_device(hip) as dev:
                d_dst = dev.upload(_stack(d0))
                d_in = [_dev_ct(x[0], dev.upload(_stack(x))) for x in ins]
                got = _dev_ct(dst, d_dst)
                ckks.plan_add_many(got, d_in).launch(hip, got, batch, d_in, route=route)
                hip.sync()
                if not np.array_equal(_down(d_dst, _stack(want).shape), _stack(want)) or \
                        (got.log_delta, got.log_budget) != (want[0].log_delta, want[0].log_budget):
                    bad.append((label, route))
    assert not bad, bad


def test_pt_vec_products_and_composites(mods):
    """mul_pt_vec_znx into / assign, mul_add and mul_sub, per-ciphertext and shared plaintexts"""
    B, batch = 12, 3
    ref, hip = mods(N)
    bad = []
    for i, (label, dst, a, pt) in enumerate(cases.pt_scenarios(B)):
        rng = seeded(900 + i)
        ha = _host_batch(rng, N, a, batch)
        for shared in (False, True):
            hp = [cases.materialize_pt(rng, N, pt) for _ in range(1 if shared else batch)]
            pt_of = lambda t: hp[0 if shared else t]
            for form in ("into", "assign", "add", "sub"):
                prod_budget = ckks.get_mul_pt_params(dst, a, pt)[0]
                d_meta = Ct(B, dst.size, dst.log_delta, prod_budget + 7, dst.cols) if form in ("add", "sub") else dst
                d0 = ha if form == "assign" else _host_batch(rng, N, d_meta, batch)
                want = []
                for t in range(batch):
                    w = cases.clone(d0[t])
                    if form == "into":
                        so_sum.ckks_mul_pt_vec_znx_into(ref, w, ha[t], pt_of(t))
                    elif form == "assign":
                        so_sum.ckks_mul_pt_vec_znx_into(ref, w, w, pt_of(t))
                    else:
                        so_sum.ckks_mul_add_pt_vec_znx(ref, w, ha[t], pt_of(t), sub=form == "sub")
                    want.append(w)
                with on_device(hip) as dev:
                    d_dst = dev.upload(_stack(d0))
                    d_a = _dev_ct(a, dev.upload(_stack(ha)))
                    d_pt = Pt(B, pt.size, pt.log_delta, dev.upload(np.stack([p.data.data for p in hp])).ptr, log_budget=pt.log_budget)
                    got = _dev_ct(d0[0], d_dst)
                    if form == "into":
                        ckks.plan_mul_pt_vec_znx_into(got, d_a, d_pt).launch(hip, got, batch, d_a, d_pt, pt_shared=shared)
                    elif form == "assign":
                        ckks.plan_mul_pt_vec_znx_assign(got, d_pt).launch(hip, got, batch, None, d_pt, pt_shared=shared)
                    else:
                        tmp = dev.alloc(d_dst.nbytes)
                        plan = ckks.plan_mul_add_pt_vec_znx(got, d_a, d_pt, sub=form == "sub")
                        plan.launch(hip, got, batch, d_a, d_pt, tmp.ptr, pt_shared=shared)
                        plan.apply_meta(got)
                    hip.sync()
                    if not np.array_equal(_down(d_dst, _stack(want).shape), _stack(want)) or \
                            (got.log_delta, got.log_budget) != (want[0].log_delta, want[0].log_budget):
                        bad.append((label, shared, form))
    assert not bad, bad


def _dot(ref, hip, n, dst, ops, pts, batch, seed, shared_pts, runs):
    """-> (want (batch, ...), metadata, {run: (bytes, metadata)}) for runs = [(slots, route)]"""
    rng = seeded(seed)
    hops = [_host_batch(rng, n, a, batch) for a in ops]
    hpts = [[cases.materialize_pt(rng, n, p) for _ in range(1 if shared_pts else batch)] for p in pts]
    want = []
    for t in range(batch):
        w = cases.materialize(rng, n, dst)
        so_sum.ckks_dot_product_pt_vec_znx(ref, w, [x[t] for x in hops], [p[0 if shared_pts else t] for p in hpts])
        want.append(w)
    out = {}
    shape = _stack(want).shape
    with on_device(hip) as dev:
        d_ops = [_dev_ct(a, dev.upload(_stack(x))) for a, x in zip(ops, hops)]
        d_pts = [Pt(p.base2k, p.size, p.log_delta, dev.upload(np.stack([q.data.data for q in hp])).ptr, log_budget=p.log_budget)
                 for p, hp in zip(pts, hpts)]
        for slots, route in runs:
            d_dst = dev.alloc(int(np.prod(shape)) * 8)
            tmp = dev.alloc(max(slots, 1) * int(np.prod(shape)) * 8)
            got = _dev_ct(dst, d_dst)
            plan = ckks.plan_dot_product_pt_vec_znx(got, d_ops, d_pts)
            plan.launch(hip, got, batch, d_ops, d_pts, tmp=tmp.ptr, slots=slots, pt_shared=range(len(pts)) if shared_pts else (), route=route)
            hip.sync()
            out[(slots, route)] = (_down(d_dst, shape), (got.log_delta, got.log_budget))
            dev.free(tmp)
            dev.free(d_dst)
    return _stack(want), (want[0].log_delta, want[0].log_budget), out


@pytest.mark.parametrize("B", [12, 17])
def test_dot_product_slots_and_routes(mods, B):
    """N = 64, the per-op product path: slots = 1, 2 and n give identical bytes, by the one-pass join and by the chain"""
    ref, hip = mods(N)
    bad = []
    for i, (label, dst, ops, pts) in enumerate(cases.dot_scenarios(B)):
        n = len(ops)
        runs = [(s, r) for s in sorted({1, min(2, n), n}) for r in ("sum", "chain")]
        want, meta, out = _dot(ref, hip, N, dst, ops, pts, 3, B * 17 + i, shared_pts=i % 2 == 1, runs=runs)
        bad += [(label, run) for run, (got, m) in out.items() if not np.array_equal(got, want) or m != meta]
    assert not bad, bad


def test_dot_product_mid_cnv_path(mods):
    """N = 8192, batch 2, 3 terms, 4-limb ciphertexts and a 2-limb shared plaintext: the products run k_mid_cnv"""
    n, B = 8192, 12
    ref, hip = mods(n)
    d = 2 * B + 3
    a4 = Ct(B, 4, d, 4 * B - d)
    ops = [a4, Ct(B, 4, d, 4 * B - d - 2), a4]
    pts = [Pt(B, 2, B + 3, log_budget=B - 3), Pt(B, 2, B + 3, log_budget=B - 3), Pt(B, 2, B + 6, log_budget=B - 6)]
    want, meta, out = _dot(ref, hip, n, Ct(B, 4, 0, 0), ops, pts, 2, 8192, shared_pts=True, runs=[(1, "sum"), (2, "sum"), (3, "sum"), (2, "chain")])
    bad = [run for run, (got, m) in out.items() if not np.array_equal(got, want) or m != meta]
    assert not bad, bad


# ---- workspace guards ------------------------------------------------------------------------------------------------------------------------------
CANARY_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from oracle.ref import RefModule
from poulpy_amd.hal import Module
from tests import ckks_sum_cases as cases
from tests import test_gpu_ckks_sum as t
ref, hip = RefModule(t.N), Module(t.N)
label, dst, ops, pts = cases.dot_scenarios(12)[2]
want, meta, out = t._dot(ref, hip, t.N, dst, ops, pts, 3, 1, shared_pts=False, runs=[(2, "sum"), (2, "chain")])
assert all(np.array_equal(got, want) and m == meta for got, m in out.values())
rng = t.seeded(3)
res0, terms, want = t._chain_case(rng, ref, t.N, 2, 12, 3, 5, True, 3, inplace=True, acc_shift=True)
assert np.array_equal(t._run_chain(hip, 12, res0, terms), want)
print("guarded run ok", flush=True)
"""


def test_workspace_guards():
    env = dict(os.environ, POULPY_DBG_CANARY="1")
    out = subprocess.run([sys.executable, "-c", CANARY_CHILD % ROOT], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "WORKSPACE OVERRUN" not in out.stderr and "guarded run ok" in out.stdout
