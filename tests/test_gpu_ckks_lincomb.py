"""GPU parity of the weighted sums by constants - pz_glwe_lincomb_const_batched through the plans of poulpy_amd/ckks.py - bit-exact on
every i64 limb against the restatement of the reference's composites (tests/ckks_lincomb_oracle.py): poulpy-ckks
leveled/delegates/composite.rs ckks_mul_add_pt_const_* / ckks_mul_sub_pt_const_* / ckks_dot_product_pt_const_znx.  The cases are
tests/ckks_lincomb_cases.py's (what they cover is asserted on the host, tests/test_ckks_lincomb_host.py)."""
import os

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import Cst, Ct
from tests import ckks_lincomb_cases as cases
from tests import ckks_lincomb_oracle as lo
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu
GRAPHS = os.environ.get("POULPY_DBG_GRAPHS") != "0" and os.environ.get("POULPY_DBG_CANARY") != "1"


def _down(buf, shape):
    return buf.download(np.int64, int(np.prod(shape))).reshape(shape)


def _plan(sc, dst, ops):
    if sc["kind"] == "dot":
        return ckks.plan_dot_product_pt_const(dst, ops, sc["csts"])
    return ckks.plan_mul_add_pt_const(dst, ops[0], sc["csts"][0], sub=sc["kind"] == "sub")


def _oracle(ref, sc, dst, ops):
    if sc["kind"] == "dot":
        lo.ckks_dot_product_pt_const(ref, dst, ops, sc["csts"])
    else:
        lo.ckks_mul_add_pt_const(ref, dst, ops[0], sc["csts"][0], sub=sc["kind"] == "sub")


def _run(ref, hip, sc, n, rank, batch, seed, pool=None, route="fused"):
    """`pool` distinct inputs tiled over the batch; -> (got, want, metadata of the device dst, of the oracle's)"""
    cols, pool = rank + 1, pool or batch
    host = cases.host_inputs(seeded(seed), sc, n, cols, pool)
    want = np.empty((pool, sc["dst"].size, cols, n), dtype=np.int64)
    for t in range(pool):
        d, ops = cases.on_host(sc, host, t, n, cols)
        _oracle(ref, sc, d, ops)
        want[t] = d.data.data
    idx = np.arange(batch) % pool
    with on_device(hip) as dev:
        d_dst = dev.upload(host["dst"][idx])
        d_ops = [dev.upload(host[i] if i in sc["shared"] else host[i][idx]) for i in range(len(sc["ops"]))]
        tmp = dev.alloc(d_dst.nbytes) if route == "composed" else None
        dst = Ct(**{**sc["dst"].__dict__, "cols": cols, "data": d_dst.ptr})
        ops = [Ct(**{**o.__dict__, "cols": cols, "data": b.ptr}) for o, b in zip(sc["ops"], d_ops)]
        plan = _plan(sc, dst, ops)
        plan.launch(hip, dst, batch, ops, sc["csts"], shared=sc["shared"], tmp=tmp.ptr if tmp else None, route=route)
        hip.sync()
        got = _down(d_dst, (batch, sc["dst"].size, cols, n))
    return got, want[idx], (dst.log_delta, dst.log_budget), (d.log_delta, d.log_budget)


# the last workgroup is partly filled in both mappings: batch * N / 128 and batch * N / 256 are not whole (or below one workgroup)
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("n,batch", [(8, 5), (64, 3), (128, 2)])
@pytest.mark.parametrize("B", [12, 19])
def test_lincomb_const_scenarios(mods, n, batch, rank, B):
    ref, hip = mods(n)
    bad = []
    for i, sc in enumerate(cases.scenarios(B)):
        got, want, meta, meta_want = _run(ref, hip, sc, n, rank, batch, seed=n + 97 * rank + 13 * i + B)
        if not np.array_equal(got, want) or meta != meta_want:
            bad.append(sc["label"])
    assert not bad, bad


def test_composed_route_is_the_same_sum(mods):
    """LincombPlan.launch_composed (pz_glwe_mul_const_batched into a scratch batch + pz_glwe_combine_batched): the route the one-pass call is
    measured against gives the same digits"""
    n, B = 64, 12
    ref, hip = mods(n)
    bad = []
    for i, sc in enumerate(cases.scenarios(B)):
        got, want, meta, meta_want = _run(ref, hip, sc, n, 1, 3, seed=500 + i, route="composed")
        if not np.array_equal(got, want) or meta != meta_want:
            bad.append(sc["label"])
    assert not bad, bad


def test_operand_may_be_res_where_res_starts_the_sum(mods):
    """mul_add(dst, dst, c): the operand is the initial accumulator itself"""
    n, B, cols, size, batch = 64, 12, 2, 4, 3
    ref, hip = mods(n)
    rng = seeded(41)
    c = cases.constant(rng, B, "both", (3, B - 3))
    sc = dict(kind="add", dst=Ct(B, size, B, B + 5), ops=[Ct(B, size, B, B + 5)], csts=[c], shared=(), wide=True)
    host = cases.host_inputs(rng, sc, n, cols, batch)
    host[0] = host["dst"]
    want = np.empty_like(host["dst"])
    for t in range(batch):
        d, ops = cases.on_host(sc, host, t, n, cols)
        _oracle(ref, sc, d, ops)
        want[t] = d.data.data
    with on_device(hip) as dev:
        d_dst = dev.upload(host["dst"])
        dst = Ct(B, size, B, B + 5, cols, d_dst.ptr)
        plan = ckks.plan_mul_add_pt_const(dst, dst, c)
        plan.launch(hip, dst, batch, [dst], [c], route="fused")
        hip.sync()
        got = _down(d_dst, want.shape)
    assert np.array_equal(got, want)


def test_refusals_return_their_code_and_launch_nothing(mods):
    from poulpy_amd import abi
    from poulpy_amd.hal import PoulpyHipError
    n, cols, size, B, batch = 64, 2, 3, 12, 2
    ref, hip = mods(n)
    rng = seeded(5)
    # res and the operand are as large as the largest shape a refused call names, so that only the overlaps asked for are overlaps
    r0 = cases.fill(rng, (batch, 97, cols, n), B, False)
    a0 = cases.fill(rng, (batch, 65, cols, n), B, False)
    re = [3, -5, 7]
    with on_device(hip) as dev:
        d_r, d_a = dev.upload(r0), dev.upload(a0)
        t = dict(a=d_a.ptr, a_size=size, cnv_offset=B, re=re, im=None)
        INV, ALIAS, UNS = abi.PZ_ERR_INVALID, abi.PZ_ERR_ALIAS, abi.PZ_ERR_UNSUPPORTED
        bad = [([], {}, INV),                                                     # no term
               ([t] * 5, {"base2k": 61}, INV),                                    # 5 > 2^(63 - 61): ensure_accumulation_fits
               ([dict(t, a_size=0)], {}, INV), ([dict(t, a_size=4097)], {}, INV),  # sizes
               ([t], {"res_size": 0}, INV), ([t], {"base2k": 64}, INV), ([t], {"base2k": 0}, INV), ([t], {"rank": 0}, INV),
               ([dict(t, b_size=0)], {}, INV), ([dict(t, b_size=4097)], {}, INV),  # digit counts
               ([dict(t, cnv_offset=8 * B)], {}, INV),                            # cnv_offset beyond the product: hi = 7 >= 3 + 3
               ([t, dict(t, join="lsh_term", k=1 << 41)], {}, INV),               # shifts
               ([t, dict(t, join="plain", k=3)], {}, INV),
               ([t, dict(t, join=7)], {}, INV), ([dict(t, sign=2)], {}, INV), ([dict(t, sign=0)], {}, INV),
               ([dict(t, a=d_r.at(8 * n))], {}, ALIAS),                           # overlaps res without being res
               ([dict(t, a=d_r.ptr)], {}, ALIAS),                                 # res itself, but the sum does not start from res
               ([dict(t, a=d_r.ptr, a_size=2)], {"init_res": True}, ALIAS),       # res with another limb count
               ([t] * 65, {}, UNS),                                               # the device table holds 64 terms
               ([dict(t, a_size=65)], {}, UNS), ([dict(t, re=[1] * 33)], {}, UNS),
               ([dict(t, a_size=16, im=re)], {"res_size": 65}, UNS),              # (16 + 65) x 2 x 1 KiB > 160 KiB
               ([dict(t, a_size=16, im=re), dict(t, a_size=16, join="lsh_term", k=5)], {"res_size": 33}, UNS),   # a shifting join: (16 + 66) x 2 KiB
               ([dict(t, a_size=64)], {"res_size": 97}, UNS)]                     # (64 + 97) x 1 KiB > 160 KiB
        for terms, kw, code in bad:
            with pytest.raises(PoulpyHipError) as e:
                hip.glwe_lincomb_const_batched(d_r.ptr, kw.get("rank", 1), kw.get("res_size", size), kw.get("base2k", B), terms,
                                               kw.get("init_res", False), kw.get("normalize", False), batch)
            assert str(e.value).startswith("[%d]" % code), (terms and {k: v for k, v in terms[-1].items() if k != "a"}, kw, str(e.value))
        hip.sync()
        assert np.array_equal(_down(d_r, r0.shape), r0)
        # at the limits it runs: (16 + 64) x 2 KiB = 160 KiB of LDS, and 64 terms.  The constant 1 at cnv_offset = base2k is the identity
        # on normalized digits: 64 copies of a, added without normalization
        hip.glwe_lincomb_const_batched(d_r.ptr, 1, 64, B, [dict(t, a_size=16, im=re)], False, False, batch)
        hip.glwe_lincomb_const_batched(d_r.ptr, 1, size, B, [dict(t, re=[1])] * 64, False, False, batch)
        hip.sync()
        a3 = a0.reshape(-1)[:batch * size * cols * n].reshape(batch, size, cols, n)
        assert np.array_equal(_down(d_r, a3.shape), 64 * a3)


def test_replayed_call_picks_up_new_constants_behind_the_same_arguments(mods):
    """The launch goes through the module's graph cache; the constants travel through the term table written in front of the graph.  The
    same pointers, shapes and joins with other digits every time: first call plain, second captured, later ones replayed - all exact."""
    n, B, cols, batch = 128, 12, 2, 3
    ref, hip = mods(n)
    rng = seeded(90)
    dst0 = Ct(B, 4, 0, 0)
    ops0 = [Ct(B, 3, B, B + 5), Ct(B, 3, B, 2 * B)]
    host = {"dst": np.zeros((batch, 4, cols, n), dtype=np.int64)}
    for i, o in enumerate(ops0):
        host[i] = np.stack([cases.fill(rng, (o.size, cols, n), B, False) for _ in range(batch)])
    with on_device(hip) as dev:
        d_dst = dev.upload(host["dst"])
        d_ops = [dev.upload(host[i]) for i in range(2)]
        served = 0
        for call in range(5):
            csts = [cases.constant(rng, B, "both", (3, B - 3)), cases.constant(rng, B, "im", (3, B - 3))]
            sc = dict(kind="dot", dst=dst0, ops=ops0, csts=csts, shared=(), wide=False)
            want = np.empty_like(host["dst"])
            for t in range(batch):
                d, ops = cases.on_host(sc, host, t, n, cols)
                _oracle(ref, sc, d, ops)
                want[t] = d.data.data
            dst = Ct(B, 4, 0, 0, cols, d_dst.ptr)
            ops = [Ct(**{**o.__dict__, "cols": cols, "data": b.ptr}) for o, b in zip(ops0, d_ops)]
            plan = ckks.plan_dot_product_pt_const(dst, ops, csts)
            before = hip.graph_launches()
            plan.launch(hip, dst, batch, ops, csts, route="fused")
            hip.sync()
            served += hip.graph_launches() - before
            assert np.array_equal(_down(d_dst, want.shape), want), call
        assert served == (4 if GRAPHS else 0)


def test_lincomb_const_pool_at_2_16(mods):
    """N = 2^16, 16 limbs, base2k 12: 24 ciphertexts from a pool of 3 - several waves of workgroups over the device in either mapping -
    a complex dot product of three terms at three budgets and a mul_sub; every output checked."""
    n, B = 65536, 12
    ref, hip = mods(n)
    rng = seeded(1616)
    metas = cases.cst_metas(B)
    terms = [cases.term(rng, B, 16, 16, b, f, m) for b, f, m in ((100, "both", metas[1]), (93, "re", metas[2]), (114, "im", metas[0]))]
    dot = dict(label="dot3", kind="dot", dst=Ct(B, 16, 0, 0), ops=[t[0] for t in terms], csts=[t[1] for t in terms], shared=(1,), wide=False)
    o, c = cases.term(rng, B, 16, 16, 100, "both", metas[1])
    sub = dict(label="mul_sub", kind="sub", dst=Ct(B, 16, B, 107), ops=[o], csts=[c], shared=(), wide=False)
    for i, sc in enumerate((dot, sub)):
        got, want, meta, meta_want = _run(ref, hip, sc, n, 1, 24, seed=2000 + i, pool=3)
        assert meta == meta_want and np.array_equal(got, want), sc["label"]
