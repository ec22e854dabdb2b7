"""GPU parity of the accumulating shifts (pz_vec_znx_{lsh_add_into,lsh_sub,rsh_add_into,rsh_sub}_batched) and of the CKKS linear operations
run as one pz_glwe_combine_batched call each (poulpy_amd/ckks.py), bit-exact on every i64 limb against the restatement of
tests/shift_oracle.py (poulpy-cpu-ref vec_znx/shift.rs, poulpy-ckks leveled/default/*.rs)."""
import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import Ct, Pt
from poulpy_amd.layouts import VecZnx
from tests import shift_oracle as so
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu


def _down(buf, shape):
    return buf.download(np.int64, int(np.prod(shape))).reshape(shape)


def _fill(rng, shape, base2k, wide):
    if wide:
        return rng.integers(-(1 << 62), 1 << 62, shape, dtype=np.int64)
    h = 1 << (base2k - 1)
    return rng.integers(-h, h, shape, dtype=np.int64)


# ---- the four accumulating shifts ---------------------------------------------------------------------------------------------------
SHIFT_OPS = {"lsh_add_into": (so.vec_znx_lsh_acc, False), "lsh_sub": (so.vec_znx_lsh_acc, True),
             "rsh_add_into": (so.vec_znx_rsh_acc, False), "rsh_sub": (so.vec_znx_rsh_acc, True)}
SIZES = [(3, 5), (4, 4), (6, 2)]
GRID = [(b, k, rs, as_) for b in (12, 17, 19, 50) for rs, as_ in SIZES
        for k in sorted({0, 1, b - 1, b, b + 1, 3 * b + 2, max(rs, as_) * b, (rs + as_ + 1) * b + 3})]


@pytest.mark.parametrize("wide", [False, True], ids=["normalized", "wide"])
@pytest.mark.parametrize("base2k,k,res_size,a_size", GRID)
def test_accumulating_shifts_batched(mods, base2k, k, res_size, a_size, wide):
    n, batch, cols = 256, 3, 2
    ref, hip = mods(n)
    rng = seeded(base2k * 7919 + k * 31 + res_size * 3 + a_size + int(wide))
    a = _fill(rng, (batch, a_size, cols, n), base2k, wide)
    r0 = _fill(rng, (batch, res_size, cols, n), base2k, wide)
    with on_device(hip) as dev:
        d_a = dev.upload(a)
        for name, (fn, sub) in SHIFT_OPS.items():
            want = r0.copy()
            for t in range(batch):
                rv = VecZnx(n, cols, res_size, want[t])
                fn(base2k, k, rv, 1, VecZnx(n, cols, a_size, a[t].copy()), 0, sub=sub)
            d_r = dev.upload(r0)
            getattr(hip, f"vec_znx_{name}_batched")(batch, base2k, k, d_r.ptr, cols, res_size, 1, d_a.ptr, cols, a_size, 0)
            hip.sync()
            got = _down(d_r, r0.shape)
            dev.free(d_r)
            assert np.array_equal(got, want), name


@pytest.mark.parametrize("base2k,k", [(12, 0), (12, 5), (12, 12), (12, 29), (19, 40), (50, 101)])
def test_accumulating_shifts_on_res_itself(mods, base2k, k):
    """a = res: the same column (the in-place walk; the operand is res as it was before the call) and another column (a plain read)."""
    n, batch, cols, size = 512, 2, 2, 5
    ref, hip = mods(n)
    rng = seeded(base2k + k)
    r0 = _fill(rng, (batch, size, cols, n), base2k, True)
    with on_device(hip) as dev:
        for name, (fn, sub) in SHIFT_OPS.items():
            for a_col in (1, 0):
                want = r0.copy()
                for t in range(batch):
                    fn(base2k, k, VecZnx(n, cols, size, want[t]), 1, VecZnx(n, cols, size, r0[t].copy()), a_col, sub=sub)
                d_r = dev.upload(r0)
                getattr(hip, f"vec_znx_{name}_batched")(batch, base2k, k, d_r.ptr, cols, size, 1, d_r.ptr, cols, size, a_col)
                hip.sync()
                got = _down(d_r, r0.shape)
                dev.free(d_r)
                assert np.array_equal(got, want), (name, a_col)


# ---- the CKKS operations -----------------------------------------------------------------------------------------------------------
def _scenarios(B):
    """(label, plan builder over the Ct / Pt objects, dst, operands {name: Ct | Pt}, names of shared operands)."""
    S = []
    for sub in (False, True):
        tag = "sub" if sub else "add"
        for budgets, dsize in ((((20, 40), (20, 40)), 6), (((20, 30), (20, 35)), 4), (((20, 35), (18, 30)), 4), (((20, 30), (20, 30)), 4)):
            (da, ba), (db, bb) = budgets
            for norm in (True, False):
                S.append((f"{tag}_into_{ba}_{bb}_{dsize}_{int(norm)}", lambda d, o, sub=sub, norm=norm: ckks.plan_add_into(d, o["a"], o["b"], sub, norm),
                          Ct(B, dsize, 0, 0), {"a": Ct(B, 5, da, ba), "b": Ct(B, 5, db, bb)}, ()))
        S.append((f"{tag}_into_shared_b", lambda d, o, sub=sub: ckks.plan_add_into(d, o["a"], o["b"], sub), Ct(B, 4, 0, 0),
                  {"a": Ct(B, 5, 20, 30), "b": Ct(B, 3, 20, 26)}, ("b",)))
        for bd, ba in ((30, 30), (25, 30), (30, 25)):
            for norm in (True, False):
                S.append((f"{tag}_assign_{bd}_{ba}_{int(norm)}", lambda d, o, sub=sub, norm=norm: ckks.plan_add_assign(d, o["a"], sub, norm),
                          Ct(B, 5, 20, bd), {"a": Ct(B, 5, 21, ba)}, ()))
        S.append((f"{tag}_pt_into", lambda d, o, sub=sub: ckks.plan_add_pt_into(d, o["a"], o["pt"], sub), Ct(B, 4, 0, 0),
                  {"a": Ct(B, 5, 20, 34), "pt": Pt(B, 2, 20)}, ("pt",)))
        S.append((f"{tag}_pt_into_off0", lambda d, o, sub=sub: ckks.plan_add_pt_into(d, o["a"], o["pt"], sub, False), Ct(B, 6, 0, 0),
                  {"a": Ct(B, 5, 20, 30), "pt": Pt(B, 3, 30)}, ()))
        S.append((f"{tag}_pt_assign", lambda d, o, sub=sub: ckks.plan_add_pt_assign(d, o["pt"], sub), Ct(B, 5, 20, 30),
                  {"pt": Pt(B, 3, 30)}, ("pt",)))
    S += [("neg_into_off", lambda d, o: ckks.plan_neg_into(d, o["a"]), Ct(B, 4, 0, 0), {"a": Ct(B, 5, 20, 40)}, ()),
          ("neg_into", lambda d, o: ckks.plan_neg_into(d, o["a"]), Ct(B, 5, 0, 0), {"a": Ct(B, 5, 20, 40)}, ()),
          ("neg_assign", lambda d, o: ckks.plan_neg_assign(d), Ct(B, 5, 20, 40), {}, ()),
          ("mul_pow2_into", lambda d, o: ckks.plan_mul_pow2_into(d, o["a"], 7), Ct(B, 4, 0, 0), {"a": Ct(B, 5, 20, 40)}, ()),
          ("mul_pow2_assign", lambda d, o: ckks.plan_mul_pow2_assign(d, 2 * B + 3), Ct(B, 5, 20, 40), {}, ()),
          ("div_pow2_into", lambda d, o: ckks.plan_div_pow2_into(d, o["a"], 5), Ct(B, 4, 0, 0), {"a": Ct(B, 5, 20, 40)}, ()),
          ("div_pow2_assign", lambda d, o: ckks.plan_div_pow2_assign(d, 5), Ct(B, 5, 20, 40), {}, ()),
          ("rescale_into", lambda d, o: ckks.plan_rescale_into(d, o["a"], B + 1), Ct(B, 5, 0, 0), {"a": Ct(B, 5, 20, 40)}, ()),
          ("rescale_assign", lambda d, o: ckks.plan_rescale_assign(d, 2 * B), Ct(B, 5, 20, 40), {}, ()),
          ("align_assign", lambda d, o: ckks.plan_align_assign(Ct(B, 5, 20, 33), d)[1], Ct(B, 5, 20, 40), {}, ())]
    return S


def _run_ckks(ref, hip, n, rank, B, label, build, dst, ops, shared, batch, seed, pool=None):
    cols = rank + 1
    rng = seeded(seed)
    pool = pool or batch
    for o in ops.values():
        if isinstance(o, Ct):
            o.cols = cols
    dst.cols = cols
    plan = build(dst, ops)
    idx = np.arange(batch) % pool
    host = {}
    for name, o in list(ops.items()) + [("dst", dst)]:
        c = 1 if isinstance(o, Pt) else cols
        m = 1 if name in shared else pool
        host[name] = np.stack([_fill(rng, (o.size, c, n), B, name == "dst" and not plan.normalize) for _ in range(m)])
    want = np.empty((pool, dst.size, cols, n), dtype=np.int64)
    for t in range(pool):
        def obj(name, o):
            arr = host[name][0 if name in shared else t].copy()
            v = VecZnx(n, arr.shape[1], o.size, arr)
            return Pt(o.base2k, o.size, o.log_delta, v) if isinstance(o, Pt) else Ct(o.base2k, o.size, o.log_delta, o.log_budget, cols, v)
        d = obj("dst", dst)
        kw = {k: obj(k, o) for k, o in ops.items()}
        so.run(ref, plan, d, kw.get("a"), kw.get("b"), kw.get("pt"))
        want[t] = d.data.data
    with on_device(hip) as scope:
        dev = {}
        for name, arr in host.items():
            full = arr if name in shared else arr[idx]
            dev[name] = scope.upload(full)
        args = {}
        for k, o in ops.items():
            args[k] = (Pt if isinstance(o, Pt) else Ct)(**{**o.__dict__, "data": dev[k].ptr})
        d_dst = Ct(**{**dst.__dict__, "data": dev["dst"].ptr})
        plan.launch(hip, d_dst, batch, args.get("a"), args.get("b"), args.get("pt"), shared=shared)
        hip.sync()
        got = _down(dev["dst"], (batch, dst.size, cols, n))
    assert (d_dst.log_delta, d_dst.log_budget) == (plan.log_delta, plan.log_budget)
    return got, want[idx]


@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("n", [1024, 4096, 65536])
@pytest.mark.parametrize("B", [12, 19])
def test_ckks_linear_ops(mods, n, rank, B):
    ref, hip = mods(n)
    batch = 3 if n < 65536 else 2
    bad = []
    for i, (label, build, dst, ops, shared) in enumerate(_scenarios(B)):
        got, want = _run_ckks(ref, hip, n, rank, B, label, build, dst, ops, shared, batch, seed=n + 97 * rank + 13 * i + B)
        if not np.array_equal(got, want):
            bad.append(label)
    assert not bad, bad


def test_ckks_pool_at_2_16(mods):
    """N = 2^16, 16 limbs, 32 ciphertexts (many waves of the kernel's workgroups over the device): every output checked."""
    n, B = 65536, 12
    ref, hip = mods(n)
    cases = [("add_into", lambda d, o: ckks.plan_add_into(d, o["a"], o["b"]), Ct(B, 16, 0, 0), {"a": Ct(B, 16, 40, 150), "b": Ct(B, 16, 40, 140)}, ()),
             ("add_pt_into", lambda d, o: ckks.plan_add_pt_into(d, o["a"], o["pt"]), Ct(B, 16, 0, 0), {"a": Ct(B, 16, 40, 150), "pt": Pt(B, 4, 40)},
              ("pt",)),
             ("rescale_assign", lambda d, o: ckks.plan_rescale_assign(d, 40), Ct(B, 16, 40, 150), {}, ())]
    for i, (label, build, dst, ops, shared) in enumerate(cases):
        got, want = _run_ckks(ref, hip, n, 1, B, label, build, dst, ops, shared, 32, seed=1000 + i, pool=3)
        assert np.array_equal(got, want), label


def test_combine_refusals_launch_nothing(mods):
    from poulpy_amd.hal import PoulpyHipError
    n, cols, size = 256, 2, 3
    ref, hip = mods(n)
    r0 = np.arange(size * cols * n, dtype=np.int64).reshape(1, size, cols, n)
    with on_device(hip) as dev:
        d_r, d_a = dev.upload(r0), dev.upload(r0 + 1)
        t = dict(a=d_a.ptr, a_size=size, kind="raw")
        bad = [([dict(t, base2k=13)], {}),                         # mixed base2k
               ([t] * 5, {}),                                      # too many terms
               ([], {}),                                           # no term
               ([dict(t, a_size=0)], {}),                          # bad sizes
               ([t], {"res_size": 0}),
               ([dict(t, kind="lsh", k=1 << 41)], {}),             # shift out of range
               ([dict(t, k=3)], {}),                               # RAW takes no shift
               ([dict(t, sign=2)], {}),
               ([dict(t, a=d_r.at(8 * n))], {}),                   # overlaps res without being res
               ([t], {"base2k": 64})]
        for terms, kw in bad:
            with pytest.raises(PoulpyHipError):
                hip.glwe_combine_batched(d_r.ptr, cols, kw.get("res_size", size), kw.get("base2k", 12), terms, False, 1)
        hip.sync()
        assert np.array_equal(_down(d_r, r0.shape), r0)
        # four terms is the limit, and it runs
        hip.glwe_combine_batched(d_r.ptr, cols, size, 12, [t] * 4, False, 1)
        hip.sync()
        assert np.array_equal(_down(d_r, r0.shape), 4 * (r0 + 1))


@pytest.mark.parametrize("rank", [1, 2])
def test_ckks_chain_multiply_rescale_add_add_pt_on_device(mods, rank):
    """A leveled CKKS step that never leaves the device: pz_glwe_tensor_mul_relinearize_batched (ckks_mul_into_default, leveled/default/mul.rs:49-85)
    -> rescale_assign -> add_into with a ciphertext at another budget -> add_pt_vec_znx_assign with a shared plaintext, every linear step one
    pz_glwe_combine_batched call; the oracle runs the reference operations one after the other on the host."""
    from poulpy_amd.hal import GlweOpParams, GlweTensorParams
    from poulpy_amd.layouts import MatZnx
    n, B, batch = 8192, 12, 4
    ref, hip = mods(n)
    rng = seeded(77 + rank)
    cols, pairs = rank + 1, rank * (rank + 1) // 2
    a_size, b_size, t_size, off, key_size, dnum, size = 4, 3, 5, 5, 5, 5, 4
    mat = MatZnx(n, dnum, pairs, cols, key_size).fill_uniform(B, rng)
    pr, ph = ref.vmp_pmat_alloc(dnum, pairs, cols, key_size), hip.vmp_pmat_alloc(dnum, pairs, cols, key_size)
    ref.vmp_prepare(pr, mat)
    hip.vmp_prepare(ph, mat)
    a_all = _fill(rng, (batch, a_size, cols, n), B, False)
    b_all = _fill(rng, (batch, b_size, cols, n), B, False)
    o_all = _fill(rng, (batch, size, cols, n), B, False)
    pt_h = _fill(rng, (1, 2, 1, n), B, False)
    # metadata: the product at log_delta 20, log_budget 28 (effective_k 48 = max_k); the other operand at budget 25; a 2-limb plaintext
    prod, other, pt = Ct(B, size, 20, 28, cols), Ct(B, size, 20, 25, cols), Pt(B, 2, 20)
    dst = Ct(B, size, 0, 0, cols)
    p_rs = ckks.plan_rescale_assign(prod, 10)
    p_rs.apply_meta(prod)
    p_add = ckks.plan_add_into(dst, prod, other)
    p_add.apply_meta(dst)
    p_pt = ckks.plan_add_pt_assign(dst, pt)
    assert [t.kind for t in p_add.terms] == [ckks.LSH, ckks.LSH] and p_pt.pt_shift == 14

    want = np.empty((batch, size, cols, n), dtype=np.int64)
    for t in range(batch):
        tmp = VecZnx(n, cols + pairs, t_size)
        ref.glwe_tensor_apply(off, tmp, B, VecZnx(n, cols, a_size, a_all[t].copy()), B * a_size, VecZnx(n, cols, b_size, b_all[t].copy()),
                              B * b_size, B)
        m = VecZnx(n, cols, size)
        ref.glwe_tensor_relinearize(m, B, tmp, B, pr, 1, B)
        mc = Ct(B, size, 20, 28, cols, m)
        so.run(ref, p_rs, mc)
        d = Ct(B, size, 0, 0, cols, VecZnx(n, cols, size))
        so.run(ref, p_add, d, Ct(B, size, 20, 18, cols, m), Ct(B, size, 20, 25, cols, VecZnx(n, cols, size, o_all[t].copy())))
        so.run(ref, p_pt, Ct(B, size, 20, 18, cols, d.data), pt=Pt(B, 2, 20, VecZnx(n, 1, 2, pt_h[0].copy())))
        want[t] = d.data.data

    with on_device(hip) as dev:
        d_a, d_b, d_o, d_pt = dev.upload(a_all), dev.upload(b_all), dev.upload(o_all), dev.upload(pt_h)
        d_k = dev.key(ph)
        d_m = dev.alloc(want.nbytes, poison=False)
        d_d = dev.alloc(want.nbytes, poison=False)
        tp = GlweTensorParams(rank=rank, a_size=a_size, b_size=b_size, ab_base2k=B, a_effective_k=B * a_size, b_effective_k=B * b_size, res_size=t_size,
                              res_base2k=B, cnv_offset=off)
        rp = GlweOpParams(rank=rank, dnum=dnum, dsize=1, key_size=key_size, key_base2k=B, a_size=t_size, a_base2k=B, res_size=size, res_base2k=B,
                          rank_out=rank)
        hip.glwe_tensor_mul_relinearize_batched(d_m.ptr, d_a.ptr, d_b.ptr, d_k.ptr, tp, rp, "apply", batch)
        m_dev = Ct(B, size, 20, 28, cols, d_m.ptr)
        p_rs.launch(hip, m_dev, batch)
        dd = Ct(B, size, 0, 0, cols, d_d.ptr)
        p_add.launch(hip, dd, batch, m_dev, Ct(B, size, 20, 25, cols, d_o.ptr))
        p_pt.launch(hip, dd, batch, pt=Pt(B, 2, 20, d_pt.ptr), shared=("pt",))
        hip.sync()
        got = _down(d_d, want.shape)
    assert (dd.log_delta, dd.log_budget) == (20, 18)
    assert np.array_equal(got, want)
