"""The device through the launches of poulpy_amd/ckks.py - Plan.launch, ConstPlan.launch (into and assign), LincombPlan.launch on both
routes, RotatePlan.launch - against what the CKKS operations MEAN (tests/ckks_meaning.py), on poulpy-ckks's own cases
(tests/ckks_meaning_cases.py).  No raw entry point is called here: the shift amounts, offsets and metadata are the plans' own.

* Keyless: every case and step, batch 3, N = 256: the device output within the allowance of the exact expectation, its reported metadata
  the independent statement's, and equal bit for bit to the host restatement; once more with the second operand shared by the batch;
  the family again at N = 4096 with 3 limbs.
* RotatePlan.launch under real keys (tests/fhe_sk.py, tests/core_cases.py): offset 0, a smaller destination (through the temporary),
  two rotations and the conjugation in one call, the missing temporary; device == the oracle's sequence bit for bit, every output
  decrypts to phi_p of its own plaintext at the new metadata within the key switch's bound, and swapped keys fail.
* A chain under one secret key: add, mul_pt_const, sub into a smaller output, rescale; decrypted against the exact integers.
"""
import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import Cst, Ct
from poulpy_amd.layouts import VecZnx
from tests import ckks_meaning as cm
from tests import ckks_meaning_cases as cc
from tests import core_cases as cs
from tests import fhe_sk as fs
from tests import shift_oracle as so
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu
BATCH = 3


def _down(buf, shape):
    return buf.download(np.int64, int(np.prod(shape))).reshape(shape)


# ---- keyless cases -----------------------------------------------------------------------------------------------------------------------
def launch(hip, st, plan, denv, shared=(), tmp=None, route=None):
    """the step through its plan's own launch; denv: containers whose .data are device pointers"""
    g = denv.get
    d = denv[st["dst"]]
    if isinstance(plan, ckks.Plan):
        align = st["op"] == "align_assign"
        plan.launch(hip, d, BATCH, None if align else g(st.get("a")), None if align else g(st.get("b")), g(st.get("pt")), shared=shared)
    elif isinstance(plan, ckks.ConstPlan):
        plan.launch(hip, d, BATCH, g(st.get("a")), st["csts"][0])
    else:
        ops = [denv[k] for k in st["ops"]] if "ops" in st else [denv[st["a"]]]
        plan.launch(hip, d, BATCH, ops, st["csts"], tmp=tmp, route=route)


def run_case(ref, hip, case, n, seed, shared=None, route=None):
    """-> the failures of the case: every step's device output against its meaning, its metadata, and the host restatement"""
    rng = seeded(seed)
    items = [cc.draw(case, rng, n) for _ in range(BATCH)]
    if shared:
        for it in items[1:]:
            it[shared[1]] = items[0][shared[1]]
    henvs = [cc.host_env(case, it, n) for it in items]
    bad = []
    with on_device(hip) as dev:
        bufs, denv = {}, {}
        for name, o in case.env.items():
            one = shared is not None and name == shared[1]
            bufs[name] = dev.upload(np.stack([it[name] for it in items[:1 if one else BATCH]]))
            denv[name] = type(o)(**{**o.__dict__, "data": bufs[name].ptr})
        for si, st in enumerate(case.steps):
            outs = [cc.step_outcome(st, env) for env in henvs]
            plan = cc.step_plan(st, denv)
            d = denv[st["dst"]]
            tmp = dev.alloc(BATCH * d.size * d.cols * n * 8) if route == "composed" else None
            launch(hip, st, plan, denv, shared=(shared[0],) if shared else (), tmp=tmp.ptr if tmp else None, route=route)
            hip.sync()
            got = _down(bufs[st["dst"]], (BATCH, d.size, d.cols, n))
            for t, (env, out) in enumerate(zip(henvs, outs)):
                cc.step_host(ref, st, cc.step_plan(st, env), env)
                if (d.log_delta, d.log_budget) != (out.log_delta, out.log_budget):
                    bad.append((case.name, si, t, "metadata", (d.log_delta, d.log_budget), (out.log_delta, out.log_budget)))
                dev_ulps = cm.deviation_ulps(got[t], out.want, d.size, d.base2k)
                if not dev_ulps <= out.allow:
                    bad.append((case.name, si, t, "deviation", dev_ulps, out.allow))
                if not np.array_equal(got[t], env[st["dst"]].data.data):
                    bad.append((case.name, si, t, "device != restatement"))
    return bad


def _good(P):
    return [c for c in cc.cases(P) if c.refuse is None]


def _lincomb(case):
    return any(st["op"] in ("mul_add_cst", "mul_sub_cst", "dot_cst") for st in case.steps)


@pytest.mark.parametrize("P", cc.SETS, ids=[P.tag for P in cc.SETS])
def test_every_case_means_what_it_must(mods, P):
    n = 256
    ref, hip = mods(n)
    bad = []
    for i, case in enumerate(_good(P)):
        bad += run_case(ref, hip, case, n, seed=31 * i + P.B, route="fused" if _lincomb(case) else None)
    assert not bad, bad[:8]


@pytest.mark.parametrize("P", cc.SETS, ids=[P.tag for P in cc.SETS])
def test_composed_route_means_the_same(mods, P):
    n = 256
    ref, hip = mods(n)
    bad = []
    for i, case in enumerate(c for c in _good(P) if _lincomb(c)):
        bad += run_case(ref, hip, case, n, seed=900 + i, route="composed")
    assert not bad, bad[:8]


def test_second_operand_shared_by_the_batch(mods):
    """one `b` / one plaintext for all three ciphertexts (Plan.launch's `shared`)"""
    n = 256
    ref, hip = mods(n)
    bad, ran = [], 0
    for i, case in enumerate(_good(cc.FFT64)):
        st = case.steps[0]
        if len(case.steps) != 1 or not st["op"].startswith(("add_into", "sub_into", "add_pt", "sub_pt")):
            continue
        role = "pt" if "pt" in st["op"] else "b"
        bad += run_case(ref, hip, case, n, seed=500 + i, shared=(role, st[role]))
        ran += 1
    assert ran >= 20 and not bad, bad[:8]


def test_the_family_at_n_4096_with_3_limbs(mods):
    n = 4096
    ref, hip = mods(n)
    bad = []
    for i, case in enumerate(_good(cc.SMALL3)):
        for route in (("fused", "composed") if _lincomb(case) else (None,)):
            bad += run_case(ref, hip, case, n, seed=4096 + i, route=route)
    assert not bad, bad[:8]


# ---- RotatePlan.launch under real keys -----------------------------------------------------------------------------------------------------
B_ROT = 12


def rotation_cases(n, limbs, dst_limbs, gals, seed):
    """one core_cases.automorphism_case per Galois element from one seed: the same secret and ciphertexts, that element's real key"""
    k = limbs * B_ROT
    out = [cs.automorphism_case(n, 1, 1, limbs, B_ROT, B_ROT, B_ROT, k, k, dst_limbs * B_ROT, 1, BATCH, seed, p=p) for p in gals]
    for c in out[1:]:
        assert np.array_equal(c.a, out[0].a) and np.array_equal(c.sk_out, out[0].sk_out)
    return out


def rotate(ref, hip, rcs, keys, log_delta, with_tmp=True):
    """the cases through plan_rotate_many / RotatePlan.launch and through the oracle's sequence (glwe_lsh into the destination layout, then
    glwe_automorphism with that key) -> (device [rotation][ciphertext], oracle alike, the destinations' containers, the source's)"""
    from poulpy_amd.hal import GlweOpParams
    from poulpy_amd.layouts import MatZnx
    c0 = rcs[0]
    rows, cols_in, ksz, cols, n = c0.key.shape
    a = np.ascontiguousarray(c0.a)
    a_size, res_size = a.shape[1], c0.res_size
    src = Ct(B_ROT, a_size, log_delta, a_size * B_ROT - log_delta, cols)
    dsts = [Ct(B_ROT, res_size, 0, 0, cols) for _ in rcs]
    plan = ckks.plan_rotate_many(dsts, src)
    gals = [c.p % (2 * n) for c in rcs]
    mats = [MatZnx(n, rows, cols_in, cols, ksz, np.ascontiguousarray(k)) for k in keys]
    nbytes = BATCH * res_size * cols * n * 8
    with on_device(hip) as dev:
        d_keys = []
        for m in mats:
            ph = hip.vmp_pmat_alloc(rows, cols_in, cols, ksz)
            hip.vmp_prepare(ph, m)
            d_keys.append(dev.key(ph))
        d_a, d_res = dev.upload(a), dev.alloc(len(rcs) * nbytes)
        tmp = dev.alloc(nbytes) if plan.offset and with_tmp else None
        p = GlweOpParams(rank=1, dnum=rows, dsize=1, key_size=ksz, key_base2k=B_ROT, a_size=res_size if plan.offset else a_size, a_base2k=B_ROT,
                         res_size=res_size, res_base2k=B_ROT, rank_out=1)
        src.data = d_a.ptr
        dsts[0].data = d_res.ptr
        plan.launch(hip, dsts, src, gals, [k.ptr for k in d_keys], p, BATCH, tmp=tmp.ptr if tmp else None)
        hip.sync()
        got = _down(d_res, (len(rcs), BATCH, res_size, cols, n))
    want = np.empty_like(got)
    for r, (c, m) in enumerate(zip(rcs, mats)):
        pr = ref.vmp_pmat_alloc(rows, cols_in, cols, ksz)
        ref.vmp_prepare(pr, m)
        for b in range(BATCH):
            x = VecZnx(n, cols, a_size, np.ascontiguousarray(a[b]))
            if plan.offset:
                sh = VecZnx(n, cols, res_size)
                so.glwe_lsh(ref, B_ROT, plan.offset, sh, x)
                x = sh
            res = VecZnx(n, cols, res_size)
            ref.glwe_automorphism(res, B_ROT, x, B_ROT, pr, 1, B_ROT, gals[r], "automorphism")
            want[r, b] = res.data
    return got, want, dsts, src, plan


def plaintext_of(c, b, p):
    """the plaintext of ciphertext b: phi_p^-1 of what the case says the output decrypts to, as a one-column container's limbs"""
    n = c.want[b].shape[-1]
    return fs.automorphism(c.want[b], fs.galois_inv(p, n))[:, None, :]


def check_meaning(label, c, out_cts, dst, src, fail=False):
    """every output decrypts to phi_p(value of its own plaintext) at the destination's new metadata, stated by tests/ckks_meaning.py on the
    plaintext's limbs, within the key switch's bound (tests/core_cases.py).  The source's own noise (sigma 2^-k_in, moved up by the offset)
    and the rounding at the destination's last limb lie far below that bound at these shapes; the bound is taken as it is."""
    n = out_cts.shape[-1]
    p = c.p % (2 * n)
    have = []
    for b in range(len(out_cts)):
        pt = Ct(B_ROT, src.size, src.log_delta, src.log_budget, 1, plaintext_of(c, b, c.p))
        out = cm.outcome_automorphism(Ct(B_ROT, dst.size, 0, 0, 1), pt, p)
        assert (dst.log_delta, dst.log_budget) == (out.log_delta, out.log_budget), (label, "metadata")
        bits = src.size * B_ROT
        want = fs.torus_from_int(out.want[0] >> (cm.FINE - bits), bits, B_ROT)
        have.append(fs.noise_log2(out_cts[b], B_ROT, c.sk_out, want, B_ROT))
    print(f"[noise] {label}: noise_have {max(have):.2f} (min {min(have):.2f}) noise_want {c.bound:.2f}")
    if fail:
        assert min(have) > c.bound, (label, have, c.bound, "a negative control met the bound")
    else:
        assert max(have) <= c.bound, (label, have, c.bound)


ROT_SHAPES = [(256, 5, 5), (256, 5, 4), (8192, 3, 3), (8192, 3, 2)]


@pytest.mark.parametrize("n,limbs,dst_limbs", ROT_SHAPES, ids=["n256", "n256-smaller-dst", "n8192", "n8192-smaller-dst"])
def test_rotate_into(mods, n, limbs, dst_limbs):
    ref, hip = mods(n)
    rcs = rotation_cases(n, limbs, dst_limbs, [5], seed=n + dst_limbs)
    got, want, dsts, src, plan = rotate(ref, hip, rcs, [rcs[0].key], log_delta=20)
    assert plan.offset == (limbs - dst_limbs) * B_ROT and plan.name == "rotate_into"
    assert np.array_equal(got, want), "device != lsh, then automorphism"
    check_meaning(("rotate_into", n, dst_limbs), rcs[0], got[0], dsts[0], src)


@pytest.mark.parametrize("n,limbs,dst_limbs", [(256, 5, 4), (8192, 3, 3)], ids=["n256-smaller-dst", "n8192"])
def test_rotate_many_two_rotations_and_the_conjugation(mods, n, limbs, dst_limbs):
    ref, hip = mods(n)
    gals = [5, 3, 2 * n - 1]
    rcs = rotation_cases(n, limbs, dst_limbs, gals, seed=7 * n + dst_limbs)
    got, want, dsts, src, plan = rotate(ref, hip, rcs, [c.key for c in rcs], log_delta=20)
    assert plan.name == "rotate_many"
    for r, c in enumerate(rcs):
        assert np.array_equal(got[r], want[r]), ("device != lsh, then automorphism", gals[r])
        check_meaning(("rotate_many", n, gals[r]), c, got[r], dsts[r], src)
    # two keys swapped: still the oracle's digits, and they no longer decrypt
    keys = [rcs[1].key, rcs[0].key, rcs[2].key]
    got, want, dsts, src, _ = rotate(ref, hip, rcs, keys, log_delta=20)
    for r in (0, 1):
        assert np.array_equal(got[r], want[r]), ("device != oracle, swapped keys", gals[r])
        check_meaning(("swapped keys", n, gals[r]), rcs[r], got[r], dsts[r], src, fail=True)
    check_meaning(("untouched conjugation", n), rcs[2], got[2], dsts[2], src)


def test_rotate_into_smaller_destination_refuses_without_a_temporary(mods):
    n = 256
    ref, hip = mods(n)
    rcs = rotation_cases(n, 5, 4, [5], seed=77)
    with pytest.raises(ckks.CKKSError):
        rotate(ref, hip, rcs, [rcs[0].key], log_delta=20, with_tmp=False)
    with pytest.raises(ckks.CKKSError):            # more budget asked of the source than it has
        ckks.plan_rotate_into(Ct(B_ROT, 1, 0, 0), Ct(B_ROT, 5, 50, 10))


# ---- a chain under one secret key ----------------------------------------------------------------------------------------------------------
def test_chain_add_mul_const_sub_rescale_decrypts_to_the_exact_integers(mods):
    """composition.rs::test_linear_sum's shape with a constant product: s = x1 + x2; p = s c; d = p - x3 into a smaller output; rescale d.
    The metadata travels through apply_meta; the phase of the result is compared with the exact value of the messages at the final
    metadata.  Allowed, in ulps of the final destination (2^-dst.max_k): per input 6 sigma 2^-k times its total left shift into the result
    (and, for x1 and x2, times |re| + |im| of the constant, through which they pass), plus every step's rounding allowance
    (tests/ckks_meaning.py) moved up by the shifts that follow it.  Read at a log_budget off by one, the same phase misses that."""
    n = 256
    P = cc.FFT64
    B, K, ld = P.B, P.K, P.ld
    ref, hip = mods(n)
    rng = seeded(2024)
    sk = fs.ternary_secret(n, 1, rng)
    c = Cst(ld, P.lb, cm.encode_cst(5 * (1 << (ld - 3)), B, ld, P.lb), cm.encode_cst(-(1 << (ld - 3)), B, ld, P.lb))     # 0.625 - 0.125 i
    gain = abs(cm.cst_value(c.re, B, ld, P.lb)) + abs(cm.cst_value(c.im, B, ld, P.lb))

    def fresh():
        return Ct(B, P.size, ld, K - ld, 2)
    x = [fresh() for _ in range(3)]
    s, p, d = fresh(), fresh(), Ct(B, -(-(K - ld - B - 1) // B), 0, 0, 2)
    msgs = rng.integers(-(1 << 20), 1 << 20, (3, BATCH, n), dtype=np.int64)
    pts = [[fs.encode(msgs[i, t], B, K, P.size) for t in range(BATCH)] for i in range(3)]          # at effective_k = K
    cts = [np.stack([fs.glwe_encrypt(sk, pts[i][t], B, K, rng) for t in range(BATCH)]) for i in range(3)]
    with on_device(hip) as dev:
        for i in range(3):
            x[i].data = dev.upload(cts[i]).ptr
        d_s, d_p = dev.alloc(cts[0].nbytes), dev.alloc(cts[0].nbytes)
        d_d = dev.alloc(BATCH * d.size * 2 * n * 8)
        s.data, p.data, d.data = d_s.ptr, d_p.ptr, d_d.ptr
        steps = []                                       # (allowance of the step in its destination's ulps, max_k and log_budget there)
        plan = ckks.plan_add_into(s, x[0], x[1])
        plan.launch(hip, s, BATCH, x[0], x[1])
        steps.append((cm.outcome_add(s, _meta(x[0]), _meta(x[1])).allow, cm.max_k(s), s.log_budget))
        before = _meta(s)
        plan = ckks.plan_mul_pt_const_into(p, s, c)
        plan.launch(hip, p, BATCH, s, c)
        steps.append((cm.outcome_mul_cst(p, before, c).allow, cm.max_k(p), p.log_budget))
        before = _meta(p)
        plan = ckks.plan_add_into(d, p, x[2], sub=True)
        plan.launch(hip, d, BATCH, p, x[2])
        steps.append((cm.outcome_add(d, before, _meta(x[2]), sub=True).allow, cm.max_k(d), d.log_budget))
        shift3 = x[2].log_budget - d.log_budget         # x3 enters here
        shift12 = p.log_budget - d.log_budget           # x1, x2 are in p
        k_rs = B + 2
        plan = ckks.plan_rescale_assign(d, k_rs)
        plan.launch(hip, d, BATCH)
        hip.sync()
        got = _down(d_d, (BATCH, d.size, 2, n))
    assert (d.log_delta, d.log_budget) == (ld, K - 2 * ld - (K - ld - cm.max_k(d)) - k_rs)
    noise = fs.BOUND * 2.0 ** (cm.max_k(d) - K) * (2 * gain * 2.0 ** (shift12 + k_rs) + 2.0 ** (shift3 + k_rs))
    rounding = sum(a * 2.0 ** (cm.max_k(d) - mk + b - d.log_budget) for a, mk, b in steps)
    allowed = noise + rounding
    for t in range(BATCH):
        m = [Ct(B, P.size, ld, K - ld, 1, pts[i][t][:, None, :]) for i in range(3)]
        v = cm.vsum(cm.vtimes(cm.vsum(cm.value_ct(m[0]), cm.value_ct(m[1])), c, B), cm.value_ct(m[2]), -1)
        phase = fs.glwe_phase(got[t], sk)[:, None, :]
        dev_ulps = cm.deviation_ulps(phase, cm.place(v, d.log_budget), d.size, B)
        print(f"[chain] ciphertext {t}: deviation {dev_ulps:.3e} ulps, allowed {allowed:.3e} (noise {noise:.3e}, rounding {rounding:.3e})")
        assert dev_ulps <= allowed
        for wrong in (d.log_budget - 1, d.log_budget + 1):
            assert cm.deviation_ulps(phase, cm.place(v, wrong), d.size, B) > 256 * allowed, ("read at log_budget", wrong)


def _meta(ct):
    """the container with its metadata as it is now and one item of zeros for data: the allowance needs no more"""
    return Ct(ct.base2k, ct.size, ct.log_delta, ct.log_budget, ct.cols, np.zeros((ct.size, ct.cols, 1), dtype=np.int64))
