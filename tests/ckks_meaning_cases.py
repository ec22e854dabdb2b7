"""poulpy-ckks's own test cases (src/leveled/tests/test_suite/*.rs) for the operations this project runs on the device, restated on
coefficients: tests/test_ckks_meaning_host.py runs them through the host restatements, tests/test_gpu_ckks_meaning.py through the launches
of poulpy_amd/ckks.py, and both compare with the exact statement of tests/ckks_meaning.py.

A case is a small program over named containers: env = {name: Ct | Pt} (layout and metadata, as TestContext::encrypt(k, prec) and
alloc_ct(k) make them: ceil(k / base2k) limbs, log_budget = k - log_delta) and steps = [dict(op=, dst=, a=, b=, pt=, ops=, csts=, bits=, k=,
norm=)].  Most have one step; add_many, align and composition.rs::test_linear_sum have several, and every step is checked on its own, against
the meaning of the limbs it actually read.  `refuse` names the error the reference returns instead (ckks_meaning.Refused.kind).

Parameter sets: the reference's FFT64 one (test_suite/mod.rs:80-90: base2k 19, k = 152, log_delta 30, a plaintext log_budget of 10), the
same at base2k 12 with 6 limbs, and the first once more at rank 2.  Limbs are uniform digits (no key is involved, and uniform limbs leave no
bit of a result unchecked); constants are drawn with |v| < 2^(min_k - 1)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from poulpy_amd import ckks
from poulpy_amd.ckks import Cst, Ct, Pt
from poulpy_amd.layouts import VecZnx
from tests import ckks_lincomb_oracle as lo
from tests import ckks_meaning as cm
from tests import fhe_sk as fs
from tests import plain_oracle as po
from tests import shift_oracle as so

DELTA_LOG_DELTA = 12                     # add.rs:53


def params(base2k=19, size=8, rank=1, log_delta=30, log_budget=10):
    return SimpleNamespace(B=base2k, size=size, K=base2k * size, rank=rank, cols=rank + 1, ld=log_delta, lb=log_budget,
                           tag=f"b{base2k}x{size}r{rank}")


FFT64 = params()
SETS = [FFT64, params(12, 6), params(19, 8, rank=2)]
SMALL3 = params(19, 3, log_delta=12, log_budget=6)       # three limbs, for the larger rings of the device tests


def constant(P, rng, form, log_delta=None):
    """a CKKSPlaintextCstZnx at the set's precision: re / im digits of values v drawn with |v| < 2^(min_k - 1), either sign"""
    ld = P.ld if log_delta is None else log_delta
    k = cm.cst_k(P.B, ld, P.lb)
    assert k - 1 <= 62

    def draw():
        x = int(rng.integers(0, 1 << (k - 1)))
        return cm.encode_cst(-x if rng.integers(2) else x, P.B, ld, P.lb)
    return Cst(ld, P.lb, draw() if form in ("re", "both") else None, draw() if form in ("im", "both") else None)


def cases(P, seed=0):
    B, K, ld = P.B, P.K, P.ld
    rng = np.random.default_rng(seed + 1000 * B + P.rank)
    low = ld - DELTA_LOG_DELTA

    def ct(k, log_delta=ld):
        return Ct(B, -(-k // B), log_delta, k - log_delta, P.cols)

    def pt(log_delta=ld, base2k=B):
        return Pt(base2k, -(-(log_delta + P.lb) // base2k), log_delta)

    def cst(form, log_delta=None):
        return constant(P, rng, form, log_delta)

    out = []

    def case(name, env, *steps, refuse=None, whole=None):
        out.append(SimpleNamespace(name=name, env=env, steps=[dict(s) for s in steps], refuse=refuse, whole=whole, P=P))

    full, small = ct(K), ct(K - B - 1)
    for tag, sub in (("add", False), ("sub", True)):
        o = tag + "_into"
        # add.rs / sub.rs: ct with ct
        case(f"test_{tag}_ct_aligned", dict(d=ct(K), a=full, b=full), dict(op=o, dst="d", a="a", b="b"))
        case(f"test_{tag}_ct_delta_a_lt_b", dict(d=ct(K), a=ct(K - B + 1), b=full), dict(op=o, dst="d", a="a", b="b"))
        case(f"test_{tag}_ct_delta_a_gt_b", dict(d=ct(K), a=full, b=ct(K - B + 1)), dict(op=o, dst="d", a="a", b="b"))
        case(f"test_{tag}_ct_delta_log_delta", dict(d=ct(K), a=full, b=ct(K - DELTA_LOG_DELTA, low)), dict(op=o, dst="d", a="a", b="b"))
        case(f"test_{tag}_ct_smaller_output", dict(d=small, a=full, b=full), dict(op=o, dst="d", a="a", b="b"))
        case(f"test_{tag}_ct_assign_aligned", dict(d=ct(K), a=full), dict(op=tag + "_assign", dst="d", a="a"))
        case(f"test_{tag}_ct_assign_self_lt", dict(d=ct(K - B - 1), a=full), dict(op=tag + "_assign", dst="d", a="a"))
        case(f"test_{tag}_ct_assign_self_gt", dict(d=ct(K), a=ct(K - B - 1)), dict(op=tag + "_assign", dst="d", a="a"))
        # ct with a plaintext vector
        case(f"test_{tag}_pt_vec_znx_assign", dict(d=ct(K), pt=pt()), dict(op=tag + "_pt_assign", dst="d", pt="pt"))
        case(f"test_{tag}_pt_vec_znx_into_aligned", dict(d=ct(K), a=full, pt=pt()), dict(op=tag + "_pt_into", dst="d", a="a", pt="pt"))
        case(f"test_{tag}_pt_vec_znx_into_delta_log_delta", dict(d=ct(K), a=full, pt=pt(low)), dict(op=tag + "_pt_into", dst="d", a="a", pt="pt"))
        case(f"test_{tag}_pt_vec_znx_into_smaller_output", dict(d=small, a=full, pt=pt()), dict(op=tag + "_pt_into", dst="d", a="a", pt="pt"))
        case(f"test_{tag}_pt_vec_znx_base2k_mismatch_error", dict(d=ct(K), pt=pt(base2k=B // 2)), dict(op=tag + "_pt_assign", dst="d", pt="pt"),
             refuse=cm.BASE2K)
        # add_unsafe.rs / sub_unsafe.rs: no closing normalization
        case(f"test_{tag}_ct_aligned_unsafe", dict(d=ct(K), a=full, b=full), dict(op=o, dst="d", a="a", b="b", norm=False))
        case(f"test_{tag}_ct_delta_a_lt_b_unsafe", dict(d=ct(K), a=ct(K - B + 1), b=full), dict(op=o, dst="d", a="a", b="b", norm=False))
        case(f"test_{tag}_ct_assign_aligned_unsafe", dict(d=ct(K), a=full), dict(op=tag + "_assign", dst="d", a="a", norm=False))
        case(f"test_{tag}_ct_assign_self_gt_unsafe", dict(d=ct(K), a=ct(K - B - 1)), dict(op=tag + "_assign", dst="d", a="a", norm=False))
        case(f"test_{tag}_pt_vec_znx_into_aligned_unsafe", dict(d=ct(K), a=full, pt=pt()),
             dict(op=tag + "_pt_into", dst="d", a="a", pt="pt", norm=False))
        # what the reference's list lacks: shifts by more than a limb and of at least max_k, a plaintext shift across a limb, refusals
        case(f"{tag}_ct_shift_more_than_one_limb", dict(d=ct(K), a=ct(K - 2 * B - 3), b=full), dict(op=o, dst="d", a="a", b="b"))
        case(f"{tag}_ct_assign_shift_of_max_k", dict(d=ct(K - 2 * B - 1), a=Ct(B, 2, ld, K - ld, P.cols)), dict(op=tag + "_assign", dst="d", a="a"))
        case(f"{tag}_pt_rsh_crosses_a_limb", dict(d=ct(K), a=ct(K - 5), pt=pt(low)), dict(op=tag + "_pt_into", dst="d", a="a", pt="pt"))
        # operands whose own max_k lies above their effective_k: the squeeze into a smaller dst drops bits, and the result is rounded
        case(f"{tag}_ct_smaller_output_rounds", dict(d=small, a=ct(K - 5), b=ct(K - 3)), dict(op=o, dst="d", a="a", b="b"))
        case(f"{tag}_ct_smaller_output_rounds_unsafe", dict(d=small, a=ct(K - 3), b=ct(K - 5)), dict(op=o, dst="d", a="a", b="b", norm=False))
        case(f"{tag}_pt_finer_than_ct_rounds", dict(d=ct(K), a=full, pt=pt(ld + 7)), dict(op=tag + "_pt_into", dst="d", a="a", pt="pt"))
        case(f"{tag}_pt_assign_finer_than_ct_rounds", dict(d=ct(K), pt=pt(ld + 7)), dict(op=tag + "_pt_assign", dst="d", pt="pt"))
        case(f"{tag}_ct_output_smaller_than_budget_error", dict(d=ct(B), a=Ct(B, P.size, K - 3, 3, P.cols), b=Ct(B, P.size, K - 3, 3, P.cols)),
             dict(op=o, dst="d", a="a", b="b"), refuse=cm.CAPACITY)
        case(f"{tag}_pt_alignment_error", dict(d=Ct(B, P.size, ld, 1, P.cols), pt=Pt(B, 4, ld)), dict(op=tag + "_pt_assign", dst="d", pt="pt"),
             refuse=cm.ALIGNMENT)

    # neg.rs
    case("test_neg_aligned", dict(d=ct(K), a=full), dict(op="neg_into", dst="d", a="a"))
    case("test_neg_smaller_output", dict(d=small, a=full), dict(op="neg_into", dst="d", a="a"))
    case("test_neg_assign", dict(d=ct(K)), dict(op="neg_assign", dst="d"))
    # mul_pow2.rs
    bits = 7
    case("test_mul_pow2_aligned", dict(d=ct(K), a=full), dict(op="mul_pow2_into", dst="d", a="a", bits=bits))
    case("test_mul_pow2_smaller_output", dict(d=small, a=full), dict(op="mul_pow2_into", dst="d", a="a", bits=bits))
    case("test_mul_pow2_assign", dict(d=ct(K)), dict(op="mul_pow2_assign", dst="d", bits=bits))
    case("test_div_pow2_aligned", dict(d=ct(K), a=full), dict(op="div_pow2_into", dst="d", a="a", bits=bits))
    case("test_div_pow2_smaller_output", dict(d=small, a=full), dict(op="div_pow2_into", dst="d", a="a", bits=bits))
    case("test_div_pow2_assign", dict(d=ct(K)), dict(op="div_pow2_assign", dst="d", bits=bits))
    case("test_div_pow2_assign_explicit_error", dict(d=ct(K)), dict(op="div_pow2_assign", dst="d", bits=K - ld + 1), refuse=cm.CAPACITY)
    case("mul_pow2_more_than_one_limb", dict(d=ct(K)), dict(op="mul_pow2_assign", dst="d", bits=2 * B + 3))
    case("mul_pow2_of_max_k", dict(d=ct(K), a=full), dict(op="mul_pow2_into", dst="d", a="a", bits=K))
    # rescale.rs (the reference tests it through the compositions)
    case("rescale_into", dict(d=ct(K), a=full), dict(op="rescale_into", dst="d", a="a", k=B + 1))
    case("rescale_into_smaller_output", dict(d=small, a=full), dict(op="rescale_into", dst="d", a="a", k=2 * B))
    case("rescale_assign_two_limbs", dict(d=ct(K)), dict(op="rescale_assign", dst="d", k=2 * B))
    case("rescale_assign_error", dict(d=ct(K)), dict(op="rescale_assign", dst="d", k=K - ld + 1), refuse=cm.CAPACITY)
    case("neg_smaller_output_rounds", dict(d=small, a=ct(K - 5)), dict(op="neg_into", dst="d", a="a"))
    case("mul_pow2_smaller_output_rounds", dict(d=small, a=ct(K - 5)), dict(op="mul_pow2_into", dst="d", a="a", bits=3))
    case("div_pow2_smaller_output_rounds", dict(d=small, a=ct(K - 5)), dict(op="div_pow2_into", dst="d", a="a", bits=3))
    case("rescale_into_smaller_output_rounds", dict(d=small, a=ct(K - 5)), dict(op="rescale_into", dst="d", a="a", k=3))
    case("align_assign_a_lt_b", dict(a=ct(K - 7), b=full), dict(op="align_assign", a="a", b="b"))
    case("align_assign_a_gt_b", dict(a=full, b=ct(K - B - 2)), dict(op="align_assign", a="a", b="b"))
    # add_many.rs
    for name, ks, d in (("test_add_many_aligned", [K] * 4, ct(K)), ("test_add_many_single_smaller_output", [K], small),
                        ("test_add_many_unaligned_log_budget", [K, K - B + 1, K, K], ct(K)), ("test_add_many_smaller_output", [K] * 4, small)):
        env = dict(d=d, **{f"a{i}": ct(k) for i, k in enumerate(ks)})
        case(name, env, *add_many_steps(len(ks)), whole=("add_many", [f"a{i}" for i in range(len(ks))]))
    env = dict(d=small, a0=ct(K - 5), a1=ct(K - 3), a2=ct(K - 5))
    case("add_many_smaller_output_rounds", env, *add_many_steps(3), whole=("add_many", ["a0", "a1", "a2"]))
    env = dict(d=ct(K), a0=ct(K - DELTA_LOG_DELTA, low), a1=full, a2=full, a3=full)
    case("test_add_many_delta_log_delta", env, *add_many_steps(4), whole=("add_many", ["a0", "a1", "a2", "a3"]))
    # mul.rs: the products by constants
    case("test_mul_pt_const_znx_into_aligned", dict(d=ct(K), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("both")]))
    case("test_mul_pt_const_assign", dict(d=ct(K)), dict(op="mul_cst_assign", dst="d", csts=[cst("both")]))
    case("test_mul_pt_const_rnx_into_delta_log_delta", dict(d=ct(K), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("both", low)]))
    case("test_mul_pt_const_rnx_into_real_only", dict(d=ct(K), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("re")]))
    case("mul_pt_const_into_im_only", dict(d=ct(K), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("im")]))
    case("mul_pt_const_assign_im_only", dict(d=ct(K)), dict(op="mul_cst_assign", dst="d", csts=[cst("im")]))
    case("mul_pt_const_assign_real_only", dict(d=ct(K)), dict(op="mul_cst_assign", dst="d", csts=[cst("re")]))
    case("mul_pt_const_into_smaller_output", dict(d=ct(K - ld - B - 1), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("both")]))
    case("mul_pt_const_real_into_smaller_output", dict(d=ct(K - ld - B - 1), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("re")]))
    case("mul_pt_const_into_zero", dict(d=ct(K), a=full), dict(op="mul_cst_into", dst="d", a="a", csts=[cst("none")]))
    case("mul_pt_const_precision_underflow_error", dict(d=ct(K), a=Ct(B, P.size, ld, ld - 1, P.cols)),
         dict(op="mul_cst_into", dst="d", a="a", csts=[cst("re")]), refuse=cm.UNDERFLOW)
    # mul_add.rs / mul_sub.rs: the forms by constants
    for tag, ref_name in (("add", "test_mul_add_const_znx"), ("sub", "test_mul_sub_pt_const_znx")):
        o = f"mul_{tag}_cst"
        case(f"{ref_name}_into_aligned", dict(d=ct(K), a=full), dict(op=o, dst="d", a="a", csts=[cst("both")]))
        case(f"{ref_name}_zero_preserves_dst_meta", dict(d=ct(K), a=full), dict(op=o, dst="d", a="a", csts=[cst("none", low)]))
        case(f"mul_{tag}_const_dst_at_the_product_budget", dict(d=ct(K - ld), a=full), dict(op=o, dst="d", a="a", csts=[cst("re")]))
        c = cst("im")
        low_dst = Ct(B, -(-(K - ld) // B) - 1, ld, 0, P.cols)        # one limb less than the product needs: squeezed, then 5 bits above dst
        low_dst.log_budget = cm.meta_mul_pt(low_dst, full, c)[1] - 5
        case(f"mul_{tag}_const_dst_below_the_product_budget", dict(d=low_dst, a=full), dict(op=o, dst="d", a="a", csts=[c]))
    # dot_product.rs: the form by constants
    three = {"a0": full, "a1": full, "a2": full}
    case("test_dot_product_const_znx_aligned", dict(d=ct(K), **three),
         dict(op="dot_cst", dst="d", ops=["a0", "a1", "a2"], csts=[cst("both"), cst("both"), cst("both")]))
    case("dot_product_const_unaligned", dict(d=ct(K), a0=full, a1=ct(K - B + 1), a2=ct(K - 3)),
         dict(op="dot_cst", dst="d", ops=["a0", "a1", "a2"], csts=[cst("both"), cst("re"), cst("im")]))
    case("dot_product_const_unaligned_b", dict(d=ct(K), a0=ct(K - (2 * B + 1 if K - 2 * ld >= 2 * B + 1 else 8)), a1=full, a2=full),
         dict(op="dot_cst", dst="d", ops=["a0", "a1", "a2"], csts=[cst("im"), cst("both", low), cst("none")]))
    case("dot_product_const_smaller_output", dict(d=ct(K - ld - B - 1), **three),
         dict(op="dot_cst", dst="d", ops=["a0", "a1", "a2"], csts=[cst("re"), cst("both"), cst("im")]))
    case("dot_product_const_length_mismatch_error", dict(d=ct(K), a0=full, a1=full),
         dict(op="dot_cst", dst="d", ops=["a0", "a1"], csts=[cst("re")]), refuse=cm.LENGTHS)
    # composition.rs::test_linear_sum: two scaled copies of one ciphertext, the terms allocated at x.log_budget, then ckks_add_assign
    c1, c2 = cst("both"), cst("both")
    case("test_linear_sum", dict(x=full, t1=ct(K - ld), t2=ct(K - ld)), dict(op="mul_cst_into", dst="t1", a="x", csts=[c1]),
         dict(op="mul_cst_into", dst="t2", a="x", csts=[c2]), dict(op="add_assign", dst="t1", a="t2"), whole=("dot", ["x", "x"], [c1, c2]))
    return out


def add_many_steps(n):
    """composite.rs:63-93"""
    if n == 1:
        return [dict(op="mul_pow2_into", dst="d", a="a0", bits=0)]
    steps = [dict(op="add_into", dst="d", a="a0", b="a1", norm=n == 2)]
    return steps + [dict(op="add_assign", dst="d", a=f"a{i}", norm=i == n - 1) for i in range(2, n)]


def all_cases():
    return [c for P in SETS + [SMALL3] for c in cases(P)]


def ids(cs):
    return [f"{c.P.tag}-{c.name}" for c in cs]


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def draw(case, rng, n):
    """{name: (size, cols | 1, n) uniform digits} for every container of the case"""
    return {name: fs.uniform_digits((o.size, 1 if isinstance(o, Pt) else o.cols, n), o.base2k, rng) for name, o in case.env.items()}


def host_env(case, data, n):
    """fresh containers with VecZnx copies of `data`"""
    env = {}
    for name, o in case.env.items():
        arr = data[name].copy()
        env[name] = type(o)(**{**o.__dict__, "data": VecZnx(n, arr.shape[1], o.size, arr)})
    return env


# ---- one step: its plan, its meaning, its host restatement -----------------------------------------------------------------------------------
def step_plan(st, env):
    """the plan poulpy_amd/ckks.py makes of the step (raises ckks.CKKSError where it refuses)"""
    op = st["op"]
    g = env.get
    d, a, b, p = g(st.get("dst")), g(st.get("a")), g(st.get("b")), g(st.get("pt"))
    norm = st.get("norm", True)
    if op in ("add_into", "sub_into"):
        return ckks.plan_add_into(d, a, b, op == "sub_into", norm)
    if op in ("add_assign", "sub_assign"):
        return ckks.plan_add_assign(d, a, op == "sub_assign", norm)
    if op in ("add_pt_into", "sub_pt_into"):
        return ckks.plan_add_pt_into(d, a, p, op == "sub_pt_into", norm)
    if op in ("add_pt_assign", "sub_pt_assign"):
        return ckks.plan_add_pt_assign(d, p, op == "sub_pt_assign", norm)
    if op == "neg_into":
        return ckks.plan_neg_into(d, a)
    if op == "neg_assign":
        return ckks.plan_neg_assign(d)
    if op in ("mul_pow2_into", "div_pow2_into"):
        return getattr(ckks, "plan_" + op)(d, a, st["bits"])
    if op in ("mul_pow2_assign", "div_pow2_assign"):
        return getattr(ckks, "plan_" + op)(d, st["bits"])
    if op == "rescale_into":
        return ckks.plan_rescale_into(d, a, st["k"])
    if op == "rescale_assign":
        return ckks.plan_rescale_assign(d, st["k"])
    if op == "align_assign":
        which, plan = ckks.plan_align_assign(a, b)
        st["dst"] = st[which]
        return plan
    if op == "mul_cst_into":
        return ckks.plan_mul_pt_const_into(d, a, st["csts"][0])
    if op == "mul_cst_assign":
        return ckks.plan_mul_pt_const_assign(d, st["csts"][0])
    if op in ("mul_add_cst", "mul_sub_cst"):
        return ckks.plan_mul_add_pt_const(d, a, st["csts"][0], sub=op == "mul_sub_cst")
    if op == "dot_cst":
        return ckks.plan_dot_product_pt_const(d, [env[k] for k in st["ops"]], st["csts"])
    raise ValueError(op)


def step_outcome(st, env) -> cm.Outcome:
    """what the step must compute from the limbs now in env, and the name of the container it writes (raises cm.Refused)"""
    op = st["op"]
    g = env.get
    d, a, b, p = g(st.get("dst")), g(st.get("a")), g(st.get("b")), g(st.get("pt"))
    if op in ("add_into", "sub_into"):
        return cm.outcome_add(d, a, b, op == "sub_into")
    if op in ("add_assign", "sub_assign"):
        return cm.outcome_add_assign(d, a, op == "sub_assign")
    if op in ("add_pt_into", "sub_pt_into", "add_pt_assign", "sub_pt_assign"):
        return cm.outcome_add_pt(d, a, p, op.startswith("sub"))
    if op in ("neg_into", "neg_assign"):
        return cm.outcome_neg(d, a)
    if op in ("mul_pow2_into", "mul_pow2_assign"):
        return cm.outcome_mul_pow2(d, a, st["bits"])
    if op in ("div_pow2_into", "div_pow2_assign"):
        return cm.outcome_div_pow2(d, a, st["bits"])
    if op in ("rescale_into", "rescale_assign"):
        return cm.outcome_rescale(d, a, st["k"])
    if op == "align_assign":
        which, k = cm.align(a, b)
        st["dst"] = st[which]
        return cm.outcome_rescale(env[st[which]], None, k)
    if op in ("mul_cst_into", "mul_cst_assign"):
        return cm.outcome_mul_cst(d, a, st["csts"][0])
    if op in ("mul_add_cst", "mul_sub_cst"):
        return cm.outcome_mul_add_cst(d, a, st["csts"][0], op == "mul_sub_cst")
    if op == "dot_cst":
        if len(st["ops"]) != len(st["csts"]):
            raise cm.Refused(cm.LENGTHS)
        return cm.outcome_dot_cst(d, [env[k] for k in st["ops"]], st["csts"])
    raise ValueError(op)


def whole_outcome(case, env0) -> cm.Outcome:
    """the meaning of a several-step case as one operation on its first inputs"""
    kind, names, *rest = case.whole
    d = env0[case.steps[-1]["dst"]]
    if kind == "add_many":
        return cm.outcome_add_many(env0["d"], [env0[k] for k in names])
    return cm.outcome_dot_cst(d, [env0[k] for k in names], rest[0])


def step_host(ref, st, plan, env):
    """the step on the host restatements (tests/shift_oracle.py, plain_oracle.py, ckks_lincomb_oracle.py); writes env[st["dst"]]"""
    op = st["op"]
    g = env.get
    d, a, b, p = g(st.get("dst")), g(st.get("a")), g(st.get("b")), g(st.get("pt"))
    if isinstance(plan, ckks.Plan):
        so.run(ref, plan, d, a if op != "align_assign" else None, b if op != "align_assign" else None, p)
        plan.apply_meta(d)
    elif op == "mul_cst_into":
        c = st["csts"][0]
        po.ckks_mul_pt_const_into(ref, plan.cnv_offset, d.data, d.base2k, a.data, a.base2k, c.re, c.im)
        plan.apply_meta(d)
    elif op == "mul_cst_assign":
        c = st["csts"][0]
        po.ckks_mul_pt_const_assign(ref, plan.cnv_offset, d.data, d.base2k, c.re, c.im)
        plan.apply_meta(d)
    elif op in ("mul_add_cst", "mul_sub_cst", "dot_cst"):           # the plan's own term list, not the restatement's second derivation of it
        lo.run_plan(ref, plan, d, [env[k] for k in st["ops"]] if op == "dot_cst" else [a], st["csts"])
    else:
        raise ValueError(op)
