"""The host restatements of the CKKS operations (tests/shift_oracle.py, plain_oracle.py, ckks_lincomb_oracle.py), driven by the plans of
poulpy_amd/ckks.py, against what the operations MEAN (tests/ckks_meaning.py: exact integers, written from poulpy-ckks's layouts and test
helpers), on the reference's own cases (tests/ckks_meaning_cases.py), N = 16.

Per case and step: (a) the metadata the plan reports equals the independent statement; (b) the result lies within the allowance, computed
from metadata alone (ckks_meaning's docstring); (c) one wrong amount each - an LSH by one bit, a sign, the two budget branches, cnv_offset,
pt_shift, re for im, the reported log_budget - misses the allowance by at least 2^8; (d) plan_* raises CKKSError exactly where the
statement says the reference refuses.

Largest deviation of the restatements, in ulps of 2^-dst.max_k, over every case and parameter set (test_table_of_deviations prints it):

    family                                    worst      allowance there
    add / sub, nothing below dst              0          0
    add / sub, rounded into dst               0.9688     1.0002      two streams
    add_many (the whole sum)                  1.2812     1.5000      three streams
    neg / pow2 / rescale, nothing below dst   0          0
    neg / pow2 / rescale, rounded into dst    0.5000     0.5000
    add_pt / sub_pt                           0.5000     0.5000      the plaintext finer than the ciphertext; 0 otherwise
    mul_pt_const, no part (zero)              0          0
    mul_pt_const, one part                    0.4988     0.5000
    mul_pt_const, two parts                   0.9476     1.0000
    mul_add / mul_sub by a constant           15.9375    16.0000     one part, the product 5 bits above dst's budget: 0.5 x 2^5
    dot_product by constants                  1.3959     2.0005      sum_i parts_i 0.5 2^(b_i - b_out)

Most of the reference's cases shift by whole limbs into a destination that holds every bit: there the result is exact, and the test asks
for exactly that (allowance 0).  The cases named *_rounds squeeze operands whose max_k lies above their effective_k.
"""
import copy

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH, RAW, Cst
from poulpy_amd.layouts import VecZnx
from tests import ckks_meaning as cm
from tests import ckks_meaning_cases as cc
from tests import shift_oracle as so
from tests.helpers import seeded

N = 16
CASES = cc.all_cases()
GOOD = [c for c in CASES if c.refuse is None]
MISS = 256.0            # a negative control misses the allowance by this factor at least


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def family(st, out):
    op = st["op"]
    if op in ("mul_cst_into", "mul_cst_assign"):
        return "mul_pt_const, %d part(s)" % cm.parts(st["csts"][0])
    if op in ("mul_add_cst", "mul_sub_cst"):
        return "mul_add / mul_sub by a constant"
    if op == "dot_cst":
        return "dot_product by constants"
    if "pt" in op:
        return "add_pt / sub_pt"
    kind = "add / sub" if op[:3] in ("add", "sub") else "neg / pow2 / rescale"
    return kind + (", rounded into dst" if out.allow else ", nothing below dst")


def run(ref, case, seed=0, worst=None):
    """every step of the case on the restatements -> [(step, deviation, outcome, metadata reported)], and the whole-case check"""
    data = cc.draw(case, seeded(seed), N)
    env = cc.host_env(case, data, N)
    env0 = cc.host_env(case, data, N)
    rows = []
    for st in case.steps:
        out = cc.step_outcome(st, env)
        plan = cc.step_plan(st, env)
        cc.step_host(ref, st, plan, env)
        d = env[st["dst"]]
        dev = cm.deviation_ulps(d, out.want, d.size, d.base2k)
        rows.append((st, dev, out, (d.log_delta, d.log_budget)))
        if worst is not None:
            f = family(st, out)
            if dev > worst.get(f, (-1.0, 0.0))[0]:
                worst[f] = (dev, out.allow)
    if case.whole:
        out = cc.whole_outcome(case, env0)
        d = env[case.steps[-1]["dst"]]
        dev = cm.deviation_ulps(d, out.want, d.size, d.base2k)
        rows.append((dict(op="whole:" + case.whole[0]), dev, out, (d.log_delta, d.log_budget)))
        if worst is not None and case.whole[0] == "add_many":
            worst["add_many"] = max(worst.get("add_many", (-1.0, 0.0)), (dev, out.allow))
    return rows


@pytest.mark.parametrize("case", GOOD, ids=cc.ids(GOOD))
def test_metadata_and_deviation(ref, case):
    for st, dev, out, meta in run(ref, case, seed=len(case.name)):
        assert meta == (out.log_delta, out.log_budget), (st["op"], "metadata", meta, (out.log_delta, out.log_budget))
        assert dev <= out.allow, (st["op"], "deviation", dev, "allowance", out.allow)


def test_allowance_stays_within_twice_the_plain_count_plus_one():
    """HALF(B) per rounding instead of 0.5: the one addition to the issue's formula, far inside 2 x formula + 1"""
    for B in (12, 19):
        assert 0.5 <= cm.HALF(B) <= 0.5 * (1 + 2.0 ** -(B - 1))


def test_table_of_deviations(ref):
    worst = {}
    for case in GOOD:
        run(ref, case, seed=7, worst=worst)
    for f in sorted(worst):
        print(f"[deviation] {f:45s} worst {worst[f][0]:10.4f}   allowance there {worst[f][1]:10.4f}")
    assert all(dev <= allow for dev, allow in worst.values())
    exact = [f for f in worst if f.endswith("nothing below dst")]
    assert exact and all(worst[f][0] == 0 for f in exact)


def test_expectation_is_not_the_restatement(ref):
    """the statement imports neither a restatement nor a plan"""
    code = open(cm.__file__).read().split("from __future__", 1)[1].replace("_offset_unary(", "").replace("_offset_binary(", "")
    for word in ("shift_oracle", "ckks_lincomb_oracle", "plain_oracle", "plan_", "get_mul_const_params", "offset_unary(", "offset_binary(", " min_k("):
        assert word not in code, word
    assert "from poulpy_amd.ckks import Cst, Ct, Pt" in code and code.count("poulpy_amd") == 1


# ---- (d) refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=cc.ids(CASES))
def test_plans_refuse_exactly_where_the_reference_does(case):
    data = cc.draw(case, seeded(1), N)
    env = cc.host_env(case, data, N)
    st = case.steps[0]
    try:
        cc.step_outcome(st, env)
        said = None
    except cm.Refused as e:
        said = e.kind
    assert said == case.refuse
    if said is None:
        cc.step_plan(st, env)
    else:
        with pytest.raises(ckks.CKKSError):
            cc.step_plan(st, env)


# ---- (c) negative controls ---------------------------------------------------------------------------------------------------------------
def walk(ref, plan, d, a=None, b=None, pt=None):
    """plan.terms applied in order to a zero GLWE on the restatement's shifts, then the closing normalization: what a changed term does"""
    ops = {"dst": d, "a": a, "b": b, "pt": pt}
    src = {k: o.data.copy() for k, o in ops.items() if o is not None}
    res = VecZnx(N, d.cols, d.size)
    for t in plan.terms:
        x = src[t.src]
        for i in ((0,) if t.src == "pt" else range(d.cols)):
            if t.kind == RAW:
                m = min(res.size, x.size)
                res.data[:m, i] += t.sign * x.data[:m, i]
            elif t.kind == LSH:
                so.vec_znx_lsh_acc(d.base2k, t.k, res, i, x, i, sub=t.sign < 0)
            else:
                so.vec_znx_rsh_acc(d.base2k, t.k, res, i, x, 0, sub=t.sign < 0)
    if plan.normalize:
        so.glwe_normalize_assign(ref, d.base2k, res)
    d.data.data[...] = res.data


def one(name):
    return next(c for c in cc.cases(cc.FFT64) if c.name == name)


def setup(case, seed=3):
    data = cc.draw(case, seeded(seed), N)
    env = cc.host_env(case, data, N)
    st = case.steps[0]
    return env, st, cc.step_outcome(st, env), cc.step_plan(st, env)


def dev_of(env, st, want):
    d = env[st["dst"]]
    return cm.deviation_ulps(d, want, d.size, d.base2k)


def misses(dev, out):
    return dev >= MISS * max(out.allow, cm.HALF(19))


def operands(env, st):
    return env[st["dst"]], env.get(st.get("a")), env.get(st.get("b")), env.get(st.get("pt"))


@pytest.mark.parametrize("name", ["test_add_ct_delta_a_lt_b", "test_sub_ct_delta_a_gt_b", "test_add_ct_smaller_output", "test_add_pt_vec_znx_into_aligned",
                                  "test_sub_pt_vec_znx_into_smaller_output", "test_neg_smaller_output", "test_mul_pow2_aligned"])
def test_walk_of_the_terms_is_the_restatement(ref, name):
    env, st, out, plan = setup(one(name))
    env2 = copy.deepcopy(env)
    cc.step_host(ref, st, plan, env)
    walk(ref, plan, *operands(env2, st))
    assert np.array_equal(env[st["dst"]].data.data, env2[st["dst"]].data.data)


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("name,term", [("test_add_ct_delta_a_lt_b", 1), ("test_sub_ct_delta_a_gt_b", 0), ("test_add_ct_smaller_output", 0),
                                       ("test_add_ct_smaller_output", 1), ("test_mul_pow2_aligned", 0), ("test_neg_smaller_output", 0)])
def test_control_one_lsh_amount_off_by_one(ref, name, term, delta):
    env, st, out, plan = setup(one(name))
    assert plan.terms[term].kind == LSH
    plan.terms[term].k += delta
    walk(ref, plan, *operands(env, st))
    assert misses(dev_of(env, st, out.want), out)


@pytest.mark.parametrize("name", ["test_add_ct_aligned", "test_sub_ct_aligned", "test_sub_ct_delta_a_lt_b", "test_add_pt_vec_znx_into_aligned",
                                  "test_neg_aligned"])
def test_control_one_sign_flipped(ref, name):
    env, st, out, plan = setup(one(name))
    plan.terms[-1].sign = -plan.terms[-1].sign
    walk(ref, plan, *operands(env, st))
    assert misses(dev_of(env, st, out.want), out)


@pytest.mark.parametrize("name", ["test_add_ct_delta_a_lt_b", "test_add_ct_delta_a_gt_b", "test_sub_ct_delta_a_lt_b", "test_add_ct_assign_self_lt",
                                  "test_sub_ct_assign_self_gt"])
def test_control_budget_branches_swapped(ref, name):
    """the plan of the same operands with their two log_budgets exchanged, run on the true data"""
    env, st, out, _ = setup(one(name))
    x, y = env[st["dst"] if "assign" in st["op"] else st["a"]], env[st["a"] if "assign" in st["op"] else st["b"]]
    x.log_budget, y.log_budget = y.log_budget, x.log_budget
    plan = cc.step_plan(st, env)
    cc.step_host(ref, st, plan, env)
    assert misses(dev_of(env, st, out.want), out)


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("name", ["test_mul_pt_const_znx_into_aligned", "test_mul_pt_const_rnx_into_real_only", "test_mul_pt_const_assign"])
def test_control_cnv_offset_off_by_one(ref, name, delta):
    env, st, out, plan = setup(one(name))
    plan.cnv_offset += delta
    cc.step_host(ref, st, plan, env)
    assert misses(dev_of(env, st, out.want), out)


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("name", ["test_add_pt_vec_znx_into_aligned", "test_sub_pt_vec_znx_assign", "test_add_pt_vec_znx_into_delta_log_delta"])
def test_control_pt_shift_off_by_one(ref, name, delta):
    env, st, out, plan = setup(one(name))
    plan.terms[-1].k += delta
    walk(ref, plan, *operands(env, st))
    assert misses(dev_of(env, st, out.want), out)


@pytest.mark.parametrize("name", ["test_mul_pt_const_znx_into_aligned", "test_mul_pt_const_assign", "test_mul_add_const_znx_into_aligned",
                                  "test_dot_product_const_znx_aligned"])
def test_control_re_and_im_exchanged(ref, name):
    env, st, out, plan = setup(one(name))
    st = dict(st, csts=[Cst(c.log_delta, c.log_budget, c.im, c.re) for c in st["csts"]])
    cc.step_host(ref, st, plan, env)
    assert misses(dev_of(env, st, out.want), out)


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("name", ["test_add_ct_aligned", "test_add_ct_smaller_output", "test_neg_smaller_output", "test_div_pow2_aligned",
                                  "test_mul_pt_const_znx_into_aligned", "test_dot_product_const_znx_aligned", "rescale_into"])
def test_control_reported_log_budget_off_by_one(ref, name, delta):
    """a correct result read at log_budget +- 1 means another value: T 2^(b +- 1).  At b - 1 the expected torus element doubles; at b + 1
    it halves, to either of the two halves of want mod 1"""
    env, st, out, plan = setup(one(name))
    cc.step_host(ref, st, plan, env)
    assert dev_of(env, st, out.want) <= out.allow
    q = 1 << cm.FINE
    wants = [(out.want * 2) % q] if delta < 0 else [out.want // 2, (out.want // 2 + q // 2) % q]
    assert all(misses(dev_of(env, st, w), out) for w in wants)
