"""The cases of the weighted sums by constants, shared by tests/test_ckks_lincomb_host.py (plans, oracle, the stand-alone walk) and
tests/test_gpu_ckks_lincomb.py (the device): metadata chosen so that every branch of the reference is taken.

A product's budget is a.log_budget - cst.log_delta, less the offset that squeezes it into dst (get_mul_const_params, leveled/default/mul.rs:
498-513).  The budget lists below give, per term, the product budget wanted; the operand's budget follows from it.  With running minimum m:
  equal       every join is plain
  ascending   every later product has more budget than m: glwe_lsh_add by 7 (< base2k) and by base2k + 2 (more than a limb)
  descending  a later product has less: glwe_lsh_assign on the accumulator by 7 and by base2k + 2, then equal ones
The constants cycle through {re, im, both, neither} and through three metadata (min_k = 0: cnv_offset below base2k; = base2k; = 2 base2k).
"""
from __future__ import annotations

import numpy as np

from poulpy_amd.ckks import Cst, Ct
from poulpy_amd.layouts import VecZnx

SIZES = [(3, 4), (5, 3)]     # (a_size, res_size); the second has product limbs below res (the carry-only range)
FORMS = ["re", "im", "both", "none"]


def budgets(B, pattern, n):
    asc = [B - 9, B - 2, 2 * B - 7, 2 * B - 7, 2 * B]
    desc = [2 * B, 2 * B - 7, B - 9, B - 9, B - 9 - (B - 12)]
    return {"equal": [B + 2] * n, "ascending": asc[:n], "descending": desc[:n]}[pattern]


def constant(rng, B, form, meta, b_size=3):
    """digits in [-2^(B-1), 2^(B-1)), the first of each array negative"""
    h = 1 << (B - 1)

    def digits():
        d = rng.integers(-h, h, b_size, dtype=np.int64)
        d[0] = -abs(int(d[0])) - 1 if d[0] > -h else d[0]
        return d
    log_delta, log_budget = meta
    return Cst(log_delta, log_budget, digits() if form in ("re", "both") else None, digits() if form in ("im", "both") else None)


def cst_metas(B):
    return [(0, 0), (3, 2 * B - 3), (3, B - 3)]


def term(rng, B, a_size, res_size, want_budget, form, meta):
    """(operand Ct, Cst) whose product into a res_size-limb dst has log_budget `want_budget`; at the cap of dst (2 B with log_delta B and
    the (5, 3) sizes) the operand carries 5 bits more, which the product's offset takes away again"""
    c = constant(rng, B, form, meta)
    log_budget = want_budget + c.log_delta
    if a_size > res_size and want_budget + B == res_size * B:
        log_budget += 5
    return Ct(B, a_size, B, log_budget), c


def scenarios(B, seed=0):
    """-> [dict(label, kind: "dot" | "add" | "sub", dst: Ct, ops: [Ct], csts: [Cst], shared: (indices), wide: bool)]"""
    rng = np.random.default_rng(1000 * B + seed)
    out = []
    for si, (a_size, res_size) in enumerate(SIZES):
        metas = cst_metas(B)
        for n, patterns in ((1, ["equal"]), (2, ["equal", "ascending", "descending"]), (5, ["equal", "ascending", "descending"])):
            for pi, pattern in enumerate(patterns):
                ops, csts = [], []
                for i, b in enumerate(budgets(B, pattern, n)):
                    o, c = term(rng, B, a_size, res_size, b, FORMS[(i + pi + si + n) % 4], metas[(i + pi) % 3])
                    ops.append(o)
                    csts.append(c)
                wide = (pi + n + si) % 2 == 1
                shared = (n - 1,) if n > 1 and pattern == "ascending" else ()
                out.append(dict(label=f"dot{n}_{pattern}_{a_size}_{res_size}", kind="dot", dst=Ct(B, res_size, 0, 0), ops=ops, csts=csts, shared=shared,
                                wide=wide))
        # a dot product of real constants only (the unpaired mapping), and one whose first constant is empty
        for n, forms in ((2, ["re", "none"]), (5, ["re"] * 5), (2, ["none", "both"])):
            ops, csts = [], []
            for i, b in enumerate(budgets(B, "descending" if n == 5 else "ascending", n)):
                o, c = term(rng, B, a_size, res_size, b, forms[i], metas[i % 3])
                ops.append(o)
                csts.append(c)
            out.append(dict(label=f"dot{n}_{'_'.join(forms[:2])}_{a_size}_{res_size}", kind="dot", dst=Ct(B, res_size, 0, 0), ops=ops, csts=csts, shared=(),
                            wide=n == 5))
        # mul_add / mul_sub on a dst with a higher, an equal and a lower budget than the product's
        for kind in ("add", "sub"):
            for di, (d, form) in enumerate(((7, "both"), (0, "im"), (-(B + 2), "re"), (B - 5, "none"))):
                prod = 2 * B - 7 if d <= 0 else B - 2
                o, c = term(rng, B, a_size, res_size, prod, form, metas[di % 3])
                out.append(dict(label=f"mul_{kind}_{form}_{d}_{a_size}_{res_size}", kind=kind, dst=Ct(B, res_size, B - 1, prod + d), ops=[o], csts=[c],
                                shared=(0,) if di == 1 else (), wide=(di + si) % 2 == 0))
    return out


def fill(rng, shape, base2k, wide):
    """normalized digits, or un-normalized limbs as tests/test_gpu_ckks_linear.py::_fill makes them"""
    if wide:
        return rng.integers(-(1 << 62), 1 << 62, shape, dtype=np.int64)
    h = 1 << (base2k - 1)
    return rng.integers(-h, h, shape, dtype=np.int64)


def host_inputs(rng, sc, n, cols, pool):
    """-> {"dst": (pool, size, cols, n), i: (pool | 1, size, cols, n)}; dst is wide only where the sum starts from it"""
    host = {"dst": np.stack([fill(rng, (sc["dst"].size, cols, n), sc["dst"].base2k, sc["wide"]) for _ in range(pool)])}
    for i, o in enumerate(sc["ops"]):
        m = 1 if i in sc["shared"] else pool
        host[i] = np.stack([fill(rng, (o.size, cols, n), o.base2k, sc["wide"]) for _ in range(m)])
    return host


def on_host(sc, host, t, n, cols):
    """the scenario's containers for pool item t: (dst Ct, [operand Ct]) with fresh VecZnx copies"""
    def ct(o, arr):
        return Ct(o.base2k, o.size, o.log_delta, o.log_budget, cols, VecZnx(n, cols, o.size, arr.copy()))
    dst = ct(sc["dst"], host["dst"][t])
    ops = [ct(o, host[i][0 if i in sc["shared"] else t]) for i, o in enumerate(sc["ops"])]
    return dst, ops
