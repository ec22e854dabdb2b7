"""The accumulating shifts and the CKKS linear operations restated in numpy, in the reference's own order.

* vec_znx_lsh::<false> / vec_znx_lsh_sub / vec_znx_rsh::<false> / vec_znx_rsh_sub: poulpy-cpu-ref src/reference/vec_znx/shift.rs:68-180 and
  :245-... with the step functions of reference/znx/normalization.rs, in wrapping int64 (numpy arrays wrap).
* The GLWE / CKKS sequences of poulpy-ckks src/leveled/default/{add,sub,neg,pow2,rescale,pt_znx}.rs, column by column as poulpy-core
  operations/glwe.rs:1096-1330 runs them, built from the restatement above and the C oracle (oracle/ref.py: vec_znx_lsh, vec_znx_add_into,
  vec_znx_sub, vec_znx_negate, vec_znx_normalize_assign ...).  The CKKS metadata rules come from poulpy_amd.ckks.

Containers are poulpy_amd.layouts.VecZnx objects; results are written into `res` in place.  pz_glwe_combine_batched and the four
pz_vec_znx_*_batched shifts must reproduce these digits."""
from __future__ import annotations

import numpy as np

from poulpy_amd import ckks
from poulpy_amd.layouts import VecZnx

_ERR = np.seterr(over="ignore")


def _digit(k, x):      # normalization.rs:4-7
    s = np.int64(64 - k)
    return (x << s) >> s


def _carry(k, x, d):   # :9-12
    return (x - d) >> np.int64(k)


def _first_carry_only(b, lsh, x):                                   # :24-41
    kk = b if lsh == 0 else b - lsh
    return _carry(kk, x, _digit(kk, x))


def _middle_carry_only(b, lsh, x, c):                               # :107-129
    kk = b if lsh == 0 else b - lsh
    d = _digit(kk, x)
    cy = _carry(kk, x, d)
    dpc = (d << np.int64(lsh)) + c
    return cy + _carry(b, dpc, _digit(b, dpc))


def _middle(b, lsh, a, c):                                          # :179-221 (x1 and the new carry)
    kk = b if lsh == 0 else b - lsh
    d = _digit(kk, a)
    cy = _carry(kk, a, d)
    dpc = (d << np.int64(lsh)) + c
    x1 = _digit(b, dpc)
    return x1, cy + _carry(b, dpc, x1)


def _final(b, lsh, a, c):                                           # :275-330
    kk = b if lsh == 0 else b - lsh
    return _digit(b, (_digit(kk, a) << np.int64(lsh)) + c)


def _middle_assign(b, x, c):                                        # :132-157, lsh = 0
    d = _digit(b, x)
    cy = _carry(b, x, d)
    dpc = d + c
    x1 = _digit(b, dpc)
    return x1, cy + _carry(b, dpc, x1)


def _final_assign(b, x, c):                                         # :254-272, lsh = 0
    return _digit(b, _digit(b, x) + c)


def vec_znx_lsh_acc(base2k, k, res: VecZnx, res_col, a: VecZnx, a_col, sub=False):
    """shift.rs:68-135 with OVERWRITE = false (sub=False) and :137-180 (vec_znx_lsh_sub)."""
    res_size, a_size = res.size, a.size
    steps, k_rem = divmod(k, base2k)                                # :90
    if steps >= max(res_size, a_size):                              # :92-100
        return
    min_size = min(res_size, max(a_size - steps, 0))                # :102
    carry_only_start = min(steps + min_size, a_size)                # :103
    c = np.zeros(res.n, dtype=np.int64)
    for j in range(a_size - 1, carry_only_start - 1, -1):           # :105-111
        x = a.at(a_col, j)
        c = _first_carry_only(base2k, k_rem, x) if j == a_size - 1 else _middle_carry_only(base2k, k_rem, x, c)
    for j in range(min_size - 1, -1, -1):                           # :119-125
        x = a.at(a_col, j + steps)
        if j == 0:
            x1 = _final(base2k, k_rem, x, c)
        else:
            x1, c = _middle(base2k, k_rem, x, c)
        r = res.at(res_col, j)
        r[...] = r - x1 if sub else r + x1


def vec_znx_rsh_acc(base2k, k, res: VecZnx, res_col, a: VecZnx, a_col, sub=False):
    """shift.rs:245-342 with OVERWRITE = false (sub=False) and :344-... (vec_znx_rsh_sub)."""
    res_size, a_size = res.size, a.size
    steps, k_rem = divmod(k, base2k)                                # :275-284
    if k_rem != 0:
        steps += 1
    lsh = (base2k - k_rem) % base2k                                 # :286
    res_end = min(res_size, steps)                                  # :287-289
    res_start = min(res_size, a_size + steps)
    a_start = min(a_size, max(res_size - steps, 0))
    a_out_range = max(a_size - a_start, 0)                          # :293
    c = np.zeros(res.n, dtype=np.int64)
    for j in range(a_out_range):                                    # :295-301
        x = a.at(a_col, a_size - j - 1)
        c = _first_carry_only(base2k, lsh, x) if j == 0 else _middle_carry_only(base2k, lsh, x, c)
    for j in range(max(res_start - res_end, 0)):                    # :315-325
        x1, c = _middle(base2k, lsh, a.at(a_col, a_start - j - 1), c)
        r = res.at(res_col, res_start - j - 1)
        r[...] = r - x1 if sub else r + x1
    if sub:                                                         # rsh_sub: the carry is negated before it propagates
        c = -c
    for j in range(res_end):                                        # :334-340
        r = res.at(res_col, res_end - j - 1)
        if j == res_end - 1:
            r[...] = _final_assign(base2k, r, c)
        else:
            r[...], c = _middle_assign(base2k, r, c)


# ---- GLWE primitives (poulpy-core operations/glwe.rs), every column ----------------------------------------------------------------
def glwe_lsh(ref, base2k, k, res, a):                 # :1135-1161
    for i in range(res.cols):
        ref.vec_znx_lsh(base2k, k, res, i, a, i)


def glwe_lsh_assign(ref, base2k, k, res):             # :1114-1133
    for i in range(res.cols):
        ref.vec_znx_lsh_assign(base2k, k, res, i)


def glwe_lsh_add(base2k, k, res, a):                  # :1163-1189
    for i in range(res.cols):
        vec_znx_lsh_acc(base2k, k, res, i, a, i)


def glwe_lsh_sub(base2k, k, res, a):                  # :1191-1215
    for i in range(res.cols):
        vec_znx_lsh_acc(base2k, k, res, i, a, i, sub=True)


def glwe_add_into(ref, res, a, b):
    for i in range(res.cols):
        ref.vec_znx_add_into(res, i, a, i, b, i)


def glwe_sub(ref, res, a, b):
    for i in range(res.cols):
        ref.vec_znx_sub(res, i, a, i, b, i)


def glwe_add_assign(ref, res, a):
    for i in range(res.cols):
        ref.vec_znx_add_assign(res, i, a, i)


def glwe_sub_assign(ref, res, a):
    for i in range(res.cols):
        ref.vec_znx_sub_assign(res, i, a, i)


def glwe_negate(ref, res, a):
    for i in range(res.cols):
        ref.vec_znx_negate(res, i, a, i)


def glwe_negate_assign(ref, res):
    for i in range(res.cols):
        ref.vec_znx_negate_assign(res, i)


def glwe_normalize_assign(ref, base2k, res):          # :1313-1329
    for i in range(res.cols):
        ref.vec_znx_normalize_assign(base2k, res, i)


# ---- CKKS operations (poulpy-ckks leveled/default), `dst` / `a` / `b`: ckks.Ct with a VecZnx in .data ----------------------------------
def _fin(ref, op, dst):
    if op.normalize:
        glwe_normalize_assign(ref, dst.base2k, dst.data)


def run(ref, op: ckks.Plan, dst: ckks.Ct, a: ckks.Ct | None = None, b: ckks.Ct | None = None, pt: ckks.Pt | None = None):
    """Runs the reference sequence of `op` (a ckks.Plan built by poulpy_amd.ckks) on host containers, in the reference's order."""
    B, name = dst.base2k, op.name
    d = dst.data
    if name in ("add_into", "sub_into"):                            # add.rs:76-104, sub.rs:76-104
        sub = name == "sub_into"
        off = op.offset
        if off == 0 and a.log_budget == b.log_budget:
            (glwe_sub if sub else glwe_add_into)(ref, d, a.data, b.data)
        elif a.log_budget <= b.log_budget:
            glwe_lsh(ref, B, off, d, a.data)
            (glwe_lsh_sub if sub else glwe_lsh_add)(B, b.log_budget - a.log_budget + off, d, b.data)
        elif sub:
            glwe_lsh(ref, B, a.log_budget - b.log_budget + off, d, a.data)
            glwe_lsh_sub(B, off, d, b.data)
        else:
            glwe_lsh(ref, B, off, d, b.data)
            glwe_lsh_add(B, a.log_budget - b.log_budget + off, d, a.data)
    elif name in ("add_assign", "sub_assign"):                      # add.rs:120-146, sub.rs:122-146
        sub = name == "sub_assign"
        if dst.log_budget < a.log_budget:
            (glwe_lsh_sub if sub else glwe_lsh_add)(B, a.log_budget - dst.log_budget, d, a.data)
        else:
            if dst.log_budget > a.log_budget:
                glwe_lsh_assign(ref, B, dst.log_budget - a.log_budget, d)
            (glwe_sub_assign if sub else glwe_add_assign)(ref, d, a.data)
    elif name == "neg_into":                                        # neg.rs:21-40
        if op.offset != 0:
            glwe_lsh(ref, B, op.offset, d, a.data)
            glwe_negate_assign(ref, d)
        else:
            glwe_negate(ref, d, a.data)
    elif name == "neg_assign":                                      # neg.rs:42-48
        glwe_negate_assign(ref, d)
    elif name in ("mul_pow2_into", "div_pow2_into", "rescale_into"):   # pow2.rs:25-36, :52-66, rescale.rs:38-52
        glwe_lsh(ref, B, op.shift, d, a.data)
    elif name in ("mul_pow2_assign", "rescale_assign"):             # pow2.rs:38-50, rescale.rs:23-36
        glwe_lsh_assign(ref, B, op.shift, d)
    elif name == "div_pow2_assign":                                 # pow2.rs:68-71: metadata only
        pass
    elif name in ("add_pt_into", "sub_pt_into", "add_pt_assign", "sub_pt_assign"):   # add.rs:148-210, sub.rs analogues, pt_znx.rs:17-53
        if name.endswith("_into"):
            glwe_lsh(ref, B, op.offset, d, a.data)
        (vec_znx_rsh_acc)(B, op.pt_shift, d, 0, pt.data, 0, sub=name.startswith("sub"))
    else:
        raise ValueError(name)
    _fin(ref, op, dst)
