"""CMUX and the loops that are nothing but CMUX, restated from the CPU oracle's per-op calls (oracle/ref.py) in the reference's own order:
poulpy-bin-fhe/src/bdd_arithmetic/eval.rs:524-626 (cmux, cmux_assign_neg, cmux_assign), blind_rotation.rs:45-106 and :196-264
(ggsw_blind_rotation, glwe_blind_rotation / _assign), blind_selection.rs:41-104 (glwe_blind_selection with its sparse HashMap), on top of
poulpy-core's glwe_sub / glwe_sub_assign (api/operations.rs:330-394), glwe_rotate (:423-444) and glwe_external_product_internal
(external_product/glwe.rs:197-271).  Containers are poulpy_amd.layouts objects; every ciphertext, the GGSWs and the results share one base2k
(external_product/glwe.rs:213).  The device entry points pz_glwe_cmux_batched / pz_glwe_blind_rotation_batched must reproduce these digits."""
from __future__ import annotations

import os

import numpy as np

from poulpy_amd.layouts import VecZnx, VecZnxDft


# ---- poulpy-core callees ------------------------------------------------------------------------------------------------------------
def glwe_sub(ref, res: VecZnx, a: VecZnx, b: VecZnx):
    """api/operations.rs:330-376 at equal ranks: vec_znx_sub per column (:359-361)."""
    assert res.cols == a.cols == b.cols
    for i in range(res.cols):
        ref.vec_znx_sub(res, i, a, i, b, i)


def glwe_sub_assign(ref, res: VecZnx, a: VecZnx):
    """api/operations.rs:378-394."""
    assert res.cols == a.cols
    for i in range(a.cols):
        ref.vec_znx_sub_assign(res, i, a, i)


def glwe_rotate(ref, k: int, res: VecZnx, a: VecZnx):
    """api/operations.rs:423-444 at equal ranks."""
    assert res.cols == a.cols
    for i in range(a.cols):
        ref.vec_znx_rotate(k, res, i, a, i)


def glwe_copy(res: VecZnx, a: VecZnx):
    """glwe_copy: vec_znx_copy per column - the common limbs, zero beyond."""
    mn = min(res.size, a.size)
    res.data[:mn] = a.data[:mn]
    res.data[mn:] = 0


def glwe_external_product_internal(ref, a: VecZnx, ggsw, dsize: int):
    """external_product/glwe.rs:197-271 -> the VecZnxBig of ggsw.size limbs (res_dft zeroed by the callers, :122)."""
    n, cols, ksz, a_size = a.n, ggsw.cols_out, ggsw.size, a.size
    assert a.cols == cols == ggsw.cols_in
    res_dft = VecZnxDft(n, cols, ksz)
    a_dft_full = VecZnxDft(n, cols, -(-a_size // dsize))                                  # :225-226
    if dsize == 1:                                                                        # :228-234
        a_dft = a_dft_full.view(a_size)
        for j in range(cols):
            ref.vec_znx_dft_apply(1, 0, a_dft, j, a, j)
        ref.vmp_apply_dft_to_dft(res_dft, a_dft, ggsw, 0)
    else:                                                                                 # :235-267
        tmp_full = VecZnxDft(n, cols, ksz)
        for di in range(dsize):
            a_dft = a_dft_full.view((a_size + di) // dsize)                               # :242
            rd = res_dft.view(ksz - max(dsize - di - 2, 0))                               # :251
            for j in range(cols):
                ref.vec_znx_dft_apply(dsize, dsize - 1 - di, a_dft, j, a, j)              # :253-255
            if di == 0:
                ref.vmp_apply_dft_to_dft(rd, a_dft, ggsw, 0)                              # :258
            else:
                tmp = tmp_full.view(rd.size)                                              # :261
                ref.vmp_apply_dft_to_dft(tmp, a_dft, ggsw, di)
                for col in range(cols):
                    ref.vec_znx_dft_add_assign(rd, col, tmp, col)                         # :263-265
    return ref.vec_znx_idft_apply_consume(res_dft)                                        # :270 (the last iteration left ggsw.size limbs)


# ---- the gate (eval.rs:524-626) -----------------------------------------------------------------------------------------------------
def _add_f_and_normalize(ref, res: VecZnx, big, f: VecZnx, base2k: int):
    for j in range(res.cols):
        ref.vec_znx_big_add_small_assign(big, j, f, j)
        ref.vec_znx_big_normalize(res, base2k, 0, j, big, base2k, j)


def cmux(ref, res: VecZnx, t: VecZnx, f: VecZnx, ggsw, base2k: int, dsize: int = 1):
    """eval.rs:550-572: res = (t - f) s + f; the difference is written into res (:565)."""
    glwe_sub(ref, res, t, f)                                                              # :565
    big = glwe_external_product_internal(ref, res, ggsw, dsize)                           # :566-567
    _add_f_and_normalize(ref, res, big, f, base2k)                                        # :568-571


def cmux_assign_neg(ref, res: VecZnx, a: VecZnx, ggsw, base2k: int, dsize: int = 1):
    """eval.rs:575-603: res = (a - res) s + res; the difference lives in a temporary of ceil(max(res.k, a.k) / base2k) limbs (:590-596)."""
    tmp = VecZnx(res.n, res.cols, max(res.size, a.size))
    glwe_sub(ref, tmp, a, res)                                                            # :596
    big = glwe_external_product_internal(ref, tmp, ggsw, dsize)                           # :597-598
    _add_f_and_normalize(ref, res, big, res, base2k)                                      # :599-602 (column j of res is read, then written)


def cmux_assign(ref, res: VecZnx, a: VecZnx, ggsw, base2k: int, dsize: int = 1):
    """eval.rs:606-625: res = (res - a) s + a."""
    glwe_sub_assign(ref, res, a)                                                          # :618
    big = glwe_external_product_internal(ref, res, ggsw, dsize)                           # :619-620
    _add_f_and_normalize(ref, res, big, a, base2k)                                        # :621-624


def cmux_rotated(ref, res: VecZnx, f: VecZnx, rot: int, ggsw, base2k: int, dsize: int = 1):
    """One step of glwe_blind_rotation_assign (blind_rotation.rs:225-232): res = X^rot f, then cmux_assign(res, f)."""
    glwe_rotate(ref, rot, res, f)
    cmux_assign(ref, res, f, ggsw, base2k, dsize)


# ---- blind rotation by encrypted bits (blind_rotation.rs) ---------------------------------------------------------------------------
def glwe_blind_rotation_assign(ref, res: VecZnx, get_bit, sign: bool, bit_rsh: int, bit_mask: int, bit_lsh: int, base2k: int, dsize: int = 1):
    """blind_rotation.rs:196-242; get_bit(i) -> the prepared GGSW of bit i."""
    tmp_res = VecZnx(res.n, res.cols, res.size)                                           # :212
    a_is_res = True
    for i in range(bit_mask):                                                             # :218
        a, b = (res, tmp_res) if a_is_res else (tmp_res, res)                             # :219-223
        glwe_rotate(ref, (1 << (i + bit_lsh)) if sign else -(1 << (i + bit_lsh)), b, a)   # :226-229
        cmux_assign(ref, b, a, get_bit(i + bit_rsh), base2k, dsize)                       # :232
        a_is_res = not a_is_res                                                           # :235
    if not a_is_res:                                                                      # :239-241
        glwe_copy(res, tmp_res)


def glwe_blind_rotation(ref, res: VecZnx, a: VecZnx, get_bit, sign: bool, bit_rsh: int, bit_mask: int, bit_lsh: int, base2k: int, dsize: int = 1):
    """blind_rotation.rs:246-264."""
    glwe_copy(res, a)                                                                     # :262
    glwe_blind_rotation_assign(ref, res, get_bit, sign, bit_rsh, bit_mask, bit_lsh, base2k, dsize)


def ggsw_blind_rotation(ref, res, a, get_bit, sign: bool, bit_rsh: int, bit_mask: int, bit_lsh: int, base2k: int, dsize: int = 1):
    """blind_rotation.rs:70-106 on MatZnx GGSWs (res.rows <= a.rows, :89): every entry (row, col) through glwe_blind_rotation."""
    assert res.rows <= a.rows
    for col in range(res.cols_in):                                                        # :92-93
        for row in range(res.rows):
            r = VecZnx(res.n, res.cols_out, res.size)
            glwe_blind_rotation(ref, r, a.at(row, col), get_bit, sign, bit_rsh, bit_mask, bit_lsh, base2k, dsize)
            res.data[row, col] = r.data


# ---- blind selection (blind_selection.rs:41-104) ------------------------------------------------------------------------------------
def glwe_blind_selection(ref, res: VecZnx, a: dict, get_bit, bit_rsh: int, bit_mask: int, base2k: int, dsize: int = 1):
    """blind_selection.rs:41-104 with its sparse map {index: VecZnx}: the entries are clobbered, absent ones are zero ciphertexts."""
    a = dict(a)
    for i in range(bit_mask):                                                             # :59
        t = 1 << (bit_mask - i - 1)                                                       # :60
        bit = get_bit(bit_rsh + bit_mask - i - 1)                                         # :62
        for j in range(t):                                                                # :64
            hi, lo = a.pop(j, None), a.pop(j + t, None)                                   # :65-66
            if lo is not None and hi is not None:                                         # :69-72
                cmux_assign(ref, lo, hi, bit, base2k, dsize)
                a[j] = lo
            elif lo is not None:                                                          # :74-79
                zero = VecZnx(res.n, res.cols, res.size)
                cmux_assign(ref, lo, zero, bit, base2k, dsize)
                a[j] = lo
            elif hi is not None:                                                          # :81-87
                zero = VecZnx(res.n, res.cols, res.size)
                cmux_assign(ref, zero, hi, bit, base2k, dsize)
                glwe_copy(hi, zero)
                a[j] = hi
    out = a.pop(0, None)                                                                  # :97
    if out is not None:
        glwe_copy(res, out)                                                               # :99-100
    else:
        res.data[...] = 0                                                                 # :102


def glwe_blind_selection_dense(ref, slots: list, get_bit, bit_rsh: int, bit_mask: int, base2k: int, dsize: int = 1) -> VecZnx:
    """What poulpy_amd.bdd.glwe_blind_selection issues, on the oracle: `slots` = 2^bit_mask ciphertexts of one layout (absent entries zero),
    level i one cmux_assign per pair over the LAST 2t slots, lo = slot T - t + j, hi = slot T - 2t + j.  The result is the last slot."""
    T = 1 << bit_mask
    assert len(slots) == T
    for i in range(bit_mask):
        t = 1 << (bit_mask - i - 1)
        bit = get_bit(bit_rsh + bit_mask - i - 1)
        for j in range(t):
            cmux_assign(ref, slots[T - t + j], slots[T - 2 * t + j], bit, base2k, dsize)
    return slots[T - 1]


# ---- decoding (poulpy-hal layouts/encoding.rs:240-263 on the normalized phase) --------------------------------------------------------
def decode_i64(phase: np.ndarray, base2k: int, k_pt: int) -> np.ndarray:
    """glwe_decrypt + decode_vec_i64: `phase` = (size, n) un-normalized phase limbs; the message at 2^-k_pt, read from the first
    ceil(k_pt / base2k) limbs of the normalized phase (the balanced digits below round it to nearest)."""
    from tests import fhe_sk
    pt = fhe_sk.normalize(phase, base2k)
    size = -(-k_pt // base2k)
    rem = base2k - (k_pt % base2k)
    res = np.zeros(pt.shape[1], dtype=np.int64)
    for j in range(size):
        x = pt[j]
        if j == size - 1 and rem != base2k:
            scale = 1 << rem
            res = (res << ((base2k - rem) % base2k)) + np.floor_divide(x + scale // 2, scale)   # div_round
        else:
            res = (res << base2k) + x
    return res


# ---- shared by the test modules -------------------------------------------------------------------------------------------------------
def blind_rotation_walk(n):
    """(bit_start, bit_size, bit_step, mask) as test_suite/glwe_blind_rotation.rs:93-137 walks them: the two-digit split of log N over a 32-bit k."""
    log_n = n.bit_length() - 1
    base = [log_n >> 1, log_n - (log_n >> 1)]
    out, bit_start = [], 0
    for _ in range(-(-32 // log_n)):
        bit_step = 0
        for digit in base:
            out.append((bit_start, min(32 - bit_start, digit), bit_step, (1 << digit) - 1))
            bit_step += digit
            bit_start += digit
            if bit_start >= 32:
                break
    return out


# the dispatch notes of the device's three CMUX routes
NOTE_ONE, NOTE_TWO, NOTE_MAT = "cmux: fused small-one", "cmux: fused small two-kernel", "cmux: materialised difference"
# composite calls are replayed as HIP graphs unless the graphs are off or the workspaces are guarded (every call plain then)
GRAPHS = os.environ.get("POULPY_DBG_GRAPHS") != "0" and os.environ.get("POULPY_DBG_CANARY") != "1"
