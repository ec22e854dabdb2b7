"""The byte operations of FheUint (poulpy-bin-fhe/src/bdd_arithmetic/ciphertexts/fhe_uint.rs:259-524) restated literally on the oracle, call
by call in the reference's order: get_bit_glwe, get_byte, zero_byte, splice_u8, splice_u16, sext out of vec_znx_rotate (glwe_rotate),
glwe_trace_assign / glwe_trace_assign_bases, vec_znx_add_assign and vec_znx_sub_assign (glwe_add_assign / glwe_sub_assign: no carry, no
normalization) - and a symbolic walk of the same calls that names every trace, against which the device's stage plan is checked."""
from __future__ import annotations

import numpy as np

from poulpy_amd.layouts import VecZnx
from tests.fhe_uint_cases import coefficient

TS = 3     # T::LOG_BITS - T::LOG_BYTES


class Ctx:
    """What every operation takes: the module, the word's base, the log2(n) trace steps with their prepared keys, and - with the keys in
    another base than the word - that base and the word's limb count in it (glwe_trace.rs:153-163).  index (a negative control): where
    bit i of a word lies."""

    def __init__(self, ref, n, word_bits, base2k, gals, keys, key_base2k=None, conv_size=0, index=coefficient):
        self.ref, self.n, self.word_bits, self.base2k, self.gals, self.keys = ref, n, word_bits, base2k, list(gals), list(keys)
        self.key_base2k = base2k if key_base2k is None else key_base2k
        self.conv_size, self.index = conv_size, index
        self.bytes = word_bits // 8

    def c(self, bit):
        return self.index(bit, self.word_bits, self.n)

    def vz(self, data):
        size, cols, n = data.shape
        return VecZnx(n, cols, size, np.ascontiguousarray(data).copy())

    def rotate(self, k, a):
        """glwe_rotate(k, res, a): vec_znx_rotate on every column"""
        res = VecZnx(a.n, a.cols, a.size)
        for col in range(a.cols):
            self.ref.vec_znx_rotate(int(k), res, col, a, col)
        return res

    def trace_assign(self, x, skip):
        if self.key_base2k == self.base2k:
            self.ref.glwe_trace_assign(x, self.base2k, self.gals[skip:], self.keys[skip:])
        else:
            self.ref.glwe_trace_assign_bases(x, self.base2k, self.conv_size, self.key_base2k, self.gals[skip:], self.keys[skip:])

    def add_assign(self, res, a):
        for col in range(a.cols):
            self.ref.vec_znx_add_assign(res, col, a, col)

    def sub_assign(self, res, a):
        for col in range(a.cols):
            self.ref.vec_znx_sub_assign(res, col, a, col)


def get_bit_glwe(ctx, word, bit):
    """:401-414"""
    res = ctx.rotate(-ctx.c(bit), ctx.vz(word))
    ctx.trace_assign(res, 0)
    return res.data


def get_byte(ctx, word, byte):
    """:416-430"""
    res = ctx.rotate(-ctx.c(byte << 3), ctx.vz(word))
    ctx.trace_assign(res, TS)
    return res.data


def _zero_byte(ctx, s, byte):
    """:466-489 on the VecZnx s -> the new s.  glwe_trace with equal layouts is glwe_trace_assign on a copy."""
    rot = ctx.c(byte << 3)
    s = ctx.rotate(-rot, s)
    tmp_trace = ctx.vz(s.data)
    ctx.trace_assign(tmp_trace, TS)
    ctx.sub_assign(s, tmp_trace)
    return ctx.rotate(rot, s)


def _splice_u8(ctx, dst, src, a, b):
    """:286-329 on VecZnx a, b -> the new self"""
    rot = ctx.c(dst << 3)
    s = ctx.vz(a.data)                                   # glwe_copy(self, a)
    s = _zero_byte(ctx, s, dst)
    t = ctx.rotate(-ctx.c(src << 3), b)
    ctx.trace_assign(t, TS)
    t = ctx.rotate(rot, t)
    ctx.add_assign(s, t)
    return s


def zero_byte(ctx, word, byte):
    return _zero_byte(ctx, ctx.vz(word), byte).data


def splice_u8(ctx, dst, src, a, b):
    return _splice_u8(ctx, dst, src, ctx.vz(a), ctx.vz(b)).data


def splice_u16(ctx, dst, src, a, b):
    """:259-282"""
    bv = ctx.vz(b)
    tmp = _splice_u8(ctx, dst << 1, src << 1, ctx.vz(a), bv)
    return _splice_u8(ctx, (dst << 1) + 1, (src << 1) + 1, tmp, bv).data


def sext(ctx, word, byte):
    """:491-524"""
    w = ctx.vz(word)
    log_gap = (ctx.n // ctx.word_bits).bit_length() - 1
    s = ctx.rotate(-ctx.c((byte << 3) + 7), w)
    ctx.trace_assign(s, 0)
    for i in range(3):
        tmp = ctx.rotate((ctx.bytes << log_gap) << i, s)
        ctx.add_assign(s, tmp)
    for i in range(byte + 1, ctx.bytes):
        w = _splice_u8(ctx, i, 0, w, s)                  # into tmp, then glwe_copy(self, tmp)
    return w.data


# ---- the same calls, symbolically: which ciphertext every trace sees, turned by what ---------------------------------------------------------
class Walk:
    """Records the reference's traces as (label of the traced value's source, exponent of X^-e in front of it, skip) and the X^r of every
    zero_byte / splice (the closing steps).  Labels: "a", "b", "s'" (sext's replicated sign), ("word", k) = the running word after k
    splices."""

    def __init__(self, n, word_bits):
        self.n, self.word_bits, self.bytes = n, word_bits, word_bits // 8
        self.traces, self.closings = [], []

    def c(self, bit):
        return coefficient(bit, self.word_bits, self.n)

    def get_bit(self, bit):
        self.traces.append(("a", self.c(bit), 0))

    def get_byte(self, byte):
        self.traces.append(("a", self.c(byte << 3), TS))

    def zero_byte(self, label, byte):
        self.traces.append((label, self.c(byte << 3), TS))
        self.closings.append(self.c(byte << 3))

    def splice_u8(self, dst, src, a_label, b_label):
        self.zero_byte(a_label, dst)
        self.traces.append((b_label, self.c(src << 3), TS))

    def splice_u16(self, dst, src):
        self.splice_u8(dst << 1, src << 1, "a", "b")
        self.splice_u8((dst << 1) + 1, (src << 1) + 1, ("word", 1), "b")

    def sext(self, byte):
        self.traces.append((("word", 0), self.c((byte << 3) + 7), 0))
        for k, i in enumerate(range(byte + 1, self.bytes)):
            self.splice_u8(i, 0, ("word", k), "s'")


def plan_traces(stages, first="a"):
    """The device's stage plan (poulpy_amd.hal.fhe_uint_word_plan) in the Walk's terms: -> (traces, closings).  Source 2, the running word,
    is the word after as many closing steps as stages have combined before this one; `first`: what source 0 is called."""
    traces, closings, combined = [], [], 0
    for st in stages:
        for src, exp, _slot in st["items"]:
            label = {0: first, 1: "b", 2: ("word", combined), 3: "s'"}[src]
            traces.append((label, exp, st["skip"]))
        if st["close"] == 1:
            closings.append(st["r"])
            combined += 1
    return traces, closings


# ---- what the reference's tests expect (bdd_arithmetic/tests/test_suite/fheuint.rs) -----------------------------------------------------------
def _rotr(x, r, w):
    r %= w
    return ((x >> r) | (x << (w - r))) & ((1 << w) - 1)


def want_splice(a, b, dst, src, width, word_bits=32):
    """:133-146, :194-204: c_want = ((a.rotate_right(rj) & !low) | (b.rotate_right(ri) & low)).rotate_left(rj), low = the width low bits"""
    rj, ri, low, full = dst * width, src * width, (1 << width) - 1, (1 << word_bits) - 1
    c = (_rotr(a, rj, word_bits) & (full ^ low)) | (_rotr(b, ri, word_bits) & low)
    return _rotr(c, word_bits - rj, word_bits)


def want_sext(x, bits, word_bits=32):
    """:82-86"""
    full = (1 << word_bits) - 1
    lo = x & ((1 << bits) - 1)
    hi = ((x >> bits) & 1) * ((full << bits) & full)
    return hi | lo
