"""The conditional swap and the butterfly network built on it, restated from the CPU oracle's per-op calls (oracle/ref.py) in the reference's
own order: poulpy-bin-fhe/src/bdd_arithmetic/eval.rs:417-461 (Cswap::cswap, the branch where the ciphertexts and the GGSW share one base2k)
and blind_retrieval.rs:195-266 (glwe_blind_retrieval_statefull / _rev).  The callees are those of tests/cmux_oracle.py (glwe_sub,
glwe_external_product_internal) plus vec_znx_big_add_small_into / vec_znx_big_sub_small_a on a one-column temporary.  The device entry points
pz_glwe_cswap_batched / pz_glwe_blind_retrieval_batched must reproduce these digits."""
from __future__ import annotations

import numpy as np

from poulpy_amd.layouts import VecZnx, VecZnxBig
from tests import cmux_oracle as co


def _column(big: VecZnxBig, j: int) -> VecZnxBig:
    """A one-column copy of column j of the big value (res_big_tmp, eval.rs:447)."""
    return VecZnxBig(big.n, 1, big.size, np.ascontiguousarray(big.data[:, j:j + 1]))


def cswap(ref, a: VecZnx, b: VecZnx, ggsw, base2k: int, dsize: int = 1):
    """eval.rs:432-461, in place: a' = (b - a) s + a, b' = b - (b - a) s - ONE external product, both results from its big value."""
    assert a.cols == b.cols
    tmp_c = VecZnx(a.n, a.cols, max(a.size, b.size))                                      # :436-443, k = max(res_a.max_k, res_b.max_k)
    co.glwe_sub(ref, tmp_c, b, a)                                                         # :443
    big = co.glwe_external_product_internal(ref, tmp_c, ggsw, dsize)                      # :444
    # both one-column copies of every column are taken from `big` before either result is written (the reference reads res_big, never a or b,
    # once the product is made - the operand column j of a / b is read right before that column is written)
    for_a = [_column(big, j) for j in range(a.cols)]
    for_b = [_column(big, j) for j in range(b.cols)]
    for j in range(a.cols):                                                               # :450-453
        ref.vec_znx_big_add_small_assign(for_a[j], 0, a, j)                               # big[j] + a[j]
        ref.vec_znx_big_normalize(a, base2k, 0, j, for_a[j], base2k, 0)
    for j in range(b.cols):                                                               # :456-459
        ref.vec_znx_big_sub_small_negate_assign(for_b[j], 0, b, j)                        # b[j] - big[j]
        ref.vec_znx_big_normalize(b, base2k, 0, j, for_b[j], base2k, 0)


def glwe_blind_retrieval(ref, res_list: list, get_bit, bit_rsh: int, bit_mask: int, base2k: int, dsize: int = 1):
    """blind_retrieval.rs:214-236: res_list[0] ends up holding element (k >> bit_rsh) mod 2^bit_mask; get_bit(i) -> the prepared GGSW of bit i."""
    for i in range(bit_mask):                                                             # :226
        t = 1 << (bit_mask - i - 1)                                                       # :227
        bit = get_bit(bit_rsh + bit_mask - i - 1)                                         # :228
        for j in range(t):                                                                # :229
            if j + t < len(res_list):                                                     # :230
                cswap(ref, res_list[j], res_list[j + t], bit, base2k, dsize)              # :231-232


def glwe_blind_retrieval_rev(ref, res_list: list, get_bit, bit_rsh: int, bit_mask: int, base2k: int, dsize: int = 1):
    """blind_retrieval.rs:243-265: the same network in the opposite order."""
    for i in reversed(range(bit_mask)):                                                   # :255
        t = 1 << (bit_mask - i - 1)
        bit = get_bit(bit_rsh + bit_mask - i - 1)
        for j in range(t):
            if j < len(res_list) and j + t < len(res_list):                               # :259
                cswap(ref, res_list[j], res_list[j + t], bit, base2k, dsize)


def retrieval_levels(nslots: int, nbits: int, reverse: bool = False) -> list:
    """The dense form pz_glwe_blind_retrieval_batched issues: [(t, index into bits, cnt)] in call order - level i pairs slot j with slot j + t for
    j < cnt = min(t, nslots - t) (0 once t >= nslots); levels with cnt == 0 are kept in the list (they launch nothing)."""
    out = []
    for i in (reversed(range(nbits)) if reverse else range(nbits)):
        t = 1 << (nbits - 1 - i)
        out.append((t, nbits - 1 - i, min(t, nslots - t) if t < nslots else 0))
    return out


def reference_pairs(nslots: int, nbits: int, reverse: bool = False) -> list:
    """[(bit index, j, j + t)] in the order the reference's loops swap them (blind_retrieval.rs:226-233 / :255-262)."""
    out = []
    for i in (reversed(range(nbits)) if reverse else range(nbits)):
        t = 1 << (nbits - i - 1)
        for j in range(t):
            if j < nslots and j + t < nslots:
                out.append((nbits - i - 1, j, j + t))
    return out


# the dispatch notes of the device's three conditional-swap routes
NOTE_ONE, NOTE_TWO, NOTE_MAT = "cswap: fused small-one", "cswap: fused small two-kernel", "cswap: materialised difference"
