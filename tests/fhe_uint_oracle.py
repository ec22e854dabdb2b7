"""FheUintPrepared::prepare (bdd_arithmetic/ciphertexts/fhe_uint_prepared.rs:399-460) restated as a composition of oracle calls, in the
reference's own per-bit order - the rank-reducing key switch of get_bit_lwe (fhe_uint.rs:385-394) runs once per BIT here, as it does there:

    get_bit_lwe            glwe_keyswitch (optional) -> lwe_from_glwe at bit_index(i) << log_gap
    execute_to_constant    mod_switch_2n (direction Left) -> circuit_bootstrap_bases, log_domain = 1, extension_factor = 1
    ggsw_prepare           vmp_prepare
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import lwe_cases as lc
from tests.fhe_uint_cases import coefficient


class PreparedKey:
    """The BDD key of a case prepared for one module (oracle or device host API), once."""

    def __init__(self, mod, c):
        self.brk = lc.brk_prepared(mod, c)
        self.atk = [lc.prepare(mod, k) for k in c.atk]
        self.tsk = [lc.prepare(mod, k) for k in c.tsk]
        self.ks_glwe = lc.prepare(mod, c.ks_glwe_key)
        self.ks_lwe = {name: lc.prepare(mod, k) for name, k in c.ks_lwe_key.items()}


def get_bit_lwe(ref, c, key, word, bit, word_bits, with_ks_glwe, index=coefficient):
    """fhe_uint.rs:369-399 on one word ((size, rank + 1, n)) -> the LWE (lwe_size, n_lwe + 1)."""
    a = VecZnx(c.n, c.rank + 1, c.word_size, np.ascontiguousarray(word))
    a_b = c.word_b
    if with_ks_glwe:
        mid = VecZnx(c.n, 2, c.mid_size)
        ref.glwe_keyswitch(mid, c.ks_b, a, c.word_b, key.ks_glwe, 1, c.ks_b)
        a, a_b = mid, c.ks_b
    return ref.lwe_from_glwe(c.n_lwe, c.lwe_size, c.lwe_b, a, a_b, index(bit, word_bits, c.n), key.ks_lwe["mid" if with_ks_glwe else "direct"], 1,
                             c.ks_b)


def prepare_word(ref, c, key, word, word_bits, bit_start, bit_count, with_ks_glwe, index=coefficient):
    """-> lwe (bit_count, lwe_size, n_lwe + 1), lwe_2n (bit_count, n_lwe + 1), ggsw (word_bits, res_dnum, cols, res_size, cols, n) with the bits
    outside the range zero (ggsw_zero, :453-459), pmat (word_bits, doubles of one prepared GGSW)."""
    cols = c.rank + 1
    xpa = ref.blind_rotation_x_pow_a()
    lut = VecZnx(c.n, 1, c.lut.shape[1], np.ascontiguousarray(c.lut[0][:, None, :]))
    lwes, lwe_2ns = [], []
    ggsw = np.zeros((word_bits, c.res_dnum, cols, c.res_size, cols, c.n), dtype=np.int64)
    pmat = np.zeros((word_bits, c.res_dnum * cols * cols * c.res_size * c.n), dtype=np.float64)
    for bit in range(bit_start, bit_start + bit_count):
        lwe = get_bit_lwe(ref, c, key, word, bit, word_bits, with_ks_glwe, index)
        lwe_2n = ref.mod_switch_2n(c.n2, lwe, c.lwe_b, True)
        g = MatZnx(c.n, c.res_dnum, cols, cols, c.res_size)
        ref.circuit_bootstrap_bases(g, c.bases, False, np.ascontiguousarray(lwe_2n), lut, key.brk, c.brk_dnum, c.sh["glwe_size"], c.sh["glwe_size"],
                                    c.sh["atk_glwe_size"], c.sh["trace_size"], c.block_size, xpa, c.gals, key.atk, key.tsk, c.gap, 0, 0, 0)
        pm = ref.vmp_pmat_alloc(c.res_dnum, cols, cols, c.res_size)
        ref.vmp_prepare(pm, g)
        lwes.append(lwe)
        lwe_2ns.append(lwe_2n)
        ggsw[bit] = g.data
        pmat[bit] = pm.data.reshape(-1)
    return SimpleNamespace(lwe=np.stack(lwes) if lwes else np.zeros((0, c.lwe_size, c.n_lwe + 1), dtype=np.int64),
                           lwe_2n=np.stack(lwe_2ns) if lwe_2ns else np.zeros((0, c.n_lwe + 1), dtype=np.int64), ggsw=ggsw, pmat=pmat)


def prepare_words(ref, c, key, words, word_bits, bit_start, bit_count, with_ks_glwe, index=coefficient):
    """The batch: every field of prepare_word stacked over the words."""
    per = [prepare_word(ref, c, key, w, word_bits, bit_start, bit_count, with_ks_glwe, index) for w in words]
    return SimpleNamespace(lwe=np.stack([p.lwe for p in per]), lwe_2n=np.stack([p.lwe_2n for p in per]), ggsw=np.stack([p.ggsw for p in per]),
                           pmat=np.stack([p.pmat for p in per]))
