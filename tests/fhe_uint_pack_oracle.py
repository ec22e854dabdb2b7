"""The oracle's statement of FheUint::pack (poulpy-bin-fhe/src/bdd_arithmetic/ciphertexts/fhe_uint.rs:239-255): glwe_pack on the word_bits
single-bit GLWEs of a word, bit s at index bit_index(s) << log_gap, log_gap_out = log_gap = log2(n / word_bits) - and a Python walk of
glwe_pack_default's loop (poulpy-core/src/glwe_packing.rs:147-168) over those indices, which names the two slots of every merge."""
from __future__ import annotations

from poulpy_amd.layouts import VecZnx
from tests.fhe_uint_cases import bit_index


def log_gap(n: int, word_bits: int) -> int:
    assert n % word_bits == 0
    return (n // word_bits).bit_length() - 1


def word_indices(n: int, word_bits: int, index=bit_index) -> list:
    """fhe_uint.rs:250-252: the HashMap key of bit s."""
    return [index(s, word_bits) << log_gap(n, word_bits) for s in range(word_bits)]


def pack_word(ref, bits, word_bits: int, base2k: int, gals, keys, key_base2k=None, trace_size: int = 0, index=bit_index):
    """bits: (word_bits, size, cols, n) int64, slot s = bit s of the word -> (size, cols, n): ref.glwe_pack, or ref.glwe_pack_bases with the
    automorphism keys in key_base2k (trace_size limbs of glwe_trace's temporary).  index (a negative control): where bit s goes."""
    _, size, cols, n = bits.shape
    cts = {j: VecZnx(n, cols, size, bits[s].copy()) for s, j in enumerate(word_indices(n, word_bits, index))}
    assert len(cts) == word_bits
    res = VecZnx(n, cols, size)
    if key_base2k is None or key_base2k == base2k:
        ref.glwe_pack(res, base2k, cts, log_gap(n, word_bits), gals, keys)
    else:
        ref.glwe_pack_bases(res, base2k, key_base2k, trace_size, cts, log_gap(n, word_bits), gals, keys)
    return res.data


def walk_levels(n: int, word_bits: int, index=bit_index):
    """glwe_packing.rs:147-168 on the dict {index: slot}: -> per level the list of (lo slot, hi slot, t) in the order of j, and the set of
    branches of pack_internal (:41-86) the walk met ("both", "lo", "hi")."""
    log_n = n.bit_length() - 1
    lg = log_gap(n, word_bits)
    a = {j: s for s, j in enumerate(word_indices(n, word_bits, index))}
    levels, branches = [], set()
    for i in range(log_n - lg):
        t = min(1 << log_n, 1 << (log_n - 1 - i))
        merges = []
        for j in range(t):
            lo, hi = a.pop(j, None), a.pop(j + t, None)
            if lo is not None and hi is not None:
                branches.add("both")
                merges.append((lo, hi, t))
            elif lo is not None:
                branches.add("lo")
            elif hi is not None:
                branches.add("hi")
            if lo is not None:
                a[j] = lo
            elif hi is not None:
                a[j] = hi
        levels.append(merges)
    assert sorted(a) == [0], "glwe_trace reads a.get(&0)"
    return levels, branches, a[0]
