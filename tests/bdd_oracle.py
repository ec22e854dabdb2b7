"""ExecuteBDDCircuit restated from the CPU oracle's per-op calls in the reference's own order: poulpy-bin-fhe/src/bdd_arithmetic/eval.rs:172-239
(execute_bdd_circuit_multi_thread: a zero output for state_size 0, the outputs beyond output_size zeroed) and :241-305 (eval_level: two banks
of state_size ciphertexts in the layout of the result, all zero but slot 1, a level per chunk of state_size nodes, the banks swapped after every
level, a None slot keeping what its bank held two levels earlier, the last chunk's first node writing the result), on top of tests/cmux_oracle.py
(cmux, glwe_copy).  The device entry point pz_bdd_circuit_execute_batched must reproduce these digits."""
from __future__ import annotations

import numpy as np

from poulpy_amd import bdd
from poulpy_amd.layouts import VecZnx
from tests import cmux_oracle as co

# the dispatch notes of the device's routes
NOTE_ONE, NOTE_TWO, NOTE_GATE = "bdd: gathered small-one", "bdd: gathered small two-kernel", "bdd: per-gate ("


def one_ciphertext(n: int, cols: int, size: int, base2k: int) -> VecZnx:
    """level[1] (eval.rs:262): encode_coeff_i64(base2k, col 0, k = 2, idx 0, 1) on a zero ciphertext (poulpy-hal layouts/encoding.rs:116-155) - the
    value 1 at 2^-2: limb ceil(2 / base2k) - 1 takes 1 << (that limb's bits below 2^-2), then the limbs are normalized."""
    ct = VecZnx(n, cols, size)
    used = -(-2 // base2k)
    assert used <= size
    limbs = np.zeros(size, dtype=np.int64)
    limbs[used - 1] = 1 << (used * base2k - 2)
    half, mask, carry = 1 << (base2k - 1), (1 << base2k) - 1, 0
    for j in reversed(range(used)):   # balanced digits, the carry out of limb 0 dropped
        v = int(limbs[j]) + carry
        d = ((v + half) & mask) - half
        carry = (v - d) >> base2k
        limbs[j] = d
    ct.data[:, 0, 0] = limbs
    return ct


def eval_level(ref, res: VecZnx, get_bit, nodes, state_size: int, base2k: int, dsize: int = 1):
    """eval.rs:241-305."""
    assert len(nodes) % state_size == 0                                                         # :254
    level = [VecZnx(res.n, res.cols, res.size) for _ in range(2 * state_size)]                  # :257-259
    level[1] = one_ciphertext(res.n, res.cols, res.size, base2k)                                # :262
    prev, nxt = level[:state_size], level[state_size:]                                          # :265
    for c in range(0, len(nodes) - state_size, state_size):                                     # :269
        for j, (kind, sel, hi, lo) in enumerate(nodes[c:c + state_size]):
            if kind == bdd.CMUX:
                co.cmux(ref, nxt[j], prev[hi], prev[lo], get_bit(sel), base2k, dsize)           # :272-280
            elif kind == bdd.COPY:
                co.glwe_copy(nxt[j], prev[j])                                                   # :281
        prev, nxt = nxt, prev                                                                   # :286
    kind, sel, hi, lo = nodes[len(nodes) - state_size]
    assert kind == bdd.CMUX, "invalid last node, should be CMUX"                                # :301-303
    co.cmux(ref, res, prev[hi], prev[lo], get_bit(sel), base2k, dsize)                          # :292-299


def execute_bdd_circuit(ref, circuit: bdd.Circuit, get_bit, n_out: int, cols: int, size: int, base2k: int, dsize: int = 1) -> list:
    """eval.rs:172-239 for one input: -> n_out ciphertexts (VecZnx of `size` limbs); get_bit(i) -> the prepared GGSW of input bit i."""
    assert n_out >= circuit.output_size                                                         # :192-197
    out = [VecZnx(ref.n(), cols, size) for _ in range(n_out)]
    for o, (nodes, state_size) in enumerate(circuit.outputs):
        if state_size:                                                                          # :225-229 (else: zero)
            eval_level(ref, out[o], get_bit, nodes, state_size, base2k, dsize)
    return out                                                                                  # :235-237: the rest stays zero


def execute_batch(ref, circuit: bdd.Circuit, bits, n_out: int, cols: int, size: int, base2k: int, dsize: int = 1) -> np.ndarray:
    """`bits[b][i]`: prepared GGSW of input bit i of input b -> the device's dense slot-major buffer (n_out, batch, size, cols, n)."""
    batch = len(bits)
    want = np.zeros((n_out, batch, size, cols, ref.n()), dtype=np.int64)
    for b in range(batch):
        for o, ct in enumerate(execute_bdd_circuit(ref, circuit, lambda i: bits[b][i], n_out, cols, size, base2k, dsize)):
            want[o, b] = ct.data
    return want


# ---- shared by the test modules -------------------------------------------------------------------------------------------------------
_X, _NONE, _COPY = bdd.CMUX, (bdd.NONE, 0, 0, 0), (bdd.COPY, 0, 0, 0)


def hand_circuit() -> bdd.Circuit:
    """Four input bits, four output bits - depth 5 (state 3), a zero output (state 0), depth 1 and depth 2 (state 2) - with every node kind and
    every way a level may lean on its banks:
      output 0, level 0  [cmux(0; 1, 1), cmux(1; 1, 0), none]   hi == lo; two gates read slot 1; the gate at position 1 reads position 1;
                                                                 position 2 of the second bank keeps its initial zero
                level 1  [cmux(2; 0, 2), cmux(0; 1, 1), cmux(1; 0, 1)]   reads that stale position 2
                level 2  [none, copy, cmux(2; 2, 0)]             position 0 stays stale (level 0's gate), position 2 is overwritten at last
                level 3  [cmux(0; 0, 2), none, none]             reads the stale position 0; positions 1 and 2 of this bank stay stale
                level 4  [cmux(3; 0, 1), none, none]             the root reads position 1, stale since level 1."""
    return bdd.Circuit(4, [
        ([(_X, 0, 1, 1), (_X, 1, 1, 0), _NONE, (_X, 2, 0, 2), (_X, 0, 1, 1), (_X, 1, 0, 1), _NONE, _COPY, (_X, 2, 2, 0), (_X, 0, 0, 2), _NONE, _NONE,
          (_X, 3, 0, 1), _NONE, _NONE], 3),
        ([], 0),
        ([(_X, 3, 1, 0), _NONE], 2),
        ([(_X, 1, 0, 1), (_X, 1, 1, 0), (_X, 2, 1, 0), _NONE], 2),
    ])
