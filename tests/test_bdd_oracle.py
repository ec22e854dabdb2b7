"""CPU: the BDD circuits poulpy_amd.bdd builds compute what they should on clear bits, and the restatement of the circuit evaluator
(tests/bdd_oracle.py) means what it should under real keys (tests/fhe_sk.py: exact integer arithmetic, neither the oracle's transforms nor the
device): the outputs of an encrypted 3-bit addition decrypt to a + b, within the noise of the gates on the longest path."""
import math
import random

import numpy as np
import pytest

from poulpy_amd import bdd
from poulpy_amd.layouts import MatZnx
from tests import bdd_oracle as bo
from tests import cmux_oracle as co
from tests import fhe_sk
from tests.helpers import seeded


def _value(circuit, x, n_in):
    return sum(b << i for i, b in enumerate(bdd.eval_plain(circuit, [(x >> i) & 1 for i in range(n_in)])))


def _interleaved(w):
    return [v for j in range(w) for v in (j, w + j)]


@pytest.mark.parametrize("w", [2, 3])
def test_truth_table_adder_with_carry_out(w):
    m = (1 << w) - 1
    for order in (None, _interleaved(w)):
        c = bdd.from_truth_table(lambda x: (x & m) + (x >> w), 2 * w, w + 1, order)
        assert c.input_size == 2 * w and c.output_size == w + 1
        for x in range(1 << (2 * w)):
            assert _value(c, x, 2 * w) == (x & m) + (x >> w), (w, order, x)


def test_truth_table_xor_ltu_and_a_constant_zero_output():
    w = 2
    m = (1 << w) - 1
    x_c = bdd.from_truth_table(lambda x: (x & m) ^ (x >> w), 2 * w, w)
    l_c = bdd.from_truth_table(lambda x: int((x & m) < (x >> w)), 2 * w, 1)
    # bit 0: x0, bit 1: the constant zero (state_size 0, no nodes), bit 2: the constant one, bit 3: not x1
    z_c = bdd.from_truth_table(lambda x: (x & 1) | 4 | ((~x >> 1) & 1) << 3, 2, 4)
    assert z_c.outputs[1] == ([], 0) and z_c.outputs[0][1] == 2
    for x in range(1 << (2 * w)):
        assert _value(x_c, x, 2 * w) == (x & m) ^ (x >> w)
        assert _value(l_c, x, 2 * w) == int((x & m) < (x >> w))
    for x in range(4):
        assert _value(z_c, x, 2) == (x & 1) | 4 | ((~x >> 1) & 1) << 3


def test_every_circuit_keeps_the_node_format():
    """Chunks of state_size nodes, indices below state_size, selectors below input_size, the last chunk [Cmux, None, ...]."""
    for c in (bdd.adder(5, carry_out=True), bdd.sub(4), bdd.xor(3), bdd.ltu(4), bdd.from_truth_table(lambda x: x * 3, 3, 5)):
        for nodes, s in c.outputs:
            if s == 0:
                assert nodes == []
                continue
            assert len(nodes) % s == 0 and len(nodes) >= s
            for kind, sel, hi, lo in nodes:
                assert kind in (bdd.NONE, bdd.COPY, bdd.CMUX)
                if kind == bdd.CMUX:
                    assert hi < s and lo < s and sel < c.input_size
            assert nodes[-s][0] == bdd.CMUX and all(nd[0] == bdd.NONE for nd in nodes[len(nodes) - s + 1:])


@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_structural_circuits_agree_with_the_truth_table_build(w):
    m = (1 << w) - 1
    fns = {"adder": (bdd.adder(w), lambda a, b: (a + b) & m, w), "adder+carry": (bdd.adder(w, carry_out=True), lambda a, b: a + b, w + 1),
           "sub": (bdd.sub(w), lambda a, b: (a - b) & m, w), "xor": (bdd.xor(w), lambda a, b: a ^ b, w), "ltu": (bdd.ltu(w), lambda a, b: int(a < b), 1)}
    for name, (c, fn, n_out) in fns.items():
        t = bdd.from_truth_table(lambda x: fn(x & m, x >> w), 2 * w, n_out, _interleaved(w))
        assert c.outputs == t.outputs, (name, w)   # the same reduced BDD, the same layout
        for a in range(1 << w):
            for b in range(1 << w):
                bits = bdd.word_bits(a, b, w)
                assert sum(v << i for i, v in enumerate(bdd.eval_plain(c, bits))) == fn(a, b), (name, w, a, b)


def test_adder_32():
    c = bdd.adder(32)
    assert c.input_size == 64 and c.output_size == 32
    assert c.max_state_size <= 3 and c.max_depth <= 64
    assert c.count(bdd.CMUX) == 1584 and c.count(bdd.COPY) == 961   # (the node counts of the u32 addition this mirrors)
    rng = random.Random(32)
    pairs = [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(1000)] + [(0xFFFFFFFF, 1), (0, 0), (0x80000000, 0x80000000)]
    for a, b in pairs:
        got = sum(v << i for i, v in enumerate(bdd.eval_plain(c, bdd.word_bits(a, b, 32))))
        assert got == (a + b) & 0xFFFFFFFF, (hex(a), hex(b), hex(got))


def test_none_keeps_the_stale_value_of_its_bank():
    """A None slot holds what was written two levels earlier: a hand-made circuit that depends on it."""
    s = 2
    nodes = [(bdd.CMUX, 0, 1, 0), (bdd.NONE, 0, 0, 0),     # bank B: [x0, 0]
             (bdd.CMUX, 1, 1, 0), (bdd.CMUX, 0, 0, 1),     # bank A: [x1 ? B[1] : B[0], x0 ? B[0] : B[1]] = [x1 ? 0 : x0, x0]
             (bdd.NONE, 0, 0, 0), (bdd.COPY, 0, 0, 0),     # bank B: [x0 (stale), A[1] = x0]
             (bdd.CMUX, 2, 0, 1), (bdd.NONE, 0, 0, 0)]     # x2 ? B[0] : B[1]
    c = bdd.Circuit(3, [(nodes, s)])
    for x in range(8):
        assert bdd.eval_plain(c, [(x >> i) & 1 for i in range(3)]) == [x & 1]


# ---- under real keys ---------------------------------------------------------------------------------------------------------------------
N, BASE2K, SIZE, DNUM, K_PT, W = 64, 12, 3, 3, 2, 3
K_GLWE, K_GGSW = BASE2K * SIZE, BASE2K * (SIZE + 1)


def noise_bound(rank: int, depth: int) -> float:
    """Every gate on a path adds the noise of one external product to its output (the selected source passes through with the noise it has);
    the products are independent, so over a path of `depth` gates the variances add - the way tests/core_cases.py adds the variances of the
    terms of one output - on top of the reference's bound for one product (external_product/glwe_ct.rs:133-152 as
    fhe_sk.external_product_bound states it, its + 1 bit included; the message here is the monomial 2^-2 or zero, below the bound's own
    model).  tests/test_core_semantics.py has no looser allowance for chains: none is added."""
    return fhe_sk.external_product_bound(N, BASE2K, rank, K_GLWE, K_GGSW) + 0.5 * math.log2(depth)


@pytest.mark.parametrize("rank", [1, 2])
def test_encrypted_three_bit_addition_decrypts(rank):
    from oracle.ref import RefModule
    ref, rng = RefModule(N), seeded(9300 + rank)
    sk = fhe_sk.ternary_secret(N, rank, rng)
    ggsw = {}
    for v in (0, 1):
        msg = np.zeros(N, dtype=np.int64)
        msg[0] = v
        g = fhe_sk.ggsw_encrypt(sk, msg, BASE2K, K_GGSW, DNUM, 1, rng)
        dnum, cols, size, _, n = g.shape
        ggsw[v] = ref.vmp_pmat_alloc(dnum, cols, cols, size)
        ref.vmp_prepare(ggsw[v], MatZnx(n, dnum, cols, cols, size, np.ascontiguousarray(g)))
    circuit = bdd.adder(W, carry_out=True)
    bound = noise_bound(rank, circuit.max_depth)

    def run(bits):
        return bo.execute_bdd_circuit(ref, circuit, lambda i: ggsw[bits[i]], W + 2, rank + 1, SIZE, BASE2K)

    def decode(out):
        return [int(co.decode_i64(fhe_sk.glwe_phase(ct.data, sk), BASE2K, K_PT)[0]) & 3 for ct in out]

    worst = -math.inf
    for a, b in ((0, 0), (7, 1), (5, 6), (3, 4), (7, 7)):
        bits = bdd.word_bits(a, b, W)
        out = run(bits)
        got = decode(out)
        assert sum(v << i for i, v in enumerate(got[:W + 1])) == a + b, (a, b, got)
        assert not out[W + 1].data.any()                                  # the slot beyond output_size is zeroed
        for o in range(W + 1):
            want = np.zeros(N, dtype=np.int64)
            want[0] = (a + b) >> o & 1
            have = fhe_sk.noise_log2(out[o].data, BASE2K, sk, fhe_sk.encode(want, BASE2K, K_PT, SIZE), BASE2K)
            worst = max(worst, have)
            assert have <= bound, (a, b, o, have, bound)
            assert np.abs(out[o].data).max() <= 1 << (BASE2K - 1)
        # negative control: the GGSW of one input bit exchanged for the other bit's - the decoded sum is that other addition's
        flipped = list(bits)
        flipped[0] ^= 1
        other = decode(run(flipped))
        assert sum(v << i for i, v in enumerate(other[:W + 1])) == (a ^ 1) + b != a + b
    print(f"[noise] 3-bit adder rank {rank}: worst {worst:.2f} bound {bound:.2f}")
