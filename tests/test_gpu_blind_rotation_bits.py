"""pz_glwe_blind_rotation_batched - the CMUX ladder of GLWEBlindRotation (poulpy-bin-fhe bdd_arithmetic/blind_rotation.rs:196-264) - and the
blind-selection helper on the device.

The reference's own test (tests/test_suite/glwe_blind_rotation.rs: data[i] = i, a 32-bit k encrypted bit by bit, coefficient 0 of the
result against ((k >> bit_start) & mask) << bit_step) on a batch of three plaintexts sharing k, at N = 256 (materialised difference) and
N = 1024 (fused forward stage); every output against tests/cmux_oracle.py bit for bit; equality with nbits single CMUX calls; HIP-graph
replay with new contents in the same buffers; the rows of a GGSW as a batch; blind selection over a dense slot-major buffer with holes."""
import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import cmux_oracle as co
from tests.cmux_oracle import GRAPHS, NOTE_MAT as MAT, NOTE_ONE as ONE, NOTE_TWO as TWO
from tests import fhe_sk
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu

BATCH = 3
# n -> (rank, base2k, k_glwe, k_ggsw, dnum, note): the reference's parameters at N = 256; rank 1, base2k 12 on the fused small-ring kernel
SHAPES = {256: (2, 13, 26, 39, 3, MAT), 1024: (1, 12, 24, 36, 3, ONE)}
NBITS = 10


class Setup:
    """Secret, a random k with its NBITS low bits as prepared GGSWs (oracle and device), three test vectors data_b[i] = i + 3 b."""

    def __init__(self, ref, hip, n):
        from poulpy_amd.hal import GlweOpParams
        self.n, self.ref, self.hip = n, ref, hip
        self.rank, self.base2k, k_glwe, k_ggsw, self.dnum, self.note = SHAPES[n]
        rng = self.rng = seeded(18000 + n)
        self.cols = self.rank + 1
        self.sk = fhe_sk.ternary_secret(n, self.rank, rng)
        self.k = int(rng.integers(0, 1 << NBITS)) | 1 | (1 << (NBITS - 1))
        self.size, self.ksz = fhe_sk.limbs_for(k_glwe, self.base2k), fhe_sk.limbs_for(k_ggsw, self.base2k)
        self.keys = []
        for i in range(NBITS):
            msg = np.zeros(n, dtype=np.int64)
            msg[0] = (self.k >> i) & 1
            mat = MatZnx(n, self.dnum, self.cols, self.cols, self.ksz,
                         np.ascontiguousarray(fhe_sk.ggsw_encrypt(self.sk, msg, self.base2k, k_ggsw, self.dnum, 1, rng)))
            self.keys.append(prepared_key(ref, hip, mat))
        # the plaintext container the reference rotates (a GLWE with a zero mask), one per ciphertext of the batch
        self.k_pt = self.base2k
        self.data = np.stack([(np.arange(n, dtype=np.int64) + 3 * b) % n for b in range(BATCH)])
        self.a = np.zeros((BATCH, self.size, self.cols, n), dtype=np.int64)
        for b in range(BATCH):
            self.a[b, :, 0] = fhe_sk.encode(self.data[b], self.base2k, self.k_pt, self.size)
        self.p = GlweOpParams(rank=self.rank, dnum=self.dnum, dsize=1, key_size=self.ksz, key_base2k=self.base2k, a_size=self.size,
                              a_base2k=self.base2k, res_size=self.size, res_base2k=self.base2k, rank_out=self.rank)

    def get_bit(self, i):
        return self.keys[i][0]

    def oracle(self, a, sign, rsh, nbits, lsh):
        want = np.empty_like(a)
        for b in range(a.shape[0]):
            res = VecZnx(self.n, self.cols, self.size)
            co.glwe_blind_rotation(self.ref, res, VecZnx(self.n, self.cols, self.size, a[b].copy()), self.get_bit, sign, rsh, nbits, lsh, self.base2k)
            want[b] = res.data
        return want


@pytest.fixture(scope="module")
def setups(mods):
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = Setup(*mods(n), n)
        return cache[n]
    return get


class Ladder:
    """Device buffers of one argument set: the keys, a, res, tmp - allocated once, contents replaced between calls."""

    def __init__(self, dev, s, in_place=False):
        self.s, self.in_place = s, in_place
        self.d_keys = [dev.key(ph) for _, ph in s.keys]
        self.d_a = dev.alloc(s.a.nbytes, poison=False)
        self.d_res = self.d_a if in_place else dev.alloc(s.a.nbytes)
        self.tmp_bytes = s.hip.glwe_blind_rotation_tmp_bytes(s.p, BATCH)
        assert self.tmp_bytes == s.a.nbytes
        self.d_tmp = dev.alloc(self.tmp_bytes)

    def run(self, a, sign, rsh, nbits, lsh):
        s = self.s
        self.d_a.upload(a)
        s.hip.glwe_blind_rotation_batched(self.d_res.ptr, self.d_a.ptr, [self.d_keys[rsh + i].ptr for i in range(nbits)], sign, lsh, s.p,
                                          self.d_tmp.ptr, self.tmp_bytes, BATCH)
        s.hip.sync()
        return self.d_res.download(np.int64, a.size).reshape(a.shape)


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_the_references_own_test_through_the_device(mods, setups, n):
    """test_suite/glwe_blind_rotation.rs:93-137 on the low NBITS bits of k (its walk of bit_start / bit_size / bit_step, cut at NBITS), sign
    false as there; three plaintexts sharing k.  Even and odd step counts both occur (N = 256: 4; N = 1024: 5)."""
    s = setups(n)
    sizes = set()
    with on_device(s.hip, chunk=2) as dev:
        lad = Ladder(dev, s)
        s.hip.dispatch_notes(reset=True)
        for bit_start, bit_size, bit_step, mask in co.blind_rotation_walk(n):
            if bit_start + bit_size > NBITS:
                break
            sizes.add(bit_size)
            got = lad.run(s.a, False, bit_start, bit_size, bit_step)
            assert np.array_equal(got, s.oracle(s.a, False, bit_start, bit_size, bit_step)), (n, bit_start, "device != oracle")
            want0 = ((s.k >> bit_start) & mask) << bit_step
            for b in range(BATCH):
                dec = co.decode_i64(fhe_sk.glwe_phase(got[b], s.sk), s.base2k, s.k_pt)
                assert int(dec[0]) == int(s.data[b][want0 % n]) * (1 if want0 < n else -1), (n, b, bit_start)
                assert np.array_equal(dec, fhe_sk.rotate(s.data[b], -want0)), (n, b, bit_start, "whole polynomial")
        assert s.note in s.hip.dispatch_notes(), s.hip.dispatch_notes()
    assert sizes, "the walk ran no rotation"


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_signs_step_counts_and_the_assign_form(mods, setups, n):
    """Both signs; 0 steps (a copy), odd counts (the final copy out of tmp, blind_rotation.rs:238-241) and even ones; res == a."""
    s = setups(n)
    with on_device(s.hip, chunk=2) as dev:
        out, inp = Ladder(dev, s), Ladder(dev, s, in_place=True)
        for sign in (True, False):
            for rsh, nbits, lsh in ((0, 0, 0), (0, 1, 0), (1, 2, 1), (2, 3, 0), (0, 4, 2), (3, 5, 1)):
                want = s.oracle(s.a, sign, rsh, nbits, lsh)
                assert np.array_equal(out.run(s.a, sign, rsh, nbits, lsh), want), (n, sign, rsh, nbits, lsh)
                assert np.array_equal(inp.run(s.a, sign, rsh, nbits, lsh), want), (n, sign, rsh, nbits, lsh, "res == a")
                r = (((s.k >> rsh) & ((1 << nbits) - 1)) << lsh) * (1 if sign else -1)
                for b in range(BATCH):
                    assert np.array_equal(co.decode_i64(fhe_sk.glwe_phase(want[b], s.sk), s.base2k, s.k_pt), fhe_sk.rotate(s.data[b], r))


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_ladder_equals_single_cmux_calls(mods, setups, n):
    s = setups(n)
    rng = seeded(18100 + n)
    a = np.stack([VecZnx(n, s.cols, s.size).fill_uniform(s.base2k, rng).data for _ in range(BATCH)])
    rsh, nbits, lsh = 1, 3, 2
    with on_device(s.hip, chunk=2, graphs=False) as dev:
        lad = Ladder(dev, s)
        got = lad.run(a, True, rsh, nbits, lsh)
        bufs = [dev.upload(a), dev.alloc(a.nbytes)]
        for i in range(nbits):
            s.hip.glwe_cmux_batched(bufs[1].ptr, None, bufs[0].ptr, lad.d_keys[rsh + i].ptr, s.p, BATCH, t_size=s.size, f_size=s.size, t_rot=1 << (i + lsh))
            bufs.reverse()
        s.hip.sync()
        assert np.array_equal(bufs[0].download(np.int64, a.size).reshape(a.shape), got)
    assert np.array_equal(got, s.oracle(a, True, rsh, nbits, lsh))


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_repeated_calls_replay_a_graph_with_new_contents(mods, n):
    """Three calls with new contents in the same buffers on a module of the test's own: every output bit-exact, and the repeats are served by
    a HIP graph (the first call of a module sizes its workspaces, which are part of the key: the capture may fall on the third call)."""
    from poulpy_amd.hal import Module
    ref, _ = mods(n)
    hip = Module(n)
    hip.set_graphs(True)
    s = Setup(ref, hip, n)
    with on_device(hip, chunk=2) as dev:
        lad = Ladder(dev, s)
        first = hip.graph_launches()
        after = []
        for call in range(4):
            a = np.stack([VecZnx(n, s.cols, s.size).fill_uniform(s.base2k, s.rng).data for _ in range(BATCH)])
            assert np.array_equal(lad.run(a, True, 0, 3, 1), s.oracle(a, True, 0, 3, 1)), (n, "call", call)
            after.append(hip.graph_launches())
        if GRAPHS:
            assert after[0] == first and after[2] > after[0] and after[3] == after[2] + 1, (first, after)
        else:
            assert after[3] == first
    hip.close()


def test_the_rows_of_a_ggsw_are_a_batch(mods, setups):
    """ggsw_blind_rotation (blind_rotation.rs:70-106): one GGSW of dnum 2, rank 1 - its dnum (rank + 1) GLWE entries are contiguous."""
    n = 1024
    s = setups(n)
    rng = seeded(18200)
    dnum = 2
    a = MatZnx(n, dnum, s.cols, s.cols, s.size).fill_uniform(s.base2k, rng)
    want = MatZnx(n, dnum, s.cols, s.cols, s.size)
    co.ggsw_blind_rotation(s.ref, want, a, s.get_bit, False, 2, 3, 1, s.base2k)
    entries = dnum * s.cols
    with on_device(s.hip, chunk=3) as dev:
        d_keys = [dev.key(ph) for _, ph in s.keys]
        d_a, d_res = dev.upload(a.data), dev.alloc(a.data.nbytes)
        tb = s.hip.glwe_blind_rotation_tmp_bytes(s.p, entries)
        d_tmp = dev.alloc(tb)
        s.hip.glwe_blind_rotation_batched(d_res.ptr, d_a.ptr, [d_keys[2 + i].ptr for i in range(3)], False, 1, s.p, d_tmp.ptr, tb, entries)
        s.hip.sync()
        got = d_res.download(np.int64, a.data.size).reshape(a.data.shape)
    assert np.array_equal(got, want.data)


def test_argument_errors_launch_nothing(mods, setups):
    from poulpy_amd import abi
    s = setups(1024)
    hip = s.hip
    with on_device(hip) as dev:
        lad = Ladder(dev, s)
        lad.d_a.upload(s.a)
        ptrs = [lad.d_keys[i].ptr for i in range(2)]
        ct = s.a.nbytes // BATCH
        import ctypes as C
        arr = (C.c_void_p * 2)(*[p.value for p in ptrs])

        def call(res, a, tmp, tmp_bytes):
            st = hip.lib.pz_glwe_blind_rotation_batched(hip.handle, res, a, 2, arr, 1, 0, C.byref(s.p), tmp, tmp_bytes, BATCH)
            return st, hip.lib.pz_last_error().decode()
        st, msg = call(lad.d_res.ptr, lad.d_a.ptr, lad.d_tmp.ptr, lad.tmp_bytes - 8)
        assert st == abi.PZ_ERR_INVALID and "tmp too small" in msg, (st, msg)
        st, msg = call(lad.d_res.ptr, lad.d_a.ptr, lad.d_res.ptr, lad.tmp_bytes)
        assert st == abi.PZ_ERR_ALIAS and "tmp overlaps" in msg, (st, msg)
        st, msg = call(C.c_void_p(lad.d_a.ptr.value + ct), lad.d_a.ptr, lad.d_tmp.ptr, lad.tmp_bytes)
        assert st == abi.PZ_ERR_ALIAS and "res overlaps a" in msg, (st, msg)
        hip.sync()
        assert np.all(lad.d_res.download(np.uint8, s.a.nbytes) == 0x5A)
        assert np.array_equal(lad.d_a.download(np.int64, s.a.size).reshape(s.a.shape), s.a)


def test_blind_selection_through_the_helper(mods, setups):
    """N = 1024, 8 slots x batch 2, entries 1, 4 and 6 absent: the helper's three calls give the digits of the reference's sparse-map walk
    per batch element, and every result decrypts to entry (k >> 1) mod 8 of its own map (zero where that entry is absent)."""
    from poulpy_amd import bdd
    n, batch, bit_rsh, bit_mask, k_pt = 1024, 2, 1, 3, 6
    s = setups(n)
    rng = seeded(18300)
    slots = 1 << bit_mask
    for absent in ((1, 4, 6), tuple(i for i in range(slots) if i != (s.k >> bit_rsh) & 7)):
        present = [i for i in range(slots) if i not in absent]
        msgs = {(i, b): rng.integers(-30, 30, n, dtype=np.int64) for i in present for b in range(batch)}
        buf = np.zeros((slots, batch, s.size, s.cols, n), dtype=np.int64)
        for (i, b), m in msgs.items():
            buf[i, b] = fhe_sk.glwe_encrypt(s.sk, fhe_sk.encode(m, s.base2k, k_pt, s.size), s.base2k, s.size * s.base2k, rng)
        want = np.empty((batch, s.size, s.cols, n), dtype=np.int64)
        for b in range(batch):
            res = VecZnx(n, s.cols, s.size)
            co.glwe_blind_selection(s.ref, res, {i: VecZnx(n, s.cols, s.size, buf[i, b].copy()) for i in present}, s.get_bit, bit_rsh, bit_mask, s.base2k)
            want[b] = res.data
        with on_device(s.hip, chunk=3) as dev:
            d_keys = [dev.key(ph) for _, ph in s.keys[:bit_rsh + bit_mask]]
            d_buf = dev.upload(buf)
            s.hip.dispatch_notes(reset=True)
            out = bdd.glwe_blind_selection(s.hip, d_buf.ptr, [d_keys[bit_rsh + i].ptr for i in range(bit_mask)], s.p, batch)
            s.hip.sync()
            assert out.value == d_buf.ptr.value + (slots - 1) * batch * want[0].nbytes
            got = d_buf.download(np.int64, buf.size).reshape(buf.shape)[slots - 1]
            notes = s.hip.dispatch_notes()
        assert np.array_equal(got, want), absent
        assert (ONE in notes or TWO in notes) and MAT not in notes, notes
        sel = (s.k >> bit_rsh) & (slots - 1)
        for b in range(batch):
            dec = co.decode_i64(fhe_sk.glwe_phase(got[b], s.sk), s.base2k, k_pt)
            assert np.array_equal(dec, msgs.get((sel, b), np.zeros(n, dtype=np.int64))), (absent, b, sel)
