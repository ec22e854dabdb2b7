"""FheUint words to word in one call: pz_fhe_uint_pack_batched, bit-exact against the oracle's statement of FheUint::pack
(tests/fhe_uint_pack_oracle.py) and against pz_glwe_pack_batched / pz_glwe_pack_bases_batched on both of its routes, with the launch count,
the graph replay and the refusals; pz_fhe_uint_execute_batched against the two public calls in sequence; then words -> adder -> word ->
comparison under real keys, checked by decryption alone.  Uniform random digits everywhere but in the last test."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

from poulpy_amd import bdd
from poulpy_amd.layouts import MatZnx
from tests import fhe_sk as fs
from tests import fhe_uint_cases as fc
from tests import fhe_uint_pack_oracle as po
from tests import unnormalized as un
from tests.cmux_oracle import GRAPHS
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded
from tests.test_gpu_fhe_uint import Key, ggsw_doubles

pytestmark = pytest.mark.gpu

NOTE_LEVELS = "fhe_uint_pack: by levels"
NOTE_PAIRS = "fhe_uint_pack: per pair"


def assert_route(notes, note, label, replayed=False):
    """replayed: a graph launch happened during the call - a replay runs no host code and leaves no note (freed buffers come back at the
    same addresses, so a later test's call can be an earlier one's second or third sighting)"""
    if replayed and "fhe_uint_pack" not in notes:
        return
    assert note in notes, (label, note, notes)
    for other in (NOTE_LEVELS, NOTE_PAIRS):
        if other != note:
            assert other not in notes, (label, other, notes)


@contextmanager
def knob(name, value):
    """a run-time switch of the library (read per call) for the body"""
    os.environ[name] = str(value)
    try:
        yield
    finally:
        os.environ.pop(name)


# name -> (n, rank, limbs, ciphertext base, key base, key limbs, key rows, trace_size).  "ref": rank, bases and precisions of the reference's own
# test of bdd_arithmetic (fhe_uint_cases.REF_SHAPE: words of k = 26 in base 13, keys of k = 52 in base 11 with 4 rows), trace_size =
# ceil(26 / 11).  n2048 / n128: two limbs, to keep the oracle's 63 / 127 merges short.
SHAPES = {
    "n256": (256, 1, 3, 13, 13, 3, 3, 0),
    "ref": (256, 2, 2, 13, 11, 5, 4, 3),
    "n1024": (1024, 1, 3, 13, 13, 3, 3, 0),
    "n2048": (2048, 1, 2, 13, 13, 2, 2, 0),
    "n128": (128, 1, 2, 13, 13, 2, 2, 0),
}
PARITY = [("n256", 8, 1), ("n256", 8, 3), ("n256", 16, 1), ("n256", 16, 3), ("n256", 32, 1), ("n256", 32, 3), ("ref", 8, 2), ("n1024", 32, 2),
          ("n2048", 64, 1), ("n128", 128, 1)]


class Shape:
    """One shape: the log2(n) automorphism keys (uniform digits) prepared for the oracle and the device, once per test file."""

    def __init__(self, name, ref, hip):
        self.name = name
        self.n, self.rank, self.size, self.ct_k, self.key_k, self.key_size, self.dnum, self.trace_size = SHAPES[name]
        self.cols = self.rank + 1
        self.ref, self.hip = ref, hip
        rng = seeded(46000 + sorted(SHAPES).index(name))
        self.gals = [-1] + [pow(5, 1 << i, 2 * self.n) for i in range(self.n.bit_length() - 2)]
        self.keys = [prepared_key(ref, hip, MatZnx(self.n, self.dnum, self.rank, self.cols, self.key_size).fill_uniform(self.key_k, rng)) for _ in self.gals]
        hip.sync()
        self.ct = self.size * self.cols * self.n

    def params(self):
        from poulpy_amd.hal import GlweOpParams
        return GlweOpParams(rank=self.rank, dnum=self.dnum, dsize=1, key_size=self.key_size, key_base2k=self.key_k, a_size=self.size, a_base2k=self.ct_k,
                            res_size=self.size, res_base2k=self.ct_k, rank_out=self.rank)

    def bits(self, word_bits, batch, seed, fill=None):
        """(word_bits, batch, size, cols, n): slot-major, uniform digits; fill(b, data, rng) rewrites ciphertexts (tests/unnormalized.py)"""
        rng = seeded(seed)
        half = 1 << (self.ct_k - 1)
        data = rng.integers(-half, half, (word_bits, batch, self.size, self.cols, self.n), dtype=np.int64)
        for s in range(word_bits if fill is not None else 0):
            for b in range(batch):
                fill(b, data[s, b], rng)
        return data

    def want(self, data, word_bits):
        """the oracle: ref.glwe_pack / glwe_pack_bases with the word's indices, one batch element at a time"""
        batch = data.shape[1]
        keys_r = [pr for pr, _ in self.keys]
        return np.stack([po.pack_word(self.ref, np.ascontiguousarray(data[:, b]), word_bits, self.ct_k, self.gals, keys_r, self.key_k, self.trace_size)
                         for b in range(batch)])

    def device_keys(self, dev):
        return [dev.key(ph).ptr for _, ph in self.keys]

    def general_pack(self, dev, d_res, d_bits, word_bits, batch, key_ptrs):
        """what bdd.fhe_uint_pack does today: pz_glwe_pack_batched / pz_glwe_pack_bases_batched with the word's indices"""
        hip, p = self.hip, self.params()
        lg = po.log_gap(self.n, word_bits)
        cts = [C.c_void_p(d_bits.ptr.value + s * batch * self.ct * 8) for s in range(word_bits)]
        idx = po.word_indices(self.n, word_bits)
        if self.trace_size == 0:
            d_tmp = dev.alloc(hip.glwe_pack_tmp_bytes(p, batch))
            hip.glwe_pack_batched(d_res.ptr, idx, cts, lg, self.gals, key_ptrs, p, d_tmp.ptr, d_tmp.nbytes, batch)
        else:
            d_tmp = dev.alloc(hip.glwe_pack_bases_tmp_bytes(p, self.trace_size, batch))
            hip.glwe_pack_bases_batched(d_res.ptr, idx, cts, lg, self.gals, key_ptrs, p, self.trace_size, d_tmp.ptr, d_tmp.nbytes, batch)
        hip.sync()


@pytest.fixture(scope="module")
def shapes(mods):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Shape(name, *mods(SHAPES[name][0]))
        return cache[name]
    return get


def run_all_three(sh, data, word_bits, label):
    """-> the oracle's words, after asserting that the level route, its per-pair twin and the general pack all give exactly them"""
    hip, p = sh.hip, sh.params()
    batch = data.shape[1]
    want = sh.want(data, word_bits)
    with on_device(hip) as dev:
        keys = sh.device_keys(dev)
        need = hip.fhe_uint_pack_tmp_bytes(p, word_bits, batch, sh.trace_size)
        assert need >= (hip.glwe_pack_bases_tmp_bytes(p, sh.trace_size, batch) if sh.trace_size else hip.glwe_pack_tmp_bytes(p, batch))
        d_tmp = dev.alloc(need)
        got = {}
        for route, note in (("levels", NOTE_LEVELS), ("pairs", NOTE_PAIRS)):
            d_bits, d_res = dev.upload(data), dev.alloc(want.nbytes)
            hip.dispatch_notes(reset=True)
            g0 = hip.graph_launches()
            with knob("POULPY_DBG_PACK_LEVELS", 1 if route == "levels" else 0):
                hip.fhe_uint_pack_batched(d_res.ptr, d_bits.ptr, word_bits, sh.gals, keys, p, d_tmp.ptr, need, batch, sh.trace_size)
                hip.sync()
            assert route == "levels" or hip.graph_launches() == g0, "the per-pair route runs on plain launches"
            assert_route(hip.dispatch_notes(), note, (label, route), replayed=hip.graph_launches() > g0)
            got[route] = d_res.download(np.int64, want.size).reshape(want.shape)
        d_bits, d_res = dev.upload(data), dev.alloc(want.nbytes)
        sh.general_pack(dev, d_res, d_bits, word_bits, batch, keys)
        got["general"] = d_res.download(np.int64, want.size).reshape(want.shape)
    for route, words in got.items():
        assert np.array_equal(words, want), (label, route, "differs from the oracle")
    return want


@pytest.mark.parametrize("name,word_bits,batch", PARITY, ids=lambda v: str(v))
def test_pack_equals_oracle_and_general_pack(shapes, name, word_bits, batch):
    sh = shapes(name)
    data = sh.bits(word_bits, batch, 46100 + word_bits + batch)
    run_all_three(sh, data, word_bits, (name, word_bits, batch))


@pytest.mark.parametrize("fill", [un.sums(13, 3), un.one_wide(1, 13, 9), un.full_range_fill()], ids=lambda f: f.label)
def test_pack_on_unnormalized_limbs(shapes, fill):
    """The wrapping sums and the halving of digits beyond the base are part of the contract: wide digits in every ciphertext, in one input
    of the batch only, and the whole int64 range."""
    sh = shapes("n256")
    data = sh.bits(16, 2, 46200, fill=fill)
    un.check_unnormalized(data, 13)
    run_all_three(sh, data, 16, ("unnormalized", fill.label))


def test_route_and_its_twin(shapes):
    """Every call plain (graphs off), so each leaves its note: by levels by default, per pair under POULPY_DBG_PACK_LEVELS=0, the same bytes."""
    sh = shapes("n1024")
    hip, p, w, batch = sh.hip, sh.params(), 16, 2
    data = sh.bits(w, batch, 46250)
    got = []
    with on_device(hip, graphs=False) as dev:
        keys = sh.device_keys(dev)
        d_tmp = dev.alloc(hip.fhe_uint_pack_tmp_bytes(p, w, batch))
        for value, note in ((None, NOTE_LEVELS), (0, NOTE_PAIRS), (1, NOTE_LEVELS)):
            d_bits, d_res = dev.upload(data), dev.alloc(batch * sh.ct * 8)
            hip.dispatch_notes(reset=True)
            if value is None:
                hip.fhe_uint_pack_batched(d_res.ptr, d_bits.ptr, w, sh.gals, keys, p, d_tmp.ptr, d_tmp.nbytes, batch)
            else:
                with knob("POULPY_DBG_PACK_LEVELS", value):
                    hip.fhe_uint_pack_batched(d_res.ptr, d_bits.ptr, w, sh.gals, keys, p, d_tmp.ptr, d_tmp.nbytes, batch)
            hip.sync()
            assert_route(hip.dispatch_notes(), note, ("knob", value))
            got.append(d_res.download(np.int64, batch * sh.ct))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    assert np.array_equal(got[0].reshape(batch, sh.size, sh.cols, sh.n), sh.want(data, w))


def launches(hip, call):
    hip.set_kernel_timing(True)     # (resets the counters)
    call()
    hip.sync()
    return sum(cnt for cnt, _ in hip.kernel_stats().values())


def test_launch_count_is_per_level_not_per_pair(shapes):
    """A u32 word is 5 levels.  By levels a level is the two new kernels around ONE automorphism call, whatever the batch: at most
    5 * (2 + A) + T launches, A = the launches of one pz_glwe_automorphism_batched on the 16 * batch ciphertexts of the widest level, T = those
    of pz_glwe_trace_batched over the log_gap closing steps - both counted here on the same module.  Per pair a merge alone is more than a
    level: 31 merges of about 17 launches."""
    sh = shapes("n256")
    hip, p, w = sh.hip, sh.params(), 32
    counts = {}
    for batch in (1, 3):
        data = sh.bits(w, batch, 46300 + batch)
        with on_device(hip, timing=True) as dev:
            keys = sh.device_keys(dev)
            d_tmp = dev.alloc(hip.fhe_uint_pack_tmp_bytes(p, w, batch))
            d_res = dev.alloc(batch * sh.ct * 8)
            d_x = dev.upload(data[:16])
            auto = launches(hip, lambda: hip.glwe_automorphism_batched(d_x.ptr, d_x.ptr, keys[0], p, sh.gals[0], "automorphism", 16 * batch))
            trace = launches(hip, lambda: hip.glwe_trace_batched(d_x.ptr, sh.gals[5:], keys[5:], p, batch))
            bound = 5 * (2 + auto) + trace
            d_bits = dev.upload(data)
            by_levels = launches(hip, lambda: hip.fhe_uint_pack_batched(d_res.ptr, d_bits.ptr, w, sh.gals, keys, p, d_tmp.ptr, d_tmp.nbytes, batch))
            d_bits = dev.upload(data)
            with knob("POULPY_DBG_PACK_LEVELS", 0):
                per_pair = launches(hip, lambda: hip.fhe_uint_pack_batched(d_res.ptr, d_bits.ptr, w, sh.gals, keys, p, d_tmp.ptr, d_tmp.nbytes, batch))
        print("[fhe_uint_pack] u32 N=256 batch %d: %d launches by levels (bound %d: automorphism %d, trace %d), %d per pair" % (batch, by_levels, bound, auto, trace, per_pair))
        assert 0 < by_levels <= bound < per_pair, (batch, by_levels, bound, per_pair)
        counts[batch] = by_levels
    assert counts[1] == counts[3], counts


def test_graph_replay_with_new_contents(shapes):
    """Three calls with identical arguments and new contents in the same buffers: each bit-exact; replayed from the second sighting.
    (A batch no other test of this file uses: freed buffers come back at the same addresses, and the same arguments are the same sighting.)"""
    sh = shapes("n256")
    hip, p, w, batch = sh.hip, sh.params(), 8, 4
    with on_device(hip) as dev:
        keys = sh.device_keys(dev)
        d_tmp = dev.alloc(hip.fhe_uint_pack_tmp_bytes(p, w, batch))
        d_bits, d_res = dev.alloc(w * batch * sh.ct * 8), dev.alloc(batch * sh.ct * 8)
        before = hip.graph_launches()
        for k in range(3):
            data = sh.bits(w, batch, 46400 + k)
            d_bits.upload(data)
            hip.lib.pz_memset_d(hip.handle, d_res.ptr, 0x5A, d_res.nbytes)
            hip.fhe_uint_pack_batched(d_res.ptr, d_bits.ptr, w, sh.gals, keys, p, d_tmp.ptr, d_tmp.nbytes, batch)
            hip.sync()
            want = sh.want(data, w)
            assert np.array_equal(d_res.download(np.int64, want.size).reshape(want.shape), want), ("call", k)
            assert hip.graph_launches() - before == (k if GRAPHS else 0), ("call", k)


def test_refusals_launch_nothing(shapes, mods):
    from poulpy_amd import abi
    sh = shapes("n256")
    hip, p, w, batch = sh.hip, sh.params(), 16, 2
    with on_device(hip, timing=True) as dev:
        keys = sh.device_keys(dev)
        need = hip.fhe_uint_pack_tmp_bytes(p, w, batch)
        d_tmp, d_bits, d_res = dev.alloc(need), dev.alloc(w * batch * sh.ct * 8), dev.alloc(batch * sh.ct * 8)
        hip.sync()
        g = (C.c_int64 * len(sh.gals))(*sh.gals)

        def call(mod=hip, res=d_res.ptr, bits=d_bits.ptr, word_bits=w, gals=g, key_ptrs=keys, params=p, trace_size=0, tmp=d_tmp.ptr, tmp_bytes=need, batch=batch):
            kp = (C.c_void_p * len(key_ptrs))(*[None if k is None else k.value for k in key_ptrs])
            st = mod.lib.pz_fhe_uint_pack_batched(mod.handle, res, bits, word_bits, gals, kp, C.byref(params), trace_size, tmp, tmp_bytes, batch)
            return st, mod.lib.pz_last_error().decode()
        hip.set_kernel_timing(True)     # (resets the counters)
        graphs = hip.graph_launches()
        even = (C.c_int64 * len(sh.gals))(*[x if i != 2 else 6 for i, x in enumerate(sh.gals)])
        even_trace = (C.c_int64 * len(sh.gals))(*[x if i != len(sh.gals) - 1 else 4 for i, x in enumerate(sh.gals)])
        from poulpy_amd.hal import GlweOpParams
        mixed = GlweOpParams.from_buffer_copy(p)
        mixed.key_base2k = 11
        inside = lambda buf, off: C.c_void_p(buf.ptr.value + off)   # noqa: E731
        for label, kw, status, msg in (
                ("word_bits 12", dict(word_bits=12), abi.PZ_ERR_INVALID, "word_bits 12"),
                ("word_bits 256", dict(word_bits=256), abi.PZ_ERR_INVALID, "word_bits 256"),
                ("tmp too small", dict(tmp_bytes=need - 1), abi.PZ_ERR_INVALID, "tmp too small"),
                ("null key of a merge", dict(key_ptrs=[None] + keys[1:]), abi.PZ_ERR_INVALID, "trace step 0"),
                ("null key of the trace", dict(key_ptrs=keys[:-1] + [None]), abi.PZ_ERR_INVALID, "trace step %d" % (len(keys) - 1)),
                ("even Galois element of a merge", dict(gals=even), abi.PZ_ERR_INVALID, "trace step 2"),
                ("even Galois element of the trace", dict(gals=even_trace), abi.PZ_ERR_INVALID, "trace step %d" % (len(keys) - 1)),
                ("mixed bases without trace_size", dict(params=mixed), abi.PZ_ERR_INVALID, "trace_size"),
                ("res inside bits", dict(res=inside(d_bits, 3 * batch * sh.ct * 8)), abi.PZ_ERR_ALIAS, "res overlaps bits"),
                ("bits inside tmp", dict(bits=d_tmp.ptr, tmp=d_tmp.ptr, tmp_bytes=need), abi.PZ_ERR_ALIAS, "bits overlaps tmp"),
                ("res inside tmp", dict(res=inside(d_tmp, 256)), abi.PZ_ERR_ALIAS, "res overlaps tmp")):
            st, text = call(**kw)
            assert st == status and msg in text, (label, st, text)
        # n % word_bits != 0 needs a ring smaller than the word: N = 64 with 128-bit words
        _, small = mods(64)
        st, text = call(mod=small, word_bits=128)
        assert st == abi.PZ_ERR_INVALID and "word_bits 128 divides" in text, (st, text)
        st, text = call(batch=0)
        assert st == 0, text
        hip.sync()
        assert all(cnt == 0 for cnt, _ in hip.kernel_stats().values()), hip.kernel_stats()
        assert hip.graph_launches() == graphs
        for buf in (d_res, d_bits, d_tmp):
            assert np.all(buf.download(np.uint8, buf.nbytes) == 0x5A), "a refused call wrote"


# ---- pz_fhe_uint_execute_batched ------------------------------------------------------------------------------------------------------------------
NKEYS = 6


def ggsw_of(b, i, variant=0):
    return (5 * b + 2 * i + 3 * variant + (b * i) % 3) % NKEYS


EXECUTE = [("n256", "adder", 2), ("n256", "ltu", 2), ("n1024", "adder", 2)]


@pytest.mark.parametrize("name,circuit,batch", EXECUTE, ids=lambda v: str(v))
def test_execute_equals_evaluator_then_pack(shapes, name, circuit, batch):
    """adder(8) fills the word, ltu(8) one slot of it (seven zero ciphertexts); N = 1024: the evaluator's gathered route, where a second call
    with a fresh bits array behind the same arguments must pick the new keys up."""
    sh = shapes(name)
    ref, hip, w = sh.ref, sh.hip, 8
    circ = bdd.adder(w) if circuit == "adder" else bdd.ltu(w)
    rng = seeded(46500 + sh.n)
    ggsws = [prepared_key(ref, hip, MatZnx(sh.n, sh.dnum, sh.cols, sh.cols, sh.size).fill_uniform(sh.ct_k, rng))[1] for _ in range(NKEYS)]
    from poulpy_amd.hal import GlweOpParams
    gate = GlweOpParams(rank=sh.rank, dnum=sh.dnum, dsize=1, key_size=sh.size, key_base2k=sh.ct_k, a_size=sh.size, a_base2k=sh.ct_k, res_size=sh.size,
                        res_base2k=sh.ct_k, rank_out=sh.rank)
    pack = sh.params()
    with on_device(hip) as dev:
        atk = sh.device_keys(dev)
        d_ggsw = [dev.key(ph).ptr for ph in ggsws]
        h = hip.bdd_circuit_new(circ)
        try:
            d_out = dev.alloc(w * batch * sh.ct * 8)
            d_etmp = dev.alloc(max(hip.bdd_circuit_execute_tmp_bytes(h, gate, batch), 8))
            d_ptmp = dev.alloc(hip.fhe_uint_pack_tmp_bytes(pack, w, batch))
            need = hip.fhe_uint_execute_tmp_bytes(h, gate, pack, w, batch)
            assert need >= w * batch * sh.ct * 8 + max(d_etmp.nbytes, d_ptmp.nbytes)
            d_tmp = dev.alloc(need)
            d_two, d_one = dev.alloc(batch * sh.ct * 8), dev.alloc(batch * sh.ct * 8)
            for call, variant in enumerate((0, 1, 1)):      # the third call: the same arguments again (the halves' graphs replay where graphs are on)
                bits = [[d_ggsw[ggsw_of(b, i, variant)] for i in range(circ.input_size)] for b in range(batch)]
                hip.bdd_circuit_execute_batched(h, d_out.ptr, w, bits, gate, d_etmp.ptr, d_etmp.nbytes, batch)
                hip.fhe_uint_pack_batched(d_two.ptr, d_out.ptr, w, sh.gals, atk, pack, d_ptmp.ptr, d_ptmp.nbytes, batch)
                hip.sync()
                want = d_two.download(np.int64, batch * sh.ct)
                hip.lib.pz_memset_d(hip.handle, d_one.ptr, 0x5A, d_one.nbytes)
                hip.dispatch_notes(reset=True)
                g0 = hip.graph_launches()
                hip.fhe_uint_execute_batched(h, d_one.ptr, w, bits, gate, sh.gals, atk, pack, d_tmp.ptr, need, batch)
                hip.sync()
                notes = hip.dispatch_notes()
                if hip.graph_launches() == g0:       # both halves on plain launches (a replayed graph leaves no note)
                    assert NOTE_LEVELS in notes and ("bdd: gathered" in notes) == (sh.n == 1024), notes
                assert np.array_equal(d_one.download(np.int64, batch * sh.ct), want), (name, circuit, call)
            assert want.any()
            with on_device(hip, graphs=False):      # the routes, whatever the graph cache held: every call plain
                hip.dispatch_notes(reset=True)
                hip.fhe_uint_execute_batched(h, d_one.ptr, w, bits, gate, sh.gals, atk, pack, d_tmp.ptr, need, batch)
                hip.sync()
                notes = hip.dispatch_notes()
                assert NOTE_LEVELS in notes and ("bdd: gathered" in notes) == (sh.n == 1024), notes
                assert np.array_equal(d_one.download(np.int64, batch * sh.ct), want), (name, circuit, "graphs off")
        finally:
            hip.bdd_circuit_free(h)


def test_execute_refusals_launch_nothing(shapes):
    from poulpy_amd import abi
    from poulpy_amd.hal import GlweOpParams, PoulpyHipError
    sh = shapes("n256")
    hip, w, batch = sh.hip, 8, 2
    rng = seeded(46600)
    ggsw = prepared_key(sh.ref, hip, MatZnx(sh.n, sh.dnum, sh.cols, sh.cols, sh.size).fill_uniform(sh.ct_k, rng))[1]
    gate = GlweOpParams(rank=sh.rank, dnum=sh.dnum, dsize=1, key_size=sh.size, key_base2k=sh.ct_k, a_size=sh.size, a_base2k=sh.ct_k, res_size=sh.size,
                        res_base2k=sh.ct_k, rank_out=sh.rank)
    pack = sh.params()
    with on_device(hip, timing=True) as dev:
        atk = sh.device_keys(dev)
        d_g = dev.key(ggsw).ptr
        wide, ok = hip.bdd_circuit_new(bdd.adder(w, carry_out=True)), hip.bdd_circuit_new(bdd.adder(w))
        try:
            need = hip.fhe_uint_execute_tmp_bytes(ok, gate, pack, w, batch) + hip.fhe_uint_execute_tmp_bytes(wide, gate, pack, w, batch)
            d_tmp, d_res = dev.alloc(need), dev.alloc(batch * sh.ct * 8)
            hip.sync()
            hip.set_kernel_timing(True)
            bits = [[d_g] * (2 * w) for _ in range(batch)]
            short = GlweOpParams.from_buffer_copy(pack)
            short.a_size = short.res_size = sh.size - 1
            for label, handle, pk, msg in (("output_size > word_bits", wide, pack, "output_size 9 > word_bits 8"), ("res_size differs", ok, short, "res_size")):
                with pytest.raises(PoulpyHipError) as e:
                    hip.fhe_uint_execute_batched(handle, d_res.ptr, w, bits, gate, sh.gals, atk, pk, d_tmp.ptr, need, batch)
                assert "[%d]" % abi.PZ_ERR_INVALID in str(e.value) and msg in str(e.value), (label, str(e.value))
            with pytest.raises(PoulpyHipError) as e:     # a refusal of the second half comes before the first half runs
                hip.fhe_uint_execute_batched(ok, d_res.ptr, w, bits, gate, sh.gals, atk[:-1] + [None], pack, d_tmp.ptr, need, batch)
            assert "trace step" in str(e.value)
            hip.sync()
            assert all(cnt == 0 for cnt, _ in hip.kernel_stats().values()), hip.kernel_stats()
            assert np.all(d_res.download(np.uint8, d_res.nbytes) == 0x5A) and np.all(d_tmp.download(np.uint8, need) == 0x5A), "a refused call wrote"
        finally:
            hip.bdd_circuit_free(wide)
            hip.bdd_circuit_free(ok)


# ---- under real keys: words -> adder -> word in one call -> ltu, decryption only ---------------------------------------------------------------
def test_encrypted_u16_addition_in_one_call_then_comparison_decrypts(mods):
    """Two u16 words per batch element through fhe_uint_prepare, then fhe_uint_execute(adder(16)): the word decrypts to (a + b) mod 2^16, and
    read at the un-interleaved indices i << log_gap it does not.  That word is prepared AGAIN and compared with a third word by
    fhe_uint_execute(ltu(16)): bit 0 of the packed word is sum < third, the other fifteen are zero."""
    from poulpy_amd.hal import GlweOpParams
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE, 47000)
    ref, hip = mods(c.n)
    w, batch, cols = 16, 2, c.rank + 1
    pairs = [(40000, 30000), (12345, 321)]
    thirds = [4465, 12665]              # (a + b) mod 2^16 = 4464 < 4465; 12666 > 12665
    size = c.res_size                   # limbs of the evaluator's GLWEs: the GGSWs' own
    gd = ggsw_doubles(c)
    ct = size * cols * c.n
    gate = GlweOpParams(rank=c.rank, dnum=c.res_dnum, dsize=1, key_size=c.res_size, key_base2k=c.res_b, a_size=size, a_base2k=c.res_b,
                        res_size=size, res_base2k=c.res_b, rank_out=c.rank)
    pack = GlweOpParams(rank=c.rank, dnum=c.atk_dnum, dsize=1, key_size=c.atk[0].shape[2], key_base2k=c.atk_b, a_size=size, a_base2k=c.res_b,
                        res_size=size, res_base2k=c.res_b, rank_out=c.rank)
    with on_device(hip) as dev:
        key = Key(dev, ref, hip, c)
        view = key.view(True)
        p_in = fc.prepare_params(c, True, w, 0, w)
        d_tmp = dev.alloc(hip.fhe_uint_prepare_tmp_bytes(p_in, batch))
        tables = []
        for k, values in enumerate(([a for a, _ in pairs], [b for _, b in pairs], thirds)):
            d_w = dev.upload(fc.words_case(c, w, values, 47100 + k))
            d_p = dev.alloc(batch * w * gd * 8)
            tables.append(bdd.fhe_uint_prepare(hip, d_p.ptr, d_w.ptr, view, p_in, batch, tmp=d_tmp))
        bits = [tables[0][b] + tables[1][b] for b in range(batch)]
        atk = [k.ptr for k in key.d_atk]
        d_sum = dev.alloc(batch * ct * 8)
        bdd.fhe_uint_execute(hip, bdd.adder(w), d_sum.ptr, w, bits, gate, c.gals, atk, pack, batch)
        total = d_sum.download(np.int64, batch * ct).reshape(batch, size, cols, c.n)
        plain_index = lambda i, wb, n: i * (n // wb)   # noqa: E731
        for b, (x, y) in enumerate(pairs):
            assert fc.decrypt_word(c, total[b], w) == (x + y) & 0xFFFF, (b, "the packed sum")
            assert fc.decrypt_word(c, total[b], w, index=plain_index) != (x + y) & 0xFFFF, (b, "read at the un-interleaved indices it is still the sum")
        # the result is a word again: its layout is the evaluator's (res_b, `size` limbs)
        p_sum = fc.prepare_params(c, True, w, 0, w)
        p_sum.ks_glwe.a_size, p_sum.ks_glwe.a_base2k = size, c.res_b
        d_ps = dev.alloc(batch * w * gd * 8)
        d_tmp2 = dev.alloc(hip.fhe_uint_prepare_tmp_bytes(p_sum, batch))
        t_sum = bdd.fhe_uint_prepare(hip, d_ps.ptr, d_sum.ptr, view, p_sum, batch, tmp=d_tmp2)
        bits = [t_sum[b] + tables[2][b] for b in range(batch)]
        d_lt = dev.alloc(batch * ct * 8)
        bdd.fhe_uint_execute(hip, bdd.ltu(w), d_lt.ptr, w, bits, gate, c.gals, atk, pack, batch)
        lt = d_lt.download(np.int64, batch * ct).reshape(batch, size, cols, c.n)
        for b, (x, y) in enumerate(pairs):
            assert fc.decrypt_word(c, lt[b], w) == int(((x + y) & 0xFFFF) < thirds[b]), (b, "sum < third")
