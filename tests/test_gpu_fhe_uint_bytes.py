"""The FheUint byte operations on the device: pz_fhe_uint_get_batched / _zero_byte_ / _splice_ / _sext_, bit-exact against the
oracle's literal restatement (tests/fhe_uint_bytes_oracle.py) on both routes - by stages and the reference's order call by call -, on wide
and full-range limbs, in place, past a gridDim.z chunk, with the launch counts, the graph replay and the refusals; then the reference's own
four tests and words -> adder -> word -> sext / splice under real keys, checked by decryption alone.  Uniform random digits and keys in the
parity tests (the operations never look at what a word encrypts); tests/fhe_uint_cases.py wherever something is decrypted."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

from poulpy_amd import abi, bdd
from poulpy_amd.layouts import MatZnx
from tests import fhe_sk as fs
from tests import fhe_uint_bytes_oracle as bo
from tests import fhe_uint_cases as fc
from tests import unnormalized as un
from tests.cmux_oracle import GRAPHS
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu

NOTE_STAGES = "fhe_uint_word: by stages"
NOTE_LITERAL = "fhe_uint_word: literal"
KNOB = "POULPY_DBG_WORD_STAGES"


@contextmanager
def knob(name, value):
    """a run-time switch of the library (read per call) for the body"""
    os.environ[name] = str(value)
    try:
        yield
    finally:
        os.environ.pop(name)


def assert_route(notes, note, label, replayed=False):
    """replayed: a graph launch happened during the call - a replay runs no host code and leaves no note"""
    if replayed and "fhe_uint_word" not in notes:
        return
    assert note in notes, (label, note, notes)
    for other in (NOTE_STAGES, NOTE_LITERAL):
        if other != note:
            assert other not in notes, (label, other, notes)


# name -> (n, rank, limbs, word base, key base, key limbs, key rows, limbs of a word in the keys' base).  "ref": rank, bases and precisions of
# the reference's own test of bdd_arithmetic (fhe_uint_cases.REF_SHAPE), the cross-base route.  n1024: the one-kernel small-ring automorphism.
# n32: with u32 words log_gap = 0 and the byte trace is steps 3..5.
SHAPES = {
    "n256": (256, 1, 3, 13, 13, 3, 3, 0),
    "ref": (256, 2, 2, 13, 11, 5, 4, 3),
    "n1024": (1024, 1, 3, 13, 13, 3, 3, 0),
    "n2048": (2048, 1, 2, 13, 13, 2, 2, 0),
    "n128": (128, 1, 2, 13, 13, 2, 2, 0),
    "n32": (32, 1, 2, 13, 13, 2, 2, 0),
}


class Shape:
    """One shape: the log2(n) automorphism keys (uniform digits) prepared for the oracle and the device, once per test file."""

    def __init__(self, name, ref, hip):
        self.name = name
        self.n, self.rank, self.size, self.ct_k, self.key_k, self.key_size, self.dnum, self.conv_size = SHAPES[name]
        self.cols = self.rank + 1
        self.ref, self.hip = ref, hip
        rng = seeded(49000 + sorted(SHAPES).index(name))
        self.gals = [-1] + [pow(5, 1 << i, 2 * self.n) for i in range(self.n.bit_length() - 2)]
        self.keys = [prepared_key(ref, hip, MatZnx(self.n, self.dnum, self.rank, self.cols, self.key_size).fill_uniform(self.key_k, rng)) for _ in self.gals]
        hip.sync()
        self.ct = self.size * self.cols * self.n

    def params(self):
        from poulpy_amd.hal import GlweOpParams
        a_size = self.size if self.key_k == self.ct_k else self.conv_size
        return GlweOpParams(rank=self.rank, dnum=self.dnum, dsize=1, key_size=self.key_size, key_base2k=self.key_k, a_size=a_size, a_base2k=self.key_k,
                            res_size=self.size, res_base2k=self.ct_k, rank_out=self.rank)

    def words(self, batch, seed, fill=None):
        """(batch, size, cols, n) uniform digits; fill(b, data, rng) rewrites ciphertexts (tests/unnormalized.py)"""
        rng = seeded(seed)
        half = 1 << (self.ct_k - 1)
        data = rng.integers(-half, half, (batch, self.size, self.cols, self.n), dtype=np.int64)
        for b in range(batch if fill is not None else 0):
            fill(b, data[b], rng)
        return data

    def ctx(self, word_bits):
        return bo.Ctx(self.ref, self.n, word_bits, self.ct_k, self.gals, [pr for pr, _ in self.keys], key_base2k=self.key_k, conv_size=self.conv_size)

    def device_keys(self, dev):
        return [dev.key(ph).ptr for _, ph in self.keys]


@pytest.fixture(scope="module")
def shapes(mods):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Shape(name, *mods(SHAPES[name][0]))
        return cache[name]
    return get


# ---- one operation: on the oracle, and on the device --------------------------------------------------------------------------------------------
def oracle(ctx, op, args, a, b=None):
    """-> what the device call of (op, args) on the batches a (and b) must give: get: (nidx, batch, ...); else (batch, ...)"""
    batch = a.shape[0]
    if op == "bits":
        return np.stack([np.stack([bo.get_bit_glwe(ctx, a[x], i) for x in range(batch)]) for i in args])
    if op == "bytes":
        return np.stack([np.stack([bo.get_byte(ctx, a[x], i) for x in range(batch)]) for i in args])
    if op == "zero":
        return np.stack([bo.zero_byte(ctx, a[x], args[0]) for x in range(batch)])
    if op == "splice8":
        return np.stack([bo.splice_u8(ctx, args[0], args[1], a[x], b[x]) for x in range(batch)])
    if op == "splice16":
        return np.stack([bo.splice_u16(ctx, args[0], args[1], a[x], b[x]) for x in range(batch)])
    assert op == "sext"
    return np.stack([bo.sext(ctx, a[x], args[0]) for x in range(batch)])


def call(hip, op, args, word_bits, d_res, d_a, d_b, gals, keys, p, d_tmp, batch):
    """the device call of (op, args); sext runs in place on d_res (d_a is not read)"""
    t, nb = d_tmp.ptr, d_tmp.nbytes
    if op in ("bits", "bytes"):
        hip.fhe_uint_get_batched(d_res.ptr, d_a.ptr, word_bits, abi.PZ_WORD_BIT if op == "bits" else abi.PZ_WORD_BYTE, args, gals, keys, p, t, nb, batch)
    elif op == "zero":
        hip.fhe_uint_zero_byte_batched(d_res.ptr, d_a.ptr, word_bits, args[0], gals, keys, p, t, nb, batch)
    elif op in ("splice8", "splice16"):
        hip.fhe_uint_splice_batched(d_res.ptr, d_a.ptr, d_b.ptr, word_bits, 8 if op == "splice8" else 16, args[0], args[1], gals, keys, p, t, nb, batch)
    else:
        hip.fhe_uint_sext_batched(d_res.ptr, word_bits, args[0], gals, keys, p, t, nb, batch)


def run_both_routes(sh, dev, keys, op, args, word_bits, a, b, label):
    """-> the oracle's result, after asserting that the staged route and its literal twin both give exactly it"""
    hip, p = sh.hip, sh.params()
    batch = a.shape[0]
    want = oracle(sh.ctx(word_bits), op, args, a, b)
    d_tmp = dev.alloc(hip.fhe_uint_word_op_tmp_bytes(p, word_bits, batch, max(len(args), 1)))
    d_a, d_b = dev.upload(a), dev.upload(b if b is not None else a)
    for route, note in (("stages", NOTE_STAGES), ("literal", NOTE_LITERAL)):
        d_res = dev.upload(a) if op == "sext" else dev.alloc(want.nbytes)
        hip.dispatch_notes(reset=True)
        g0 = hip.graph_launches()
        with knob(KNOB, 1 if route == "stages" else 0):
            call(hip, op, args, word_bits, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch)
            hip.sync()
        assert route == "stages" or hip.graph_launches() == g0, "the literal route runs on plain launches"
        assert_route(hip.dispatch_notes(), note, (label, route), replayed=hip.graph_launches() > g0)
        got = d_res.download(np.int64, want.size).reshape(want.shape)
        assert np.array_equal(got, want), (label, op, args, route, "differs from the oracle")
        dev.free(d_res)
    assert np.array_equal(d_a.download(np.int64, a.size).reshape(a.shape), a), (label, op, "a was written")
    for buf in (d_tmp, d_a, d_b):
        dev.free(buf)
    return want


def operations(word_bits, rng):
    """every operation with arguments drawn for this width: a get of a few bits (all of them up to u16) and of all bytes, one zero_byte, one
    splice of each width the word has, sext of the first byte (the most stages) and of one in the middle"""
    nbytes = word_bits // 8
    pick = lambda k: int(rng.integers(0, k))   # noqa: E731
    ops = [("bits", list(range(word_bits)) if word_bits <= 16 else sorted({0, word_bits - 1, 7, 8, pick(word_bits), pick(word_bits)})),
           ("bytes", list(range(nbytes))), ("zero", [pick(nbytes)]), ("splice8", [pick(nbytes), pick(nbytes)])]
    if nbytes >= 2:
        ops += [("splice16", [pick(nbytes // 2), pick(nbytes // 2)]), ("sext", [0])]
    if nbytes >= 4:
        ops.append(("sext", [nbytes // 2]))
    return ops


PARITY = [("n256", 8, 1), ("n256", 8, 3), ("n256", 16, 1), ("n256", 16, 3), ("n256", 32, 1), ("n256", 32, 3), ("ref", 32, 2), ("n1024", 32, 2),
          ("n2048", 64, 1), ("n128", 128, 1), ("n32", 32, 2)]


@pytest.mark.parametrize("name,word_bits,batch", PARITY, ids=lambda v: str(v))
def test_every_operation_equals_the_oracle_on_both_routes(shapes, name, word_bits, batch):
    sh = shapes(name)
    rng = seeded(49100 + word_bits + batch)
    a, b = sh.words(batch, 49200 + word_bits + batch), sh.words(batch, 49300 + word_bits + batch)
    with on_device(sh.hip) as dev:
        keys = sh.device_keys(dev)
        for op, args in operations(word_bits, rng):
            run_both_routes(sh, dev, keys, op, args, word_bits, a, b, (name, word_bits, batch))


@pytest.mark.parametrize("fill", [un.sums(13, 3), un.one_wide(1, 13, 9), un.full_range_fill()], ids=lambda f: f.label)
def test_operations_on_unnormalized_limbs(shapes, fill):
    """The wrapping adds and subs, the rotation's wrapping negation and the trace's shift of digits beyond the base are part of the contract:
    wide digits in every word, in one word of the batch only, and the whole int64 range."""
    sh = shapes("n256")
    a, b = sh.words(2, 49400, fill=fill), sh.words(2, 49401, fill=fill)
    un.check_unnormalized(a, 13)
    with on_device(sh.hip) as dev:
        keys = sh.device_keys(dev)
        for op, args in (("bits", [0, 5, 15]), ("bytes", [1]), ("zero", [1]), ("splice8", [1, 0]), ("splice16", [0, 0]), ("sext", [0])):
            run_both_routes(sh, dev, keys, op, args, 16, a, b, ("unnormalized", fill.label))


def test_unnormalized_output_of_one_splice_feeds_the_next(shapes):
    """A splice returns the reference's un-normalized limbs; the next operation traces exactly those."""
    sh = shapes("n256")
    ctx = sh.ctx(32)
    a, b = sh.words(2, 49500), sh.words(2, 49501)
    with on_device(sh.hip) as dev:
        keys = sh.device_keys(dev)
        first = run_both_routes(sh, dev, keys, "splice8", [2, 1], 32, a, b, "chain 1")
        assert any(np.abs(first[x]).max() >= 1 << 12 for x in range(2)), "the first splice came out normalized: the chain tests nothing"
        second = run_both_routes(sh, dev, keys, "splice16", [0, 1], 32, first, b, "chain 2")
        run_both_routes(sh, dev, keys, "sext", [1], 32, second, None, "chain 3")
    assert np.array_equal(second[0], bo.splice_u16(ctx, 0, 1, bo.splice_u8(ctx, 2, 1, a[0], b[0]), b[0]))


# ---- aliasing and refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n256", "ref"])
def test_in_place_forms_equal_the_oracle(shapes, name):
    """res == a, res == b and a == b, on both routes: every source of a stage is consumed before its closing kernel writes."""
    sh = shapes(name)
    hip, p, w, batch = sh.hip, sh.params(), 32, 2
    ctx = sh.ctx(w)
    a, b = sh.words(batch, 49600), sh.words(batch, 49601)
    with on_device(hip) as dev:
        keys = sh.device_keys(dev)
        d_tmp = dev.alloc(hip.fhe_uint_word_op_tmp_bytes(p, w, batch))
        for value in (1, 0):
            with knob(KNOB, value):
                for op, args in (("zero", [2]), ("splice8", [3, 1]), ("splice16", [1, 0])):
                    for form in ("res==a", "res==b", "a==b"):
                        if op == "zero" and form != "res==a":
                            continue
                        d_a, d_b = dev.upload(a), dev.upload(b)
                        if form == "res==a":
                            d_res, xa, xb = d_a, a, b
                        elif form == "res==b":
                            d_res, xa, xb = d_b, a, b
                        else:
                            d_res, d_b, xa, xb = dev.alloc(a.nbytes), d_a, a, a
                        call(hip, op, args, w, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch)
                        hip.sync()
                        want = oracle(ctx, op, args, xa, xb)
                        assert np.array_equal(d_res.download(np.int64, want.size).reshape(want.shape), want), (name, value, op, form)


def test_refusals_launch_nothing_and_write_nothing(shapes, mods):
    sh = shapes("n256")
    hip, p, w, batch = sh.hip, sh.params(), 32, 2
    from poulpy_amd.hal import GlweOpParams
    with on_device(hip, timing=True) as dev:
        keys = sh.device_keys(dev)
        need = hip.fhe_uint_word_op_tmp_bytes(p, w, batch, 4)
        ctb = batch * sh.ct * 8
        d_tmp, d_a, d_b, d_res = dev.alloc(need), dev.alloc(ctb), dev.alloc(ctb), dev.alloc(4 * ctb)
        hip.sync()
        g = (C.c_int64 * len(sh.gals))(*sh.gals)
        even = (C.c_int64 * len(sh.gals))(*[x if i != 4 else 6 for i, x in enumerate(sh.gals)])
        idx4 = (C.c_uint32 * 4)(0, 1, 2, 3)

        def kp(key_ptrs):
            return (C.c_void_p * len(key_ptrs))(*[None if k is None else k.value for k in key_ptrs])

        def get(mod=hip, res=d_res.ptr, words=d_a.ptr, word_bits=w, unit=abi.PZ_WORD_BYTE, nidx=4, idx=idx4, gals=g, key_ptrs=keys, params=p, tmp=d_tmp.ptr,
                tmp_bytes=need, batch=batch):
            return mod.lib.pz_fhe_uint_get_batched(mod.handle, res, words, word_bits, unit, nidx, idx, gals, kp(key_ptrs), C.byref(params), tmp, tmp_bytes, batch)

        def zero(mod=hip, res=d_res.ptr, a=d_a.ptr, word_bits=w, byte=1, gals=g, key_ptrs=keys, params=p, tmp=d_tmp.ptr, tmp_bytes=need, batch=batch):
            return mod.lib.pz_fhe_uint_zero_byte_batched(mod.handle, res, a, word_bits, byte, gals, kp(key_ptrs), C.byref(params), tmp, tmp_bytes, batch)

        def splice(mod=hip, res=d_res.ptr, a=d_a.ptr, b=d_b.ptr, word_bits=w, width=8, dst=1, src=2, gals=g, key_ptrs=keys, params=p, tmp=d_tmp.ptr,
                   tmp_bytes=need, batch=batch):
            return mod.lib.pz_fhe_uint_splice_batched(mod.handle, res, a, b, word_bits, width, dst, src, gals, kp(key_ptrs), C.byref(params), tmp, tmp_bytes, batch)

        def sext(mod=hip, word=d_res.ptr, word_bits=w, byte=0, gals=g, key_ptrs=keys, params=p, tmp=d_tmp.ptr, tmp_bytes=need, batch=batch):
            return mod.lib.pz_fhe_uint_sext_batched(mod.handle, word, word_bits, byte, gals, kp(key_ptrs), C.byref(params), tmp, tmp_bytes, batch)
        hip.set_kernel_timing(True)     # (resets the counters)
        graphs = hip.graph_launches()
        mixed = GlweOpParams.from_buffer_copy(p)
        mixed.key_base2k = 11
        inside = lambda buf, off: C.c_void_p(buf.ptr.value + off)   # noqa: E731
        bad_idx = (C.c_uint32 * 4)(0, 1, 2, 4)
        bad_bit = (C.c_uint32 * 4)(0, 1, 2, 32)
        inv, alias = abi.PZ_ERR_INVALID, abi.PZ_ERR_ALIAS
        for label, fn, kw, status, msg in (
                ("word_bits 12", zero, dict(word_bits=12), inv, "word_bits 12"),
                ("word_bits 256", splice, dict(word_bits=256), inv, "word_bits 256"),
                ("word_bits 24 (get)", get, dict(word_bits=24), inv, "word_bits 24"),
                ("word_bits 0 (sext)", sext, dict(word_bits=0), inv, "word_bits 0"),
                ("byte 4 of a u32 (zero_byte)", zero, dict(byte=4), inv, "byte 4"),
                ("byte 4 of a u32 (sext)", sext, dict(byte=4), inv, "byte 4"),
                ("byte 4 of a u32 (get)", get, dict(idx=bad_idx), inv, "byte 4"),
                ("bit 32 of a u32 (get)", get, dict(idx=bad_bit, unit=abi.PZ_WORD_BIT), inv, "bit 32"),
                ("unit 2", get, dict(unit=2), inv, "unit 2"),
                ("dst 4", splice, dict(dst=4), inv, "dst 4"),
                ("src 4", splice, dict(src=4), inv, "src 4"),
                ("u16 dst 2", splice, dict(width=16, dst=2, src=0), inv, "u16 dst 2"),
                ("u16 src 2", splice, dict(width=16, dst=0, src=2), inv, "src 2"),
                ("width 32", splice, dict(width=32), inv, "width 32"),
                ("tmp too small", splice, dict(tmp_bytes=need - 1), inv, "tmp too small"),
                ("tmp too small (get)", get, dict(tmp_bytes=need - 1), inv, "tmp too small"),
                ("null key of a skipped step", zero, dict(key_ptrs=[None] + keys[1:]), inv, "trace step 0"),
                ("null key of the last step", sext, dict(key_ptrs=keys[:-1] + [None]), inv, "trace step %d" % (len(keys) - 1)),
                ("even Galois element", splice, dict(gals=even), inv, "trace step 4"),
                ("even Galois element (get)", get, dict(gals=even), inv, "trace step 4"),
                ("mixed bases, a_size of the word's base", zero, dict(params=mixed), inv, "keys' base"),
                ("a get into its words", get, dict(res=d_a.ptr, nidx=1), alias, "res overlaps a"),
                ("a get over its words", get, dict(words=inside(d_res, 2 * ctb)), alias, "res overlaps a"),
                ("res half over a", zero, dict(res=inside(d_a, sh.ct * 8)), alias, "res overlaps a"),
                ("res half over b", splice, dict(res=inside(d_b, sh.ct * 8)), alias, "res overlaps b"),
                ("a half over b", splice, dict(a=inside(d_b, sh.ct * 8)), alias, "overlaps"),
                ("res inside tmp", zero, dict(res=inside(d_tmp, 256)), alias, "res overlaps tmp"),
                ("a inside tmp", splice, dict(a=d_tmp.ptr), alias, "a overlaps tmp"),
                ("b inside tmp", splice, dict(b=inside(d_tmp, 512)), alias, "b overlaps tmp"),
                ("the word inside tmp", sext, dict(word=d_tmp.ptr), alias, "overlaps tmp")):
            st = fn(**kw)
            text = hip.lib.pz_last_error().decode()
            assert st == status and msg in text, (label, st, text)
        # n % word_bits != 0 needs a ring smaller than the word: N = 64 with 128-bit words
        _, small = mods(64)
        small_g = (C.c_int64 * 6)(*([-1] + [pow(5, 1 << i, 128) for i in range(5)]))
        st = zero(mod=small, word_bits=128, gals=small_g, key_ptrs=keys[:6])
        assert st == inv and "word_bits 128 divides" in small.lib.pz_last_error().decode(), st
        # nothing to do: PZ_OK, nothing launched - no ciphertext, no index, and the sign extension from the last byte
        assert zero(batch=0) == 0 and splice(batch=0) == 0 and get(batch=0) == 0 and sext(batch=0) == 0
        assert get(nidx=0) == 0
        assert sext(byte=3) == 0
        hip.sync()
        assert all(cnt == 0 for cnt, _ in hip.kernel_stats().values()), hip.kernel_stats()
        assert hip.graph_launches() == graphs
        for buf in (d_res, d_a, d_b, d_tmp):
            assert np.all(buf.download(np.uint8, buf.nbytes) == 0x5A), "a refused call wrote"


# ---- chunking -----------------------------------------------------------------------------------------------------------------------------------
def test_get_of_every_bit_past_a_grid_chunk(shapes):
    """All 128 bits of 513 u128 words at N = 128: 65 664 items, one past a gridDim.z chunk of the pre-kernel (and 129 past the second chunk of
    nothing: the last launch is short).  The two routes byte-equal; 64 sampled items equal to the oracle."""
    sh = shapes("n128")
    hip, p, w, batch = sh.hip, sh.params(), 128, 513
    ctx = sh.ctx(w)
    a = sh.words(batch, 49700)
    rng = seeded(49701)
    with on_device(hip) as dev:
        keys = sh.device_keys(dev)
        d_tmp = dev.alloc(hip.fhe_uint_word_op_tmp_bytes(p, w, batch, w))
        d_a = dev.upload(a)
        got = []
        for value in (1, 0):
            d_res = dev.alloc(w * batch * sh.ct * 8)
            with knob(KNOB, value):
                hip.fhe_uint_get_batched(d_res.ptr, d_a.ptr, w, abi.PZ_WORD_BIT, list(range(w)), sh.gals, keys, p, d_tmp.ptr, d_tmp.nbytes, batch)
                hip.sync()
            got.append(d_res.download(np.int64, w * batch * sh.ct).reshape(w, batch, sh.size, sh.cols, sh.n))
            dev.free(d_res)
    assert np.array_equal(got[0], got[1]), "the staged route differs from the literal one"
    samples = [(127, 512), (0, 0), (127, 0), (0, 512)] + [(int(rng.integers(0, w)), int(rng.integers(0, batch))) for _ in range(60)]
    for i, x in samples:
        assert np.array_equal(got[0][i, x], bo.get_bit_glwe(ctx, a[x], i)), (i, x)


# ---- launch counts ------------------------------------------------------------------------------------------------------------------------------
def stats(hip, run):
    """-> (all launches, those of the normalize class - where k_rsh_assign is counted) of one call"""
    hip.set_kernel_timing(True)     # (resets the counters)
    run()
    hip.sync()
    st = hip.kernel_stats()
    return sum(cnt for cnt, _ in st.values()), st["normalize"][0]


def test_launch_counts_are_per_stage_not_per_trace(shapes):
    """u32 words at N = 256, one base.  T0 / T3 = the launches of pz_glwe_trace_batched over all steps / over the steps from 3, counted here on
    the same module.  By stages a splice_u8 is ONE trace's worth of automorphism calls between two kernels and without the trace's first
    k_rsh_assign - T3 + 1 launches where the literal order runs 2 T3 + 7 (two traces, four rotations, a copy, a sub, an add); splice_u16 is
    two (the reference: four), sext(0) one full trace and three byte traces (the reference: seven traces).  The same at batch 1 and 3."""
    sh = shapes("n256")
    hip, p, w = sh.hip, sh.params(), 32
    counts = {}
    for batch in (1, 3):
        a, b = sh.words(batch, 49800 + batch), sh.words(batch, 49810 + batch)
        with on_device(hip, timing=True) as dev:
            keys = sh.device_keys(dev)
            d_tmp = dev.alloc(hip.fhe_uint_word_op_tmp_bytes(p, w, batch, 32))
            d_a, d_b, d_res, d_x = dev.upload(a), dev.upload(b), dev.alloc(32 * a.nbytes), dev.upload(np.tile(a, (32, 1, 1, 1)))
            t0, n0 = stats(hip, lambda: hip.glwe_trace_batched(d_x.ptr, sh.gals, keys, p, 32 * batch))
            assert (t0, n0) == stats(hip, lambda: hip.glwe_trace_batched(d_x.ptr, sh.gals, keys, p, batch)), "the trace's launches depend on the batch"
            t3, n3 = stats(hip, lambda: hip.glwe_trace_batched(d_x.ptr, sh.gals[3:], keys[3:], p, 2 * batch))
            assert n0 >= 1 and n3 >= 1, "the trace's first shift is no launch of the normalize class here: the counts below test nothing"
            got = {}
            for op, args in (("bits", list(range(32))), ("splice8", [1, 2]), ("splice16", [1, 0]), ("sext", [0])):
                for value in (1, 0):
                    if op == "sext":
                        d_res.upload(a)
                    with knob(KNOB, value):
                        got[op, value] = stats(hip, lambda: call(hip, op, args, w, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch))
        print("[fhe_uint_word] u32 N=256 batch %d: trace %d / %d launches (normalize class %d / %d); (all, normalize) by stages | literal: %s"
              % (batch, t0, t3, n0, n3, ", ".join("%s %s | %s" % (op, got[op, 1], got[op, 0]) for op in ("bits", "splice8", "splice16", "sext"))))
        # by stages: pre + trace without its first shift (+ the closing kernel); sext's first stage closes with the replicate
        assert got["bits", 1] == (1 + t0 - 1, n0 - 1)
        assert got["splice8", 1] == (1 + t3 - 1 + 1, n3 - 1)
        assert got["splice16", 1] == (2 * (t3 + 1), 2 * (n3 - 1))
        assert got["sext", 1] == ((t0 + 1) + 3 * (t3 + 1), (n0 - 1) + 3 * (n3 - 1))
        # the literal order: one rotation + one trace per bit; splice_u8 = 2 traces + 4 rotations + copy, sub, add; sext = rotation + trace +
        # 3 x (rotation + add) + 3 splices
        assert got["bits", 0] == (32 * (1 + t0), 32 * n0)
        assert got["splice8", 0] == (2 * t3 + 7, 2 * n3)
        assert got["splice16", 0] == (2 * (2 * t3 + 7), 4 * n3)
        assert got["sext", 0] == (1 + t0 + 6 + 3 * (2 * t3 + 7), n0 + 6 * n3)
        counts[batch] = got
    assert counts[1] == counts[3], counts


# ---- routes and graph replay --------------------------------------------------------------------------------------------------------------------
def test_route_and_its_twin(shapes):
    """Every call plain (graphs off), so each leaves its note: by stages by default, literal under POULPY_DBG_WORD_STAGES=0, the same bytes."""
    sh = shapes("n1024")
    hip, p, w, batch = sh.hip, sh.params(), 32, 2
    a, b = sh.words(batch, 49900), sh.words(batch, 49901)
    got = []
    with on_device(hip, graphs=False) as dev:
        keys = sh.device_keys(dev)
        d_tmp = dev.alloc(hip.fhe_uint_word_op_tmp_bytes(p, w, batch))
        d_a, d_b = dev.upload(a), dev.upload(b)
        for value, note in ((None, NOTE_STAGES), (0, NOTE_LITERAL), (1, NOTE_STAGES)):
            d_res = dev.alloc(a.nbytes)
            hip.dispatch_notes(reset=True)
            if value is None:
                call(hip, "splice16", [1, 0], w, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch)
            else:
                with knob(KNOB, value):
                    call(hip, "splice16", [1, 0], w, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch)
            hip.sync()
            assert_route(hip.dispatch_notes(), note, ("knob", value))
            got.append(d_res.download(np.int64, a.size))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    assert np.array_equal(got[0].reshape(a.shape), oracle(sh.ctx(w), "splice16", [1, 0], a, b))


def test_graph_replay_with_new_contents_and_a_changed_index(shapes):
    """Three calls with identical arguments and new contents in the same buffers: each bit-exact, replayed from the second sighting.  Another
    byte behind the same pointers is another graph: it is captured anew, and computes the other byte.  (A batch no other test of this file
    uses: freed buffers come back at the same addresses, and the same arguments are the same sighting.)"""
    sh = shapes("n256")
    hip, p, w, batch = sh.hip, sh.params(), 32, 5
    ctx = sh.ctx(w)
    with on_device(hip) as dev:
        keys = sh.device_keys(dev)
        d_tmp = dev.alloc(hip.fhe_uint_word_op_tmp_bytes(p, w, batch))
        d_a, d_b, d_res = dev.alloc(batch * sh.ct * 8), dev.alloc(batch * sh.ct * 8), dev.alloc(batch * sh.ct * 8)
        for op, args, other in (("splice8", [3, 0], [2, 0]), ("sext", [1], [2]), ("bytes", [2], [3])):
            before = hip.graph_launches()
            for k in range(3):
                a, b = sh.words(batch, 50000 + k), sh.words(batch, 50010 + k)
                d_a.upload(a)
                d_b.upload(b)
                if op == "sext":
                    d_res.upload(a)
                else:
                    hip.lib.pz_memset_d(hip.handle, d_res.ptr, 0x5A, d_res.nbytes)
                call(hip, op, args, w, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch)
                hip.sync()
                want = oracle(ctx, op, args, a, b)
                assert np.array_equal(d_res.download(np.int64, want.size).reshape(want.shape), want), (op, "call", k)
                assert hip.graph_launches() - before == (k if GRAPHS else 0), (op, "call", k)
            if op == "sext":
                d_res.upload(a)
            call(hip, op, other, w, d_res, d_a, d_b, sh.gals, keys, p, d_tmp, batch)
            hip.sync()
            assert hip.graph_launches() - before == (2 if GRAPHS else 0), (op, "a changed index replayed the old graph")
            want = oracle(ctx, op, other, a, b)
            assert np.array_equal(d_res.download(np.int64, want.size).reshape(want.shape), want), (op, "changed index")


# ---- under real keys, by decryption alone -------------------------------------------------------------------------------------------------------
class RealKeys:
    """The automorphism keys of a fhe_uint_cases key case on the device (the byte operations use no other key)."""

    def __init__(self, dev, hip, c):
        from tests import lwe_cases as lc
        self.c = c
        self.atk = [dev.key(lc.prepare(hip, k)).ptr for k in c.atk]
        self.size, self.cols = c.word_size, c.rank + 1
        self.ct = self.size * self.cols * c.n

    def params(self, size=None, base2k=None):
        from poulpy_amd.hal import GlweOpParams
        c = self.c
        size, base2k = size or c.word_size, base2k or c.word_b
        a_size = size if c.atk_b == base2k else fs.limbs_for(size * base2k, c.atk_b)
        return GlweOpParams(rank=c.rank, dnum=c.atk_dnum, dsize=1, key_size=c.atk[0].shape[2], key_base2k=c.atk_b, a_size=a_size, a_base2k=c.atk_b,
                            res_size=size, res_base2k=base2k, rank_out=c.rank)


A32, B32 = 0xFFFFFFFF, 0xAABBCCDD


@pytest.mark.parametrize("shape", ["one_base", "ref"])
def test_reference_splice_tests_decrypt(mods, shape):
    """test_fhe_uint_splice_u8 / _splice_u16 (bdd_arithmetic/tests/test_suite/fheuint.rs:88-205) with their values: every (dst, src) in one
    batch per width, then the two controls - the same call on words encrypted at the un-interleaved coefficients, and src off by one."""
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE if shape == "one_base" else fc.REF_SHAPE, 50100)
    _, hip = mods(c.n)
    with on_device(hip) as dev:
        rk = RealKeys(dev, hip, c)
        p = rk.params()
        a, b = fc.words_case(c, 32, [A32, B32], 50101)
        d_a, d_b, d_res = dev.upload(a[None]), dev.upload(b[None]), dev.alloc(rk.ct * 8)
        for width, count in ((8, 4), (16, 2)):
            for dst in range(count):
                for src in range(count):
                    bdd.fhe_uint_splice(hip, d_res.ptr, d_a.ptr, d_b.ptr, 32, width, dst, src, c.gals, rk.atk, p, 1)
                    got = d_res.download(np.int64, rk.ct).reshape(a.shape)
                    assert fc.decrypt_word(c, got, 32) == bo.want_splice(A32, B32, dst, src, width), (width, dst, src)
        want = bo.want_splice(A32, B32, 1, 2, 8)
        bdd.fhe_uint_splice(hip, d_res.ptr, d_a.ptr, d_b.ptr, 32, 8, 1, 3, c.gals, rk.atk, p, 1)
        assert fc.decrypt_word(c, d_res.download(np.int64, rk.ct).reshape(a.shape), 32) != want, "src off by one decrypted to the value"
        plain_index = lambda i, wb, n: i * (n // wb)   # noqa: E731
        pa, pb = fc.words_case(c, 32, [A32, B32], 50102, index=plain_index)
        d_pa, d_pb = dev.upload(pa[None]), dev.upload(pb[None])
        bdd.fhe_uint_splice(hip, d_res.ptr, d_pa.ptr, d_pb.ptr, 32, 8, 1, 2, c.gals, rk.atk, p, 1)
        got = d_res.download(np.int64, rk.ct).reshape(a.shape)
        assert fc.decrypt_word(c, got, 32, index=plain_index) != want, "words at the un-interleaved coefficients spliced to the value"


@pytest.mark.parametrize("shape", ["one_base", "ref"])
def test_reference_sext_and_get_bit_tests_decrypt(mods, shape):
    """test_fhe_uint_sext (:20-80): sext(j), j = 0..2, of 0x84838281 and 0x44434241 - the six cases as one batch per j.
    test_fhe_uint_get_bit_glwe (:207-250): every bit of a word in one call, each the constant coefficient of its GLWE; every byte alike."""
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE if shape == "one_base" else fc.REF_SHAPE, 50200)
    _, hip = mods(c.n)
    values = [0x84838281, 0x44434241]
    with on_device(hip) as dev:
        rk = RealKeys(dev, hip, c)
        p = rk.params()
        words = fc.words_case(c, 32, values, 50201)
        d_w = dev.alloc(words.nbytes)
        for j in range(4):
            d_w.upload(words)
            bdd.fhe_uint_sext(hip, d_w.ptr, 32, j, c.gals, rk.atk, p, 2)
            got = d_w.download(np.int64, words.size).reshape(words.shape)
            for x, v in enumerate(values):
                assert fc.decrypt_word(c, got[x], 32) == (bo.want_sext(v, 8 * (j + 1) - 1) if j < 3 else v), (hex(v), j)
        d_w.upload(words)
        d_bits = dev.alloc(32 * words.nbytes)
        bdd.fhe_uint_get_bits(hip, d_bits.ptr, d_w.ptr, 32, list(range(32)), c.gals, rk.atk, p, 2)
        bits = d_bits.download(np.int64, 32 * words.size).reshape((32,) + words.shape)
        d_bytes = dev.alloc(4 * words.nbytes)
        bdd.fhe_uint_get_bytes(hip, d_bytes.ptr, d_w.ptr, 32, list(range(4)), c.gals, rk.atk, p, 2)
        by = d_bytes.download(np.int64, 4 * words.size).reshape((4,) + words.shape)
        d_z = dev.alloc(words.nbytes)
        bdd.fhe_uint_zero_byte(hip, d_z.ptr, d_w.ptr, 32, 2, c.gals, rk.atk, p, 2)
        z = d_z.download(np.int64, words.size).reshape(words.shape)
    for x, v in enumerate(values):
        for i in range(32):
            pt = fs.normalize(fs.glwe_phase(bits[i, x], c.sk_glwe), c.word_b)
            assert fs.decode_coeff(pt, c.word_b, 2, 0) & 1 == (v >> i) & 1, (hex(v), i)
        for j in range(4):
            assert fc.decrypt_word(c, by[j, x], 32) == (v >> (8 * j)) & 0xFF, (hex(v), j)
        assert fc.decrypt_word(c, z[x], 32) == v & 0xFF00FFFF, hex(v)


def test_encrypted_u16_sum_then_sext_and_splice_decrypts(mods):
    """Two u16 words per batch element through fhe_uint_prepare and fhe_uint_execute(adder(16)); the sum - a word in the evaluator's layout -
    is then sign-extended from its low byte, and its high byte is spliced into the low byte of another word: both decrypt to what the
    integers give."""
    from poulpy_amd.hal import GlweOpParams
    from tests.test_gpu_fhe_uint import Key, ggsw_doubles
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE, 50300)
    ref, hip = mods(c.n)
    w, batch, cols = 16, 2, c.rank + 1
    pairs = [(40000, 30128), (12345, 500)]      # sums 0x11F0 (the low byte's sign bit set) and 0x322D (clear)
    others = [0xBEEF, 0x1234]
    size = c.res_size
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
        for k, values in enumerate(([x for x, _ in pairs], [y for _, y in pairs])):
            d_w = dev.upload(fc.words_case(c, w, values, 50310 + k))
            d_p = dev.alloc(batch * w * gd * 8)
            tables.append(bdd.fhe_uint_prepare(hip, d_p.ptr, d_w.ptr, view, p_in, batch, tmp=d_tmp))
        bits = [tables[0][x] + tables[1][x] for x in range(batch)]
        atk = [k.ptr for k in key.d_atk]
        d_sum = dev.alloc(batch * ct * 8)
        bdd.fhe_uint_execute(hip, bdd.adder(w), d_sum.ptr, w, bits, gate, c.gals, atk, pack, batch)
        sums = [(x + y) & 0xFFFF for x, y in pairs]
        total = d_sum.download(np.int64, batch * ct).reshape(batch, size, cols, c.n)
        # the other words, in the sum's layout (size limbs; the encryption's own limbs first, zeros behind)
        enc = fc.words_case(c, w, others, 50320)
        other = np.zeros((batch, size, cols, c.n), dtype=np.int64)
        other[:, :enc.shape[1]] = enc
        d_o, d_res = dev.upload(other), dev.alloc(batch * ct * 8)
        bdd.fhe_uint_splice(hip, d_res.ptr, d_o.ptr, d_sum.ptr, w, 8, 0, 1, c.gals, atk, pack, batch)
        spliced = d_res.download(np.int64, batch * ct).reshape(total.shape)
        bdd.fhe_uint_sext(hip, d_sum.ptr, w, 0, c.gals, atk, pack, batch)
        extended = d_sum.download(np.int64, batch * ct).reshape(total.shape)
    for x in range(batch):
        assert fc.decrypt_word(c, total[x], w) == sums[x], (x, "the packed sum")
        assert fc.decrypt_word(c, spliced[x], w) == (others[x] & 0xFF00) | (sums[x] >> 8), (x, "high byte of the sum into the low byte of the other word")
        assert fc.decrypt_word(c, extended[x], w) == bo.want_sext(sums[x], 7, 16), (x, "the sum sign-extended from its low byte")
    assert bo.want_sext(sums[0], 7, 16) >> 8 == 0xFF and bo.want_sext(sums[1], 7, 16) >> 8 == 0, "one sum of each sign"
