"""FheUint words to prepared GGSW selectors on the device: pz_lwe_from_glwe_many_batched, pz_ggsw_prepare_batched and
pz_fhe_uint_prepare_batched, bit-exact against the existing single calls and the oracle's restatement of FheUintPrepared::prepare
(tests/fhe_uint_oracle.py); then words -> adder -> word -> comparison under real keys, checked by decryption alone."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

from poulpy_amd import bdd
from poulpy_amd.layouts import MatZnx
from tests import fhe_sk as fs
from tests import fhe_uint_cases as fc
from tests import fhe_uint_oracle as fo
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu

NOTE_MATERIALISED = "lwe_from_glwe_many: materialised rotation"
NOTE_ON_LOAD = "lwe_from_glwe_many: rotation on load"


def assert_route(notes, note, label):
    assert note in notes, (label, note, notes)
    for other in (NOTE_MATERIALISED, NOTE_ON_LOAD):
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


# ---- pz_lwe_from_glwe_many_batched ------------------------------------------------------------------------------------------------------------
# (n, rank, GLWE base, key base, LWE base, GLWE limbs, LWE limbs, route): both ring degrees, ranks 1 and 2, one base and 13 -> 4 (where
# mod_switch_2n appends limbs).  N = 256 has no small-ring kernels and 13 -> 4 is read first by a cross-base pass: materialised; N = 1024 with
# every object in the key's base: the rotation on load.
MANY_SHAPES = [(256, 1, 12, 12, 12, 3, 3, NOTE_MATERIALISED), (256, 2, 13, 4, 4, 2, 4, NOTE_MATERIALISED), (1024, 1, 12, 12, 12, 3, 3, NOTE_ON_LOAD),
               (1024, 2, 12, 12, 12, 3, 3, NOTE_ON_LOAD), (1024, 2, 13, 4, 4, 2, 4, NOTE_MATERIALISED)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("shape", MANY_SHAPES, ids=lambda s: "n%d-rank%d-b%d-%d-%d" % s[:5])
def test_many_equals_single_calls(mods, shape, batch):
    """Index-major LWEs = one pz_lwe_from_glwe_batched per index; the vectors of the fused tail = pz_lwe_sample_extract_batched's LWEs
    through pz_lwe_mod_switch_2n_batched, Left and Right; with and without the LWE limbs written."""
    from poulpy_amd.hal import GlweOpParams
    n, rank, a_b, key_b, lwe_b, a_size, lwe_size, route = shape
    ref, hip = mods(n)
    rng = seeded(41000 + n + rank + batch)
    n_lwe, dnum = 33, 3
    key_size = -(-a_size * a_b // key_b) + 1
    idx = [0, 1, n - 1, 5, 1, n // 2]          # 0, both ends, a repeated index
    _, ph = prepared_key(ref, hip, MatZnx(n, dnum, rank, 2, key_size).fill_uniform(key_b, rng))
    a = rng.integers(-(1 << (a_b - 1)), 1 << (a_b - 1), (batch, a_size, rank + 1, n), dtype=np.int64)
    p = GlweOpParams(rank=rank, dnum=dnum, dsize=1, key_size=key_size, key_base2k=key_b, a_size=a_size, a_base2k=a_b, res_size=lwe_size,
                     res_base2k=lwe_b, rank_out=1)
    lwe_len, n2 = lwe_size * (n_lwe + 1), 2 * n
    with on_device(hip) as dev:
        d_a, d_k = dev.upload(a), dev.key(ph)
        want = np.empty((len(idx), batch, lwe_size, n_lwe + 1), dtype=np.int64)
        want_2n = {neg: np.empty((len(idx), batch, n_lwe + 1), dtype=np.int64) for neg in (False, True)}
        d_one, d_one2 = dev.alloc(batch * lwe_len * 8), dev.alloc(batch * (n_lwe + 1) * 8)
        for j, i in enumerate(idx):
            hip.lwe_from_glwe_batched(d_one.ptr, n_lwe, d_a.ptr, i, d_k.ptr, p, batch)
            want[j] = d_one.download(np.int64, batch * lwe_len).reshape(want[j].shape)
            for neg in (False, True):
                hip.lwe_mod_switch_2n_batched(d_one2.ptr, d_one.ptr, n_lwe, lwe_size, lwe_b, n2, neg, batch)
                want_2n[neg][j] = d_one2.download(np.int64, batch * (n_lwe + 1)).reshape(want_2n[neg][j].shape)
        need = hip.lwe_from_glwe_many_tmp_bytes(p, len(idx), batch)
        assert need > 0
        d_tmp = dev.alloc(need)
        for neg, with_lwe in ((False, True), (True, True), (True, False)):
            d_r, d_2n = dev.alloc(want.nbytes), dev.alloc(want_2n[neg].nbytes)
            hip.dispatch_notes(reset=True)
            hip.lwe_from_glwe_many_batched(d_r.ptr if with_lwe else None, n_lwe, d_a.ptr, idx, d_k.ptr, p, d_tmp.ptr, need, batch,
                                           lwe_2n=d_2n.ptr, n2=n2, negate=neg)
            hip.sync()
            notes = hip.dispatch_notes()
            assert_route(notes, route, (shape, batch))
            got_2n = d_2n.download(np.int64, want_2n[neg].size).reshape(want_2n[neg].shape)
            assert np.array_equal(got_2n, want_2n[neg]), (shape, batch, neg, "mod-switched vectors")
            raw = d_r.download(np.uint8, want.nbytes)
            if with_lwe:
                assert np.array_equal(raw.view(np.int64).reshape(want.shape), want), (shape, batch, "LWE limbs")
            else:
                assert np.all(raw == 0x5A), "the LWE limbs were written although no pointer was given"
        # without the mod switch
        d_r = dev.alloc(want.nbytes)
        hip.lwe_from_glwe_many_batched(d_r.ptr, n_lwe, d_a.ptr, idx, d_k.ptr, p, d_tmp.ptr, need, batch)
        hip.sync()
        assert np.array_equal(d_r.download(np.int64, want.size).reshape(want.shape), want)
        if route == NOTE_ON_LOAD:      # the same shape sent down the materialised route: the same bits
            d_r2 = dev.alloc(want.nbytes)
            hip.dispatch_notes(reset=True)
            with knob("POULPY_DBG_LWE_ROT_ON_LOAD", 0):
                hip.lwe_from_glwe_many_batched(d_r2.ptr, n_lwe, d_a.ptr, idx, d_k.ptr, p, d_tmp.ptr, need, batch)
                hip.sync()
            assert_route(hip.dispatch_notes(), NOTE_MATERIALISED, (shape, batch, "knob"))
            assert np.array_equal(d_r2.download(np.int64, want.size).reshape(want.shape), want)
        assert np.array_equal(d_a.download(np.int64, a.size).reshape(a.shape), a), "the source was written"


# ---- pz_ggsw_prepare_batched ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank,dnum,size,count", [(256, 1, 2, 3, 1), (256, 2, 2, 3, 3), (1024, 1, 3, 3, 3), (256, 2, 2, 3, 6), (1024, 2, 3, 3, 4)])
def test_ggsw_prepare_equals_vmp_prepare_as_bytes(mods, n, rank, dnum, size, count):
    """(256, 2, 2, 3, 6): 6 x 54 polynomials, (1024, 2, 3, 3, 4): 4 x 81 - both beyond the 256 of one pz_vmp_prepare launch group."""
    _, hip = mods(n)
    rng = seeded(42000 + n + rank + count)
    cols = rank + 1
    mats = [MatZnx(n, dnum, cols, cols, size).fill_uniform(13, rng) for _ in range(count)]
    want = []
    for m in mats:
        ph = hip.vmp_pmat_alloc(dnum, cols, cols, size)
        hip.vmp_prepare(ph, m)
        want.append(ph.data.reshape(-1).view(np.uint8).copy())
    want = np.concatenate(want)
    with on_device(hip) as dev:
        d_g = dev.upload(np.stack([m.data for m in mats]))
        d_p = dev.alloc(want.nbytes)
        hip.ggsw_prepare_batched(d_p.ptr, d_g.ptr, count, dnum, rank, size)
        hip.sync()
        assert np.array_equal(d_p.download(np.uint8, want.nbytes), want)
        # once per workspace chunk: 7 polynomials of pass-1 scratch, so the one row of all matrices goes in ranges of 7 (the last one short)
        d_q = dev.alloc(want.nbytes)
        with knob("POULPY_DBG_PREPARE_GROUP", 7):
            hip.ggsw_prepare_batched(d_q.ptr, d_g.ptr, count, dnum, rank, size)
            hip.sync()
        assert np.array_equal(d_q.download(np.uint8, want.nbytes), want)


# ---- pz_fhe_uint_prepare_batched ----------------------------------------------------------------------------------------------------------------
SHAPES = {"ref": fc.REF_SHAPE, "ref-lwe4": fc.REF_SHAPE_LWE4, "one-base": fc.ONE_BASE_SHAPE, "one-base-n1024": dict(fc.ONE_BASE_SHAPE, n=1024)}


def route_of(c):
    """N = 1024 with one base for everything: the rotation on load; N = 256: no small-ring kernels"""
    return NOTE_ON_LOAD if c.n == 1024 and c.ks_b == c.word_b == c.lwe_b else NOTE_MATERIALISED


class Key:
    """A case's BDD key prepared and resident on the device, with the oracle's copy next to it."""

    def __init__(self, dev, ref, hip, c):
        self.c = c
        self.ref_key = fo.PreparedKey(ref, c)
        hk = fo.PreparedKey(hip, c)
        self.d_brk, self.d_lut = dev.upload(hk.brk), dev.upload(c.lut)
        self.d_atk, self.d_tsk = [dev.key(k) for k in hk.atk], [dev.key(k) for k in hk.tsk]
        self.d_ks_glwe = dev.key(hk.ks_glwe)
        self.d_ks_lwe = {name: dev.key(k) for name, k in hk.ks_lwe.items()}
        self.gals = c.gals

    def view(self, with_ks_glwe):
        """the object poulpy_amd.bdd.fhe_uint_prepare takes"""
        from types import SimpleNamespace
        return SimpleNamespace(ks_glwe=self.d_ks_glwe.ptr if with_ks_glwe else None, ks_lwe=self.d_ks_lwe["mid" if with_ks_glwe else "direct"].ptr,
                               lut=self.d_lut.ptr, brk=self.d_brk.ptr, gals=self.gals, atk=[k.ptr for k in self.d_atk], tsk=[k.ptr for k in self.d_tsk])


def ggsw_doubles(c):
    return c.res_dnum * (c.rank + 1) ** 2 * c.res_size * c.n


def run_prepare(dev, hip, key, words, word_bits, bit_start, bit_count, with_ks_glwe, chunk=0):
    """-> (pmat (batch, word_bits, doubles) as bytes, ggsw, lwe) of one call with every optional output"""
    c = key.c
    batch, cols = len(words), c.rank + 1
    p = fc.prepare_params(c, with_ks_glwe, word_bits, bit_start, bit_count)
    need = hip.fhe_uint_prepare_tmp_bytes(p, batch, chunk)
    d_tmp = dev.alloc(max(need, 8))
    d_w = dev.upload(words)
    gd = ggsw_doubles(c)
    d_p, d_g = dev.alloc(batch * word_bits * gd * 8), dev.alloc(batch * word_bits * gd * 8)
    d_l = dev.alloc(max(batch * bit_count * c.lwe_size * (c.n_lwe + 1) * 8, 8))
    hip.dispatch_notes(reset=True)
    bits = bdd.fhe_uint_prepare(hip, d_p.ptr, d_w.ptr, key.view(with_ks_glwe), p, batch, tmp=d_tmp, ggsw_out=d_g.ptr, lwe_out=d_l.ptr)
    hip.sync()
    if bit_count:
        assert_route(hip.dispatch_notes(), route_of(c), (c.n, with_ks_glwe))
    assert bits[batch - 1][word_bits - 1] == d_p.ptr.value + ((batch - 1) * word_bits + word_bits - 1) * gd * 8
    pmat = d_p.download(np.uint8, d_p.nbytes).reshape(batch, word_bits, gd * 8)
    ggsw = d_g.download(np.int64, batch * word_bits * gd).reshape(batch, word_bits, c.res_dnum, cols, c.res_size, cols, c.n)
    lwe = d_l.download(np.int64, batch * bit_count * c.lwe_size * (c.n_lwe + 1)).reshape(batch, bit_count, c.lwe_size, c.n_lwe + 1)
    return pmat, ggsw, lwe


def check_against_oracle(ref, hip, key, got, words, word_bits, bit_start, bit_count, with_ks_glwe, label):
    c = key.c
    pmat, ggsw, lwe = got
    want = fo.prepare_words(ref, c, key.ref_key, words, word_bits, bit_start, bit_count, with_ks_glwe)
    assert np.array_equal(lwe, want.lwe), (label, "lwe_out != oracle")
    assert np.array_equal(ggsw, want.ggsw), (label, "ggsw_out != oracle")
    cols = c.rank + 1
    for b in range(len(words)):
        for i in range(word_bits):
            inside = bit_start <= i < bit_start + bit_count
            if not inside:
                assert not pmat[b, i].any() and not ggsw[b, i].any(), (label, b, i, "a bit outside the range is not zero")
                continue
            ph = hip.vmp_pmat_alloc(c.res_dnum, cols, cols, c.res_size)
            hip.vmp_prepare(ph, MatZnx(c.n, c.res_dnum, cols, cols, c.res_size, np.ascontiguousarray(ggsw[b, i])))
            assert np.array_equal(pmat[b, i], ph.data.reshape(-1).view(np.uint8)), (label, b, i, "res_pmat != pz_vmp_prepare(ggsw_out)")


@pytest.mark.parametrize("with_ks_glwe", [True, False], ids=["ks_glwe", "direct"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_prepare_u8_word_equals_oracle(mods, shape, with_ks_glwe):
    c = fc.bdd_key_case(SHAPES[shape], 43000)
    ref, hip = mods(c.n)
    for values in ([0xA5], [0x3C, 0xFF, 0x00]):
        words = fc.words_case(c, 8, values, 43100 + len(values))
        with on_device(hip) as dev:
            key = Key(dev, ref, hip, c)
            got = run_prepare(dev, hip, key, words, 8, 0, 8, with_ks_glwe)
            check_against_oracle(ref, hip, key, got, words, 8, 0, 8, with_ks_glwe, (shape, with_ks_glwe, values))


@pytest.mark.parametrize("shape", ["ref", "one-base", "one-base-n1024"])
def test_prepare_u32_sub_range_and_passes(mods, shape):
    """bit_start = 5, bit_count = 7 of a u32 word, 3 words: the other 25 bits are all-zero bytes.  Then the same call on smaller tmps, the same
    bytes each time: 14 of the 21 (word, bit) pairs - two passes, of two words and of one; 11 pairs - one word per pass, three passes; 3 pairs -
    bit ranges of one word.  Last with 20 polynomials of prepare scratch: several launch pairs per pass, rows of 2 words and of 1."""
    c = fc.bdd_key_case(SHAPES[shape], 43200)
    ref, hip = mods(c.n)
    words = fc.words_case(c, 32, [0xDEADBEEF, 0x12345678, 0x0F0F0F0F], 43300)
    with on_device(hip) as dev:
        key = Key(dev, ref, hip, c)
        whole = run_prepare(dev, hip, key, words, 32, 5, 7, True)
        check_against_oracle(ref, hip, key, whole, words, 32, 5, 7, True, (shape, "u32 [5, 12)"))
        p = fc.prepare_params(c, True, 32, 5, 7)
        sizes = [hip.fhe_uint_prepare_tmp_bytes(p, 3, k) for k in (3, 11, 14, 0)]
        assert sizes == sorted(sizes) and len(set(sizes)) == 4
        for chunk, what in ((14, "passes of 2 words and 1 word"), (11, "three passes of one word")):
            split = run_prepare(dev, hip, key, words, 32, 5, 7, True, chunk=chunk)
            for a, b, part in zip(whole, split, ("res_pmat", "ggsw_out", "lwe_out")):
                assert np.array_equal(a, b), (shape, part, what, "differs from one pass")
        # fewer pairs than one word has bits: bit ranges of one word per pass
        narrow = run_prepare(dev, hip, key, words[:1], 32, 5, 7, True, chunk=3)
        for a, b, part in zip(whole, narrow, ("res_pmat", "ggsw_out", "lwe_out")):
            assert np.array_equal(a[:1], b), (shape, part, "passes of 3 bits differ from one")
        with knob("POULPY_DBG_PREPARE_GROUP", 20):      # a word's 7 GGSWs are 7 * 24 or 7 * 54 polynomials: rows wider than the scratch
            small = run_prepare(dev, hip, key, words, 32, 5, 7, True, chunk=14)
        assert np.array_equal(whole[0], small[0]), (shape, "res_pmat with a small prepare scratch")
        with knob("POULPY_DBG_PREPARE_GROUP", 400):     # 2 rows of 168 polynomials fit (rank 1): row groups; rank 2: one row of 378 per pair
            rows = run_prepare(dev, hip, key, words, 32, 5, 7, True)
        assert np.array_equal(whole[0], rows[0]), (shape, "res_pmat with row groups")


def test_refusals_launch_nothing_and_no_ops(mods):
    from poulpy_amd import abi
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE, 43400)
    ref, hip = mods(c.n)
    batch, wb = 2, 8
    words = fc.words_case(c, wb, [1, 2], 43500)
    gd = ggsw_doubles(c)
    with on_device(hip, timing=True) as dev:
        key = Key(dev, ref, hip, c)
        hip.sync()
        p = fc.prepare_params(c, True, wb, 0, wb)
        need = hip.fhe_uint_prepare_tmp_bytes(p, batch)
        d_tmp, d_w = dev.alloc(need), dev.upload(words)
        d_p = dev.alloc(batch * wb * gd * 8)
        v = key.view(True)
        g = (C.c_int64 * len(v.gals))(*v.gals)
        ap = (C.c_void_p * len(v.atk))(*[x.value for x in v.atk])
        tp = (C.c_void_p * len(v.tsk))(*[x.value for x in v.tsk])

        def call(p=p, ks_lwe=v.ks_lwe, tmp_bytes=need, batch=batch):
            st = hip.lib.pz_fhe_uint_prepare_batched(hip.handle, d_p.ptr, None, None, d_w.ptr, v.ks_glwe, ks_lwe, v.lut, v.brk, len(v.gals), g, ap, tp,
                                                     C.byref(p), d_tmp.ptr, tmp_bytes, batch)
            return st, hip.lib.pz_last_error().decode()
        hip.set_kernel_timing(True)     # (resets the counters)
        graphs = hip.graph_launches()
        one_pair = hip.fhe_uint_prepare_tmp_bytes(p, batch, 1)
        for label, kw, msg in (
                ("null key", dict(ks_lwe=None), "null argument"),
                ("word_bits 12", dict(p=fc.prepare_params(c, True, 12, 0, 8)), "word_bits = 12"),
                ("word_bits 256", dict(p=fc.prepare_params(c, True, 256, 0, 8)), "word_bits = 256"),
                ("bits leave the word", dict(p=fc.prepare_params(c, True, wb, 5, 4)), "leave the word"),
                ("tmp too small", dict(tmp_bytes=one_pair - 1), "tmp holds no")):
            st, text = call(**kw)
            assert st == abi.PZ_ERR_INVALID and msg in text, (label, st, text)
        # n % word_bits != 0 needs a ring smaller than the word: N = 64 with 128-bit words
        _, small = mods(64)
        st = small.lib.pz_fhe_uint_prepare_batched(small.handle, d_p.ptr, None, None, d_w.ptr, v.ks_glwe, v.ks_lwe, v.lut, v.brk, len(v.gals), g, ap, tp,
                                                   C.byref(fc.prepare_params(c, True, 128, 0, 8)), d_tmp.ptr, need, batch)
        assert st == abi.PZ_ERR_INVALID and "no multiple of word_bits" in small.lib.pz_last_error().decode()
        # pz_ggsw_prepare_batched: pmat inside ggsw
        st = hip.lib.pz_ggsw_prepare_batched(hip.handle, d_p.ptr.value + 64, d_p.ptr, 2, c.res_dnum, c.rank, c.res_size)
        assert st == abi.PZ_ERR_ALIAS and "overlaps" in hip.lib.pz_last_error().decode()
        # batch == 0: PZ_OK, nothing launched
        st, text = call(batch=0)
        assert st == 0, text
        hip.sync()
        assert all(cnt == 0 for cnt, _ in hip.kernel_stats().values()), hip.kernel_stats()
        assert hip.graph_launches() == graphs
        assert np.all(d_p.download(np.uint8, d_p.nbytes) == 0x5A) and np.all(d_tmp.download(np.uint8, need) == 0x5A), "a refused call wrote"
        # bit_count == 0 zeroes every bit and needs no tmp
        st, text = call(p=fc.prepare_params(c, True, wb, 3, 0), tmp_bytes=0)
        assert st == 0, text
        hip.sync()
        assert not d_p.download(np.uint8, d_p.nbytes).any()
        assert hip.graph_launches() == graphs


# ---- under real keys: words -> adder -> word -> ltu, decryption only ------------------------------------------------------------------------------
def test_encrypted_u16_addition_then_comparison_decrypts(mods):
    """Two u16 words per batch element through fhe_uint_prepare, adder(16) on the evaluator, fhe_uint_pack: the packed word decrypts to
    (a + b) mod 2^16.  That word is prepared AGAIN and compared with a third word by ltu(16).  Packing at the un-interleaved indices
    i << log_gap must not decrypt to the sum."""
    from poulpy_amd.hal import GlweOpParams
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE, 44000)
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
            d_w = dev.upload(fc.words_case(c, w, values, 44100 + k))
            d_p = dev.alloc(batch * w * gd * 8)
            tables.append(bdd.fhe_uint_prepare(hip, d_p.ptr, d_w.ptr, view, p_in, batch, tmp=d_tmp))
        bits = [tables[0][b] + tables[1][b] for b in range(batch)]
        d_out = dev.alloc(w * batch * ct * 8)
        bdd.execute_bdd_circuit(hip, bdd.adder(w), (d_out.ptr, w), bits, gate, batch)
        hip.sync()
        d_keep = dev.upload(d_out.download(np.int64, w * batch * ct))      # (packing clobbers its inputs: a copy for the control)
        d_sum, d_bad = dev.alloc(batch * ct * 8), dev.alloc(batch * ct * 8)
        atk = [k.ptr for k in key.d_atk]
        bdd.fhe_uint_pack(hip, d_sum.ptr, d_out.ptr, w, c.gals, atk, pack, batch)
        bdd.fhe_uint_pack(hip, d_bad.ptr, d_keep.ptr, w, c.gals, atk, pack, batch, index=lambda s, wb: s)
        hip.sync()
        total = d_sum.download(np.int64, batch * ct).reshape(batch, size, cols, c.n)
        bad = d_bad.download(np.int64, batch * ct).reshape(batch, size, cols, c.n)
        for b, (x, y) in enumerate(pairs):
            assert fc.decrypt_word(c, total[b], w) == (x + y) & 0xFFFF, (b, "the packed sum")
            assert fc.decrypt_word(c, bad[b], w) != (x + y) & 0xFFFF, (b, "un-interleaved packing decrypted to the sum")
        # the result is a word again: its layout is the evaluator's (res_b, `size` limbs)
        p_sum = fc.prepare_params(c, True, w, 0, w)
        p_sum.ks_glwe.a_size, p_sum.ks_glwe.a_base2k = size, c.res_b
        d_ps = dev.alloc(batch * w * gd * 8)
        d_tmp2 = dev.alloc(hip.fhe_uint_prepare_tmp_bytes(p_sum, batch))
        t_sum = bdd.fhe_uint_prepare(hip, d_ps.ptr, d_sum.ptr, view, p_sum, batch, tmp=d_tmp2)
        bits = [t_sum[b] + tables[2][b] for b in range(batch)]
        d_lt = dev.alloc(batch * ct * 8)
        bdd.execute_bdd_circuit(hip, bdd.ltu(w), (d_lt.ptr, 1), bits, gate, batch)
        hip.sync()
        lt = d_lt.download(np.int64, batch * ct).reshape(batch, size, cols, c.n)
        for b, (x, y) in enumerate(pairs):
            pt = fs.normalize(fs.glwe_phase(lt[b], c.sk_glwe), c.res_b)
            assert fs.decode_coeff(pt, c.res_b, 2, 0) & 1 == int(((x + y) & 0xFFFF) < thirds[b]), (b, "sum < third")
