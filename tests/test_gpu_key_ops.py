"""GPU parity of the key-level forms of key switching against the oracle compositions of tests/key_ops_cases.py, bit for bit on every limb:
pz_glwe_automorphism_key_automorphism_batched on both of its routes (the key switch by the permuted key on the 128-point-row plans, the
composition everywhere else), pz_ggsw_keyswitch_batched and pz_ggsw_automorphism_batched.  The fast-form shapes use base2k = 12 so that
uniform inputs hit carry ties many times per case, and each of them checks (on the oracle's output) that a tie met a minus sign: a tail with
another sign rule cannot pass."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fhe_sk as fs
from tests import key_ops_cases as kc
from tests import unnormalized as un
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import MARGIN_MAX, seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = "key composition: key switch by the permuted key"
COMPOSED = "key composition: automorphism + glwe_automorphism"


@pytest.fixture(autouse=True)
def spectral_switch(monkeypatch):
    """The switch is read at every call: the tests of this file ask for the fast form explicitly (the shapes decide where it applies); the
    composition on a fast-form shape is asked for in a child process (test_switch_forces_the_composition_with_the_same_digits)."""
    monkeypatch.setenv("POULPY_DBG_KEYAUTO_SPECTRAL", "1")


def gals(n):
    """both residues mod 4, both signs, a large element"""
    return (-1, 5, -5, 2 * n - 1 - 4)


class Shape:
    """One key-composition shape: `count` GGLWEs of a_dnum rows (rank columns, a_size limbs at a_base2k) and the applied key."""
    def __init__(self, n, rank, a_size, a_base2k, key_size, key_base2k, key_dnum, dsize=1, count=1, a_dnum=2, seed=0, wide=0):
        self.n, self.rank, self.a_size, self.a_base2k = n, rank, a_size, a_base2k
        self.key_size, self.key_base2k, self.key_dnum, self.dsize, self.count, self.a_dnum = key_size, key_base2k, key_dnum, dsize, count, a_dnum
        rng = seeded(1000 + seed + n + 7 * rank + a_size)
        cols = rank + 1
        self.a = fs.uniform_digits((count, a_dnum, rank, a_size, cols, n), a_base2k, rng)
        if wide:   # un-normalized input limbs (tests/unnormalized.py, class 1)
            self.a = un.wide_digits(rng, self.a.shape, a_base2k, wide)
        self.key = fs.uniform_digits((key_dnum, rank, key_size, cols, n), key_base2k, rng)

    def params(self, res_size):
        from poulpy_amd.hal import GlweOpParams
        return GlweOpParams(rank=self.rank, dnum=self.key_dnum, dsize=self.dsize, key_size=self.key_size, key_base2k=self.key_base2k,
                            a_size=self.a_size, a_base2k=self.a_base2k, res_size=res_size, res_base2k=self.a_base2k, rank_out=self.rank)

    def oracle(self, ref, a_gal, res_dnum=None, res_size=None):
        res_dnum, res_size = res_dnum or self.a_dnum, res_size or self.a_size
        pm = kc.prepare(ref, self.key)
        return np.stack([kc.key_composition(ref, self.a[i], self.a_base2k, a_gal, pm, self.dsize, self.key_base2k, res_dnum, res_size)
                         for i in range(self.count)])


def one_base(n, rank, limbs, base2k=12, dnum=None, **kw):
    return Shape(n, rank, limbs, base2k, limbs, base2k, dnum or limbs, **kw)


def device(hip, s, a_gal, res_dnum=None, res_size=None, in_place=False, key="device", pin=False):
    """One call -> (digits, dispatch notes)."""
    res_dnum, res_size = res_dnum or s.a_dnum, res_size or s.a_size
    ph = kc.prepare(hip, s.key)
    shape = (s.count, res_dnum, s.rank, res_size, s.rank + 1, s.n)
    with on_device(hip) as dev:
        d_a, d_key = dev.upload(s.a), dev.key(ph)
        key_ptr = d_key.ptr if key == "device" else ph.data.ctypes.data
        if in_place:
            assert shape == s.a.shape
            d_res = d_a
        else:
            d_res = dev.alloc(int(np.prod(shape)) * 8)
        if pin:   # ... and one plain key switch by the pinned key first, so that its cached row slices exist when the composition runs
            dev.pin(d_key, s.key_dnum, s.rank, s.rank + 1, s.key_size)
            d_warm = dev.alloc(int(np.prod(shape)) * 8, poison=False)
            hip.glwe_keyswitch_batched(d_warm.ptr, d_a.ptr, d_key.ptr, s.params(res_size), s.count * res_dnum * s.rank)
            hip.sync()
            warm = d_warm.download(np.int64, int(np.prod(shape))).reshape(shape)
            dev.free(d_warm)
        hip.dispatch_notes(reset=True)
        gal = hip.glwe_automorphism_key_automorphism_batched(d_res.ptr, res_dnum, d_a.ptr, s.a_dnum, a_gal, key_ptr, -5, s.params(res_size), s.count)
        assert gal == (a_gal * -5) % (2 * s.n)
        hip.sync()
        got = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
        notes = hip.dispatch_notes()
        extra = None
        if pin:   # a plain key switch by the pinned key afterwards: its cached row slices are still the key's own
            hip.glwe_keyswitch_batched(d_res.ptr, d_a.ptr, d_key.ptr, s.params(res_size), s.count * res_dnum * s.rank)
            hip.sync()
            extra = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
            assert np.array_equal(extra, warm), "the pinned key's cached slices changed across the composition call"
    return (got, notes, extra) if pin else (got, notes)


def run_all_gals(ref, hip, s, route, ties=False):
    for a_gal in gals(s.n):
        want = s.oracle(ref, a_gal)
        if ties:
            assert kc.has_tie_sign(want, s.a_base2k), ("no carry tie under a minus sign in this case: enlarge count", s.n, a_gal)
        for in_place in (False, True):
            got, notes = device(hip, s, a_gal, in_place=in_place)
            assert route in notes, (s.n, a_gal, notes)
            assert np.array_equal(got, want), (s.n, s.rank, a_gal, "in place" if in_place else "out of place", route)


# ---- 4. parity on every route ----
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("dsize", [1, 2])
def test_composition_cross_base_n256(mods, rank, dsize):
    """per-op plans, input key in base2k - 1 and applied key in base2k, 2 GGLWEs of 3 rows, res with 3 and with 2 rows (and other limbs)"""
    ref, hip = mods(256)
    k_in = 3 * 16
    s = Shape(256, rank, 3, 16, -(-(k_in + 17 * dsize) // 17), 17, -(-k_in // (17 * dsize)), dsize=dsize, count=2, a_dnum=3, seed=dsize)
    run_all_gals(ref, hip, s, COMPOSED)
    for a_gal in gals(256):
        got, notes = device(hip, s, a_gal, res_dnum=2, res_size=4)
        assert COMPOSED in notes
        assert np.array_equal(got, s.oracle(ref, a_gal, res_dnum=2, res_size=4)), (rank, dsize, a_gal)


@pytest.mark.parametrize("n", [2048, 4096])
def test_composition_small_rings(mods, n):
    """N = 2048: the one-kernel small ring; N = 4096 with 3 key limbs: the two-kernel path - both take the composition"""
    ref, hip = mods(n)
    run_all_gals(ref, hip, one_base(n, 1, 3, count=2), COMPOSED)


FAST_SHAPES = {"n4096-rank1": dict(n=4096, rank=1, limbs=6, a_dnum=6, count=2), "n4096-rank2": dict(n=4096, rank=2, limbs=6, a_dnum=6, count=2),
               "n8192": dict(n=8192, rank=1, limbs=5, a_dnum=2, count=1), "n65536": dict(n=65536, rank=1, limbs=4, dnum=2, a_dnum=2, count=1)}


def fast_shape(name, **kw):
    d = dict(FAST_SHAPES[name], **kw)
    return one_base(d.pop("n"), d.pop("rank"), d.pop("limbs"), **d)


@pytest.mark.parametrize("name", list(FAST_SHAPES))
def test_fast_form_parity(mods, name):
    s = fast_shape(name)
    ref, hip = mods(s.n)
    run_all_gals(ref, hip, s, FAST, ties=True)


def test_fast_form_fewer_result_rows(mods):
    """res_dnum < a_dnum with two GGLWEs: one call per GGLWE, the rows beyond res_dnum neither read nor written"""
    s = fast_shape("n4096-rank1", a_dnum=3)
    ref, hip = mods(s.n)
    got, notes = device(hip, s, -5, res_dnum=2, res_size=5)
    assert FAST in notes
    assert np.array_equal(got, s.oracle(ref, -5, res_dnum=2, res_size=5))


# ---- 5. cross-checks ----
@pytest.mark.parametrize("name", ["n4096-rank1", "n256"])
def test_identity_element_is_a_plain_key_switch(mods, name):
    from tests import core_cases as cs
    s = fast_shape(name) if name != "n256" else Shape(256, 2, 3, 16, 4, 17, 3, count=2, a_dnum=3)
    ref, hip = mods(s.n)
    got, _ = device(hip, s, 1)
    c = type("C", (), dict(op="ks", key=s.key, a=s.a.reshape((-1,) + s.a.shape[3:]), res_size=s.a_size, res_base2k=s.a_base2k,
                           a_base2k=s.a_base2k, dsize=s.dsize, key_base2k=s.key_base2k))
    want = cs.run_oracle(ref, c).reshape(got.shape)
    assert np.array_equal(got, want)
    # ... and the device's own key switch says the same
    ph = kc.prepare(hip, s.key)
    with on_device(hip) as dev:
        d_a, d_key, d_res = dev.upload(s.a), dev.key(ph), dev.alloc(s.a.nbytes, poison=False)
        hip.glwe_keyswitch_batched(d_res.ptr, d_a.ptr, d_key.ptr, s.params(s.a_size), s.count * s.a_dnum * s.rank)
        hip.sync()
        assert np.array_equal(d_res.download(np.int64, s.a.size).reshape(got.shape), got)


def _digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from oracle.ref import RefModule
from poulpy_amd.hal import Module
from tests import test_gpu_key_ops as t
name, route = sys.argv[1], sys.argv[2]
s = t.fast_shape(name)
hip = Module(s.n)
for a_gal in t.gals(s.n):
    got, notes = t.device(hip, s, a_gal)
    assert getattr(t, route) in notes, notes
    print("digest", a_gal, t._digest(got), flush=True)
"""


def _child(name, route, **env):
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, name, route], capture_output=True, text=True, env=e, cwd=ROOT, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "WORKSPACE OVERRUN" not in out.stderr
    return {int(l.split()[1]): l.split()[2] for l in out.stdout.splitlines() if l.startswith("digest")}


@pytest.mark.parametrize("name", ["n4096-rank1", "n8192"])
def test_switch_forces_the_composition_with_the_same_digits(mods, name):
    s = fast_shape(name)
    ref, hip = mods(s.n)
    composed = _child(name, "COMPOSED", POULPY_DBG_KEYAUTO_SPECTRAL="0")
    assert len(composed) == len(gals(s.n))
    for a_gal in gals(s.n):
        got, notes = device(hip, s, a_gal)
        assert FAST in notes
        assert _digest(got) == composed[a_gal], (name, a_gal)


def test_pinned_and_host_resident_keys(mods):
    s = fast_shape("n4096-rank1")
    ref, hip = mods(s.n)
    want = s.oracle(ref, -5)
    got, notes, ks = device(hip, s, -5, pin=True)
    unpinned, _ = device(hip, s, -5)
    assert FAST in notes and np.array_equal(got, want) and np.array_equal(got, unpinned)
    assert np.array_equal(ks, s.oracle(ref, 1)), "the pinned key's cached slices changed"
    got, notes = device(hip, s, -5, key="host")
    assert FAST in notes and np.array_equal(got, want)
    small = Shape(256, 1, 3, 16, 4, 17, 3, count=1, a_dnum=2)
    rs, hs = mods(256)
    got, notes = device(hs, small, 5, key="host")
    assert COMPOSED in notes and np.array_equal(got, small.oracle(rs, 5))


# ---- 6. un-normalized input limbs ----
@pytest.mark.parametrize("name,route", [("n4096-rank1", FAST), ("n8192", FAST), ("n256", COMPOSED), ("n4096-small", COMPOSED)])
def test_unnormalized_input_limbs(mods, name, route):
    if name == "n256":
        s = Shape(256, 2, 3, 16, 4, 17, 3, count=2, a_dnum=2, wide=3)
    elif name == "n4096-small":
        s = one_base(4096, 1, 3, count=2, wide=3)
    else:
        s = fast_shape(name, wide=3)
    un.check_unnormalized(s.a, s.a_base2k)
    ref, hip = mods(s.n)
    for a_gal in (-5, 5):
        got, notes = device(hip, s, a_gal)
        assert route in notes
        assert np.array_equal(got, s.oracle(ref, a_gal)), (name, a_gal)


# ---- 7. rounding margin ----
@pytest.mark.parametrize("name", ["n4096-rank1", "n65536"])
def test_fast_form_rounding_margin(mods, name):
    s = fast_shape(name)
    ref, hip = mods(s.n)
    want = s.oracle(ref, -5)
    out = {}

    def run():
        out["got"], out["notes"] = device(hip, s, -5)
    margin = hip.rounding_margin_of(run)
    print(f"[margin] key composition, fast form, {name}: {margin:.4f}")
    assert FAST in out["notes"] and np.array_equal(out["got"], want)
    assert 0.0 < margin < MARGIN_MAX, margin


# ---- 8. GGSW forms ----
class GgswShape:
    def __init__(self, n, rank, a_size, a_base2k, key_size, key_base2k, key_dnum, dsize=1, count=2, a_dnum=3, seed=0):
        self.n, self.rank, self.a_size, self.a_base2k = n, rank, a_size, a_base2k
        self.key_size, self.key_base2k, self.key_dnum, self.dsize, self.count, self.a_dnum = key_size, key_base2k, key_dnum, dsize, count, a_dnum
        rng = seeded(2000 + seed + n + 7 * rank + a_size)
        cols = rank + 1
        self.a = fs.uniform_digits((count, a_dnum, cols, a_size, cols, n), a_base2k, rng)
        self.key = fs.uniform_digits((key_dnum, rank, key_size, cols, n), key_base2k, rng)
        self.tsk = [fs.uniform_digits((key_dnum, rank, key_size, cols, n), key_base2k, rng) for _ in range(rank)]
        self.res_size = a_size

    def params(self, expand=False):
        """the key switch of the entries (row, 0): a's layout -> res's; expand: ggsw_expand_row's, res -> res"""
        from poulpy_amd.hal import GlweOpParams
        return GlweOpParams(rank=self.rank, dnum=self.key_dnum, dsize=self.dsize, key_size=self.key_size, key_base2k=self.key_base2k,
                            a_size=self.res_size if expand else self.a_size, a_base2k=self.a_base2k, res_size=self.res_size,
                            res_base2k=self.a_base2k, rank_out=self.rank)


def ggsw_device(hip, s, op, gal=None, res_dnum=None, in_place=False):
    res_dnum = res_dnum or s.a_dnum
    cols = s.rank + 1
    shape = (s.count, res_dnum, cols, s.res_size, cols, s.n)
    ph = kc.prepare(hip, s.key)
    pts = [kc.prepare(hip, t) for t in s.tsk]
    with on_device(hip) as dev:
        d_a, d_key, d_tsk = dev.upload(s.a), dev.key(ph), [dev.key(p) for p in pts]
        if in_place:
            assert shape == s.a.shape
            d_res = d_a
        else:
            d_res = dev.alloc(int(np.prod(shape)) * 8)
        if op == "ks":
            hip.ggsw_keyswitch_batched(d_res.ptr, d_a.ptr, s.a_dnum, d_key.ptr, [t.ptr for t in d_tsk], s.params(), s.params(expand=True), s.count)
        else:
            hip.ggsw_automorphism_batched(d_res.ptr, res_dnum, d_a.ptr, s.a_dnum, d_key.ptr, gal, [t.ptr for t in d_tsk], s.params(), s.params(expand=True), s.count)
        hip.sync()
        return d_res.download(np.int64, int(np.prod(shape))).reshape(shape)


def ggsw_oracle(ref, s, op, gal=None, res_dnum=None):
    pm = kc.prepare(ref, s.key)
    pts = [kc.prepare(ref, t) for t in s.tsk]
    if op == "ks":
        return np.stack([kc.ggsw_keyswitch(ref, s.a[i], s.a_base2k, pm, s.dsize, s.key_base2k, pts, s.res_size) for i in range(s.count)])
    return np.stack([kc.ggsw_automorphism(ref, s.a[i], s.a_base2k, pm, s.dsize, s.key_base2k, gal, pts, res_dnum or s.a_dnum, s.res_size)
                     for i in range(s.count)])


GGSW_SHAPES = [("n256", 1, 1), ("n256", 1, 2), ("n256", 2, 1), ("n256", 2, 2), ("n4096", 1, 1)]


def _ggsw_shape(name, rank, dsize):
    if name == "n256":
        k_in = 3 * 16
        return GgswShape(256, rank, 3, 16, -(-(k_in + 17 * dsize) // 17), 17, -(-k_in // (17 * dsize)), dsize=dsize, seed=dsize)
    return GgswShape(4096, rank, 6, 12, 6, 12, 6, a_dnum=2)


@pytest.mark.parametrize("name,rank,dsize", GGSW_SHAPES)
def test_ggsw_keyswitch_parity(mods, name, rank, dsize):
    s = _ggsw_shape(name, rank, dsize)
    ref, hip = mods(s.n)
    want = ggsw_oracle(ref, s, "ks")
    for in_place in (False, True):
        assert np.array_equal(ggsw_device(hip, s, "ks", in_place=in_place), want), (name, rank, dsize, in_place)


@pytest.mark.parametrize("name,rank,dsize", GGSW_SHAPES)
def test_ggsw_automorphism_parity(mods, name, rank, dsize):
    s = _ggsw_shape(name, rank, dsize)
    ref, hip = mods(s.n)
    for gal in (-1, -5):
        want = ggsw_oracle(ref, s, "auto", gal=gal)
        for in_place in (False, True):
            assert np.array_equal(ggsw_device(hip, s, "auto", gal=gal, in_place=in_place), want), (name, rank, dsize, gal, in_place)
        fewer = ggsw_device(hip, s, "auto", gal=gal, res_dnum=s.a_dnum - 1)
        assert np.array_equal(fewer, ggsw_oracle(ref, s, "auto", gal=gal, res_dnum=s.a_dnum - 1)), (name, rank, dsize, gal, "fewer rows")


# ---- 9. semantics on the device ----
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("dsize", [1, 2, 3, 4])
def test_key_composition_semantics_on_device(mods, rank, dsize):
    """The reference's test (test_suite/automorphism/gglwe_atk.rs:20-185, N = 256) through the entry point: device == oracle, the derived
    key's noise within the reference's bound; the control (input key declared with the other Galois element) lands beyond it."""
    ref, hip = mods(256)
    c = kc.composition_case(256, 17, rank, dsize, seed=100 * rank + dsize)
    s = Shape(256, rank, c.key_in.shape[2], c.in_b, c.key_apply.shape[2], c.key_b, c.dnum_ksk, dsize=dsize, count=1, a_dnum=c.dnum_in)
    s.a, s.key = c.key_in[None], c.key_apply
    for a_gal, fail in ((c.p0, False), (c.p1, True)):
        got, _ = device(hip, s, a_gal, res_size=c.res_size)
        assert np.array_equal(got, s.oracle(ref, a_gal, res_size=c.res_size)), (rank, dsize, a_gal)
        have = kc.composition_noise(c, got[0])
        print(f"[noise] key composition on device rank {rank} dsize {dsize} a_gal {a_gal}: {max(have):.2f} (min {min(have):.2f}) want {c.bound:.2f}")
        assert (min(have) > c.bound) if fail else (max(have) <= c.bound), (have, c.bound)


@pytest.mark.parametrize("op", ["ks", "auto"])
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("dsize", [1, 2, 3, 4])
def test_ggsw_forms_semantics_on_device(mods, op, rank, dsize):
    """test_suite/keyswitch/ggsw_ct.rs and test_suite/automorphism/ggsw_ct.rs (N = 256) through the entry points: device == oracle, every
    entry's noise within the reference's bound for its column; the controls land beyond it."""
    ref, hip = mods(256)
    for control in (False, True):
        c = kc.ggsw_case(op, 256, 17, rank, dsize, seed=300 + 10 * rank + dsize, control=control)
        s = GgswShape(256, rank, c.a.shape[2], c.in_b, c.key.shape[2], c.key_b, c.key.shape[0], dsize=dsize, count=1, a_dnum=c.dnum_in)
        s.a, s.key, s.tsk, s.res_size = c.a[None], c.key, c.tsk, c.res_size
        got = ggsw_device(hip, s, op, gal=c.p)
        assert np.array_equal(got[0], kc.ggsw_run_oracle(ref, c)), (op, rank, dsize, control)
        kc.ggsw_check((op, rank, dsize, "control" if control else "device"), c, got[0], fail=control)


# ---- 10. workspace guards ----
CANARY_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from oracle.ref import RefModule
from poulpy_amd.hal import Module
from tests import test_gpu_key_ops as t
s = t.fast_shape("n4096-rank1")
ref, hip = RefModule(s.n), Module(s.n)
got, notes = t.device(hip, s, -5)
assert t.FAST in notes and np.array_equal(got, s.oracle(ref, -5))
small = t.Shape(256, 1, 3, 16, 4, 17, 3, count=2, a_dnum=3)
r2, h2 = RefModule(256), Module(256)
got, notes = t.device(h2, small, -5, in_place=True)
assert t.COMPOSED in notes and np.array_equal(got, small.oracle(r2, -5))
g = t._ggsw_shape("n256", 2, 2)
assert np.array_equal(t.ggsw_device(h2, g, "auto", gal=-5, res_dnum=2), t.ggsw_oracle(r2, g, "auto", gal=-5, res_dnum=2))
assert np.array_equal(t.ggsw_device(h2, g, "ks"), t.ggsw_oracle(r2, g, "ks"))
print("guarded run ok", flush=True)
"""


def test_workspace_guards():
    env = dict(os.environ, POULPY_DBG_CANARY="1", POULPY_DBG_KEYAUTO_SPECTRAL="1")
    out = subprocess.run([sys.executable, "-c", CANARY_CHILD % ROOT], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "WORKSPACE OVERRUN" not in out.stderr and "guarded run ok" in out.stdout
