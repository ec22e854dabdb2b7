"""pz_glwe_cmux_batched against tests/cmux_oracle.py, bit for bit, on every route, in every form.

Every case is a batch of 3 ciphertexts in waves of 2 (a wave boundary inside the batch), each ciphertext with its own t and f; outputs are
poisoned before the call unless they are an operand.  Routes, with the dispatch note asserted: the one-kernel and two-kernel small-ring
forms whose forward stage reads both sources (N = 1024 / 2048 / 4096), and the materialised difference on the three-kernel pipeline
(N = 4096 small path off, N = 8192), the five-kernel path (N = 8192 fusion off, N = 256) and - under POULPY_DBG_CMUX_FUSED=0, in a child
process - on the small rings.  Then: the rotated source at the wrap points of the monomial map, un-normalized digits, the rounding margin
(printed with `-s`; DESIGN.md section 7 quotes it), and encrypt / CMUX / decrypt under real keys with its negative control."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import cmux_oracle as co
from tests import fhe_sk
from tests import unnormalized as un
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import MARGIN_MAX, seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, TWO, MAT = co.NOTE_ONE, co.NOTE_TWO, co.NOTE_MAT
BATCH, CHUNK = 3, 2


class Case:
    """One call: form "cmux" (t, f, res distinct), "assign" (res == t), "assign_neg" (res == f) or "rot" (t = X^rot f)."""

    def __init__(self, n, rank, form, t_size=3, f_size=3, res_size=3, key_size=3, dnum=3, dsize=1, base2k=12, rot=0, seed=0, fill=None,
                 fuse=(True, True), small_path=True, batch=BATCH):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        if form == "assign":
            assert t_size == res_size
        if form == "assign_neg":
            assert f_size == res_size
        if form == "rot":
            self.t_size = f_size
        # limbs of the difference container: res (cmux :565, cmux_assign :618), the temporary of cmux_assign_neg (:590-596)
        self.d_size = max(res_size, t_size) if form == "assign_neg" else res_size
        self.cols = rank + 1

    def inputs(self):
        rng = seeded(self.seed)
        self.mat = MatZnx(self.n, self.dnum, self.cols, self.cols, self.key_size).fill_uniform(self.base2k, rng)
        self.t = np.empty((self.batch, self.t_size, self.cols, self.n), dtype=np.int64)
        self.f = np.empty((self.batch, self.f_size, self.cols, self.n), dtype=np.int64)
        for b in range(self.batch):
            for arr in (self.t, self.f):
                arr[b] = VecZnx(self.n, self.cols, arr.shape[1]).fill_uniform(self.base2k, rng).data
                if self.fill is not None:
                    self.fill(b, arr[b], rng)
        return self

    def params(self):
        from poulpy_amd.hal import GlweOpParams
        return GlweOpParams(rank=self.rank, dnum=self.dnum, dsize=self.dsize, key_size=self.key_size, key_base2k=self.base2k, a_size=self.d_size,
                            a_base2k=self.base2k, res_size=self.res_size, res_base2k=self.base2k, rank_out=self.rank)

    def oracle(self, ref, pr):
        want = np.empty((self.batch, self.res_size, self.cols, self.n), dtype=np.int64)
        for b in range(self.batch):
            t = VecZnx(self.n, self.cols, self.t_size, self.t[b].copy())
            f = VecZnx(self.n, self.cols, self.f_size, self.f[b].copy())
            if self.form == "cmux":
                res = VecZnx(self.n, self.cols, self.res_size)
                co.cmux(ref, res, t, f, pr, self.base2k, self.dsize)
            elif self.form == "assign":
                res = t
                co.cmux_assign(ref, res, f, pr, self.base2k, self.dsize)
            elif self.form == "assign_neg":
                res = f
                co.cmux_assign_neg(ref, res, t, pr, self.base2k, self.dsize)
            else:
                res = VecZnx(self.n, self.cols, self.res_size)
                co.cmux_rotated(ref, res, f, self.rot, pr, self.base2k, self.dsize)
            want[b] = res.data
        return want

    def device(self, hip, ph, probe=False):
        """-> (outputs, dispatch notes of the call[, rounding margin])"""
        with on_device(hip, chunk=CHUNK, fuse=self.fuse, small_path=self.small_path) as dev:
            d_f, d_key = dev.upload(self.f), dev.key(ph)
            d_t = dev.upload(self.t) if self.form != "rot" else None
            d_res = {"assign": d_t, "assign_neg": d_f}.get(self.form) or dev.alloc(self.batch * self.res_size * self.cols * self.n * 8)
            hip.sync()

            def run():
                if d_res is d_t:
                    d_t.upload(self.t)
                if d_res is d_f:
                    d_f.upload(self.f)
                hip.glwe_cmux_batched(d_res.ptr, d_t.ptr if d_t else None, d_f.ptr, d_key.ptr, self.params(), self.batch,
                                      t_size=self.t_size, f_size=self.f_size, t_rot=self.rot)
                hip.sync()
            hip.dispatch_notes(reset=True)
            run()
            notes = hip.dispatch_notes()
            shape = (self.batch, self.res_size, self.cols, self.n)
            got = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
            if not probe:
                return got, notes
            margin = hip.rounding_margin_of(run)
            again = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
            assert np.array_equal(again, got), "differs under the margin probe"
            return got, notes, margin


def check(mods, c, note, also=(), absent=()):
    ref, hip = mods(c.n)
    c.inputs()
    pr, ph = prepared_key(ref, hip, c.mat)
    got, notes = c.device(hip, ph)
    label = (c.n, c.rank, c.form, c.t_size, c.f_size, c.res_size, c.key_size, c.dsize, c.base2k, c.rot)
    assert np.array_equal(got, c.oracle(ref, pr)), (label, "device != oracle", notes)
    for s in (note,) + tuple(also):
        assert s in notes, (label, s, notes)
    for s in tuple(absent) + tuple(x for x in (ONE, TWO, MAT) if x != note):
        assert s not in notes, (label, s, notes)
    return got


# route id -> (n, rank, module switches, note, notes that must / must not accompany it)
ROUTES = {
    "n1024-r1-one": (1024, 1, {}, ONE, ("k_small_one",), ("k_mid128",)),
    "n1024-r2-two": (1024, 2, {}, TWO, (), ("k_small_one", "k_mid128")),
    # (rank 1 at N = 2048 has 6 input polynomials: the dispatcher's measured rule sends that to the one-kernel form, launch_small.hip)
    "n2048-r1-one": (2048, 1, {}, ONE, ("k_small_one",), ("k_mid128",)),
    "n2048-r2-two": (2048, 2, {}, TWO, (), ("k_small_one", "k_mid128")),
    "n4096-small-on": (4096, 1, {}, TWO, (), ("k_mid128",)),
    "n4096-small-off": (4096, 1, dict(small_path=False), MAT, ("three-kernel pipeline", "k_mid128"), ()),
    "n8192-fused": (8192, 1, {}, MAT, ("three-kernel pipeline", "k_mid128"), ()),
    "n8192-unfused": (8192, 1, dict(fuse=(False, False)), MAT, ("five-kernel path",), ("k_mid128",)),
    "n256-general": (256, 1, {}, MAT, ("five-kernel path",), ("k_mid128",)),
}
FUSED_ROUTES = ("n1024-r1-one", "n1024-r2-two", "n2048-r1-one", "n2048-r2-two", "n4096-small-on")

# form, sizes: the three forms at equal sizes; res == f with a longer t (d_size > res_size); all sizes different; a key longer than res
FORMS = [
    ("cmux", {}),
    ("assign", {}),
    ("assign_neg", dict(t_size=4)),
    ("cmux", dict(t_size=2, f_size=4, res_size=3)),
    ("cmux", dict(t_size=4, f_size=2, res_size=3, key_size=4)),
    ("assign", dict(f_size=2, key_size=4)),
]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_form_on_every_route(mods, route):
    n, rank, sw, note, also, absent = ROUTES[route]
    for i, (form, sizes) in enumerate(FORMS):
        check(mods, Case(n, rank, form, seed=11000 + 10 * n + i, **sizes, **sw), note, also, absent)


def test_four_limbs_at_n4096_stay_on_the_two_kernels(mods):
    """Rank 1, 4 limbs at N = 4096 (8 polynomials in, 8 out): the plain external product takes the three-kernel pipeline there, the CMUX the two
    small-ring kernels, whose forward stage forms the difference (2.51 against 2.05 M gates / s, profiles/cmux_lines.txt); small path off: the pipeline."""
    sizes = dict(t_size=4, f_size=4, res_size=4, key_size=4, dnum=4)
    for i, form in enumerate(("cmux", "assign", "assign_neg", "rot")):
        check(mods, Case(4096, 1, form, rot=4097, seed=11400 + i, **sizes), TWO, (), ("k_mid128",))
    check(mods, Case(4096, 1, "cmux", seed=11410, small_path=False, **sizes), MAT, ("three-kernel pipeline", "k_mid128"))


@pytest.mark.parametrize("n,note", [(1024, MAT), (8192, MAT)])
def test_dsize_two(mods, n, note):
    """dsize = 2: no small-ring kernel takes it (N = 1024: the five-kernel path), the three-kernel pipeline selects digits in its middle kernel."""
    for form, sizes in (("cmux", {}), ("assign_neg", dict(t_size=5))):
        check(mods, Case(n, 1, form, seed=11500 + n, **{**dict(t_size=4, f_size=4, res_size=4, key_size=5, dnum=2, dsize=2, base2k=13), **sizes}), note)


@pytest.mark.parametrize("route", FUSED_ROUTES + ("n256-general", "n8192-fused"))
def test_rotated_source_at_the_wrap_points(mods, route):
    """t = X^rot f: the sign wraps at N and at 2N; rot = 0 is D = 0 (res = normalize(f)); negative and large exponents are taken mod 2N."""
    n, rank, sw, note, also, absent = ROUTES[route]
    for i, rot in enumerate((1, -1, n // 2, n - 1, n, n + 1, 2 * n - 1, 0, 2 * n + 3, -(n + 2))):
        got = check(mods, Case(n, rank, "rot", rot=rot, seed=12000 + n + i, **sw), note, also, absent)
        if rot == 0:
            c = Case(n, rank, "rot", rot=0, seed=12000 + n + i, **sw).inputs()
            assert np.array_equal(got, c.f)   # normalized f, D = 0: the gate returns f itself
    # res longer / shorter than f
    check(mods, Case(n, rank, "rot", rot=5, f_size=2, res_size=3, seed=12100 + n, **sw), note, also, absent)
    check(mods, Case(n, rank, "rot", rot=n + 7, f_size=4, res_size=3, key_size=4, seed=12101 + n, **sw), note, also, absent)


@pytest.mark.parametrize("base2k,s", [(12, 4), (12, 6), (17, 1)], ids=["k12-sum16", "k12-sum64", "k17-sum2"])
@pytest.mark.parametrize("route", FUSED_ROUTES)
def test_unnormalized_digits_on_the_fused_routes(mods, route, base2k, s):
    """Digits of tests/unnormalized.py on both operands: the difference then spans s + 1 bits more than a normalized digit.  The fused forward
    stage keeps 64-bit integers up to the f64 conversion - no 16- / 32-bit form anywhere on these routes - so base2k 12 and 17 (either side of a
    16-bit digit) and sums past 16 bits take the same code."""
    n, rank, sw, note, also, absent = ROUTES[route]
    fills = [un.sums(base2k, s), un.one_wide(2, base2k, s), un.wide_at("body", base2k, s), un.wide_at("bottom", base2k, s)]
    for i, fill in enumerate(fills):
        for form, extra in (("cmux", {}), ("assign_neg", dict(t_size=4)), ("rot", dict(rot=n - 1))):
            check(mods, Case(n, rank, form, base2k=base2k, fill=fill, seed=13000 + n + 7 * i + base2k, **extra, **sw), note, also, absent)


MARGIN_ROUTES = ["n1024-r1-one", "n1024-r2-two", "n2048-r1-one", "n2048-r2-two", "n4096-small-on", "n4096-small-off", "n8192-fused", "n256-general"]


@pytest.mark.parametrize("route", MARGIN_ROUTES)
def test_rounding_margin_on_uniform_inputs(mods, route):
    """Normalized uniform inputs with the module's rounding-margin probe on: below the suite's limit for uniform inputs."""
    n, rank, sw, note, _, _ = ROUTES[route]
    ref, hip = mods(n)
    worst = 0.0
    for form, extra in (("cmux", {}), ("rot", dict(rot=n // 2 + 1))):
        c = Case(n, rank, form, seed=14000 + n, **extra, **sw).inputs()
        pr, ph = prepared_key(ref, hip, c.mat)
        got, notes, margin = c.device(hip, ph, probe=True)
        assert np.array_equal(got, c.oracle(ref, pr)) and note in notes, (route, form, notes)
        worst = max(worst, margin)
    print(f"[margin] cmux {route}: {worst:.3g}")
    assert worst < MARGIN_MAX, (route, worst)


# ---- POULPY_DBG_CMUX_FUSED=0 in a child process ------------------------------------------------------------------------------------------
def switch_cases():
    out = []
    for route in FUSED_ROUTES:
        n, rank, sw, _, _, _ = ROUTES[route]
        out += [Case(n, rank, "cmux", t_size=4, f_size=2, seed=15000 + n + rank, **sw), Case(n, rank, "assign_neg", t_size=4, seed=15100 + n + rank, **sw),
                Case(n, rank, "assign", seed=15200 + n + rank, **sw), Case(n, rank, "rot", rot=n + 1, seed=15300 + n + rank, **sw)]
    return out


def run_switch_cases():
    """-> ([outputs], [notes]) of switch_cases() on fresh modules (parent and child run the same code)"""
    from oracle.ref import RefModule
    from poulpy_amd.hal import Module
    got, notes, pairs = [], [], {}
    for c in switch_cases():
        if c.n not in pairs:
            pairs[c.n] = (RefModule(c.n), Module(c.n, device=0))
        ref, hip = pairs[c.n]
        c.inputs()
        _, ph = prepared_key(ref, hip, c.mat)
        g, s = c.device(hip, ph)
        got.append(g)
        notes.append(s)
    for _, hip in pairs.values():
        hip.close()
    return got, notes


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_cmux as t
got, notes = t.run_switch_cases()
np.savez(sys.argv[1], *got)
print(json.dumps(notes), flush=True)
"""


def test_switch_sends_every_shape_to_the_materialised_route_with_the_same_digits(tmp_path):
    env = dict(os.environ)
    env.pop("POULPY_DBG_CANARY", None)
    env["POULPY_DBG_CMUX_FUSED"] = "0"
    out = tmp_path / "got.npz"
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(out)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    child_notes = json.loads(r.stdout.strip().splitlines()[-1])
    child = np.load(out)
    got, notes = run_switch_cases()
    from oracle.ref import RefModule
    refs = {}
    for i, c in enumerate(switch_cases()):
        label = (c.n, c.rank, c.form)
        assert (ONE in notes[i] or TWO in notes[i]) and MAT not in notes[i], (label, notes[i])
        assert MAT in child_notes[i] and "POULPY_DBG_CMUX_FUSED=0" in child_notes[i], (label, child_notes[i])
        assert ONE not in child_notes[i] and TWO not in child_notes[i], (label, child_notes[i])
        assert np.array_equal(child["arr_%d" % i], got[i]), (label, "materialised != fused")
        ref = refs.setdefault(c.n, RefModule(c.n))
        c.inputs()
        pr = ref.vmp_pmat_alloc(c.dnum, c.cols, c.cols, c.key_size)
        ref.vmp_prepare(pr, c.mat)
        assert np.array_equal(got[i], c.oracle(ref, pr)), (label, "device != oracle")


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_overlaps_that_are_not_equalities_are_refused_and_launch_nothing(mods):
    from poulpy_amd import abi
    n = 1024
    _, hip = mods(n)
    c = Case(n, 1, "cmux", seed=16000).inputs()
    ct = n * c.cols * 3 * 8
    with on_device(hip) as dev:
        d_t = dev.alloc(c.t.nbytes + ct, poison=False).upload(c.t)
        d_f = dev.alloc(c.f.nbytes + ct, poison=False).upload(c.f)
        d_res = dev.alloc(c.batch * ct)
        d_key = dev.alloc(n * 8 * c.dnum * c.cols * c.cols * c.key_size, poison=False)
        hip.sync()
        p = c.params()

        def call(res, t, f):
            st = hip.lib.pz_glwe_cmux_batched(hip.handle, res, t, 3, 1, f, 3, d_key.ptr, C.byref(p), c.batch)
            return st, hip.lib.pz_last_error().decode()

        def off(buf, k):
            return C.c_void_p(buf.ptr.value + k * ct)
        for label, args in (("res overlaps the tail of t", (off(d_t, 1), d_t.ptr, d_f.ptr)), ("res overlaps the tail of f", (off(d_f, 2), d_t.ptr, d_f.ptr)),
                            ("rotated source, res overlaps f", (off(d_f, 1), None, d_f.ptr)), ("rotated source, res == f", (d_f.ptr, None, d_f.ptr))):
            st, msg = call(*args)
            assert st == abi.PZ_ERR_ALIAS and "overlap" in msg, (label, st, msg)
        host = np.zeros(c.batch * ct // 8, dtype=np.int64)
        st, msg = call(host.ctypes.data_as(C.c_void_p), d_t.ptr, d_f.ptr)
        assert st == abi.PZ_ERR_INVALID and "device pointers" in msg, (st, msg)
        hip.sync()
        assert np.all(d_res.download(np.uint8, d_res.nbytes) == 0x5A)
        assert np.array_equal(d_t.download(np.int64, c.t.size).reshape(c.t.shape), c.t)
        assert np.array_equal(d_f.download(np.int64, c.f.size).reshape(c.f.shape), c.f)
        q = hip.glwe_cmux_workspace_bytes
        assert 0 < q(p, 1) <= q(p, 8) and q(p, 8) == hip.glwe_op_workspace_bytes(p, 8, 0)


def test_batch_zero_and_a_pinned_key(mods):
    n = 1024
    ref, hip = mods(n)
    c = Case(n, 1, "cmux", seed=16100).inputs()
    pr, ph = prepared_key(ref, hip, c.mat)
    want = c.oracle(ref, pr)
    with on_device(hip, chunk=CHUNK) as dev:
        d_t, d_f, d_key = dev.upload(c.t), dev.upload(c.f), dev.key(ph)
        d_res = dev.alloc(want.nbytes)
        hip.glwe_cmux_batched(d_res.ptr, d_t.ptr, d_f.ptr, d_key.ptr, c.params(), 0, t_size=3, f_size=3)
        hip.sync()
        assert np.all(d_res.download(np.uint8, d_res.nbytes) == 0x5A)
        dev.pin(d_key, c.dnum, c.cols, c.cols, c.key_size)
        hip.glwe_cmux_batched(d_res.ptr, d_t.ptr, d_f.ptr, d_key.ptr, c.params(), c.batch, t_size=3, f_size=3)
        hip.sync()
        assert np.array_equal(d_res.download(np.int64, want.size).reshape(want.shape), want)


# ---- under real keys -----------------------------------------------------------------------------------------------------------------------
def _encrypted_case(n, rank, form, bit, sk_key, seed, **sw):
    """t, f = encryptions of per-ciphertext messages under sk; the GGSW of `bit` under sk_key.  -> (case, sk, messages t, messages f)"""
    base2k, size, k_pt = 12, 3, 6
    rng = seeded(seed)
    sk = fhe_sk.ternary_secret(n, rank, rng)
    key_sk = sk if sk_key == "same" else fhe_sk.ternary_secret(n, rank, rng)
    c = Case(n, rank, form, seed=seed, **sw)
    msg = np.zeros(n, dtype=np.int64)
    msg[0] = bit
    c.mat = MatZnx(n, 3, rank + 1, rank + 1, 3, np.ascontiguousarray(fhe_sk.ggsw_encrypt(key_sk, msg, base2k, 3 * base2k, 3, 1, rng)))
    mt, mf = rng.integers(-30, 30, (BATCH, n), dtype=np.int64), rng.integers(-30, 30, (BATCH, n), dtype=np.int64)
    c.t = np.stack([fhe_sk.glwe_encrypt(sk, fhe_sk.encode(mt[b], base2k, k_pt, size), base2k, size * base2k, rng) for b in range(BATCH)])
    c.f = np.stack([fhe_sk.glwe_encrypt(sk, fhe_sk.encode(mf[b], base2k, k_pt, size), base2k, size * base2k, rng) for b in range(BATCH)])
    return c, sk, mt, mf, k_pt


@pytest.mark.parametrize("route", ["n1024-r1-one", "n1024-r2-two", "n256-general"])
def test_decrypt_on_the_device(mods, route):
    """The procedure of tests/test_gpu_core_semantics.py: device == oracle, then every output decrypts exactly to its own plaintext - t under
    GGSW(1), f under GGSW(0) - in every form; a GGSW under another secret goes through the same call, equals the oracle, and does not decrypt."""
    n, rank, sw, note, _, _ = ROUTES[route]
    ref, hip = mods(n)
    for i, (form, bit, sk_key) in enumerate((("cmux", 1, "same"), ("cmux", 0, "same"), ("assign", 1, "same"), ("assign_neg", 0, "same"),
                                             ("assign_neg", 1, "same"), ("cmux", 1, "other"))):
        c, sk, mt, mf, k_pt = _encrypted_case(n, rank, form, bit, sk_key, seed=17000 + n + i, **sw)
        pr, ph = prepared_key(ref, hip, c.mat)
        got, notes = c.device(hip, ph)
        assert np.array_equal(got, c.oracle(ref, pr)) and note in notes, (route, form, bit, sk_key, notes)
        want = mt if bit else mf
        for b in range(BATCH):
            dec = co.decode_i64(fhe_sk.glwe_phase(got[b], sk), c.base2k, k_pt)
            if sk_key == "same":
                assert np.array_equal(dec, want[b]), (route, form, bit, b)
            else:
                assert np.count_nonzero(dec != want[b]) > n // 2, (route, "the negative control decrypts", b)
