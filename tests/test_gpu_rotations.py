"""pz_glwe_automorphism_many_batched: one ciphertext batch rotated by many Galois elements in one call.

Every case is bit-exact against RefModule.glwe_automorphism per rotation and keeps its own random MatZnx key per rotation, so that a mixed-up
key or block index shows.  The hoisted route (pass 1 and the read of the body column once per wave) and the per-rotation loop are told apart
by the dispatch note; with kernel timing on, the launch count of the fwd_pass1 class shows that pass 1 ran once per wave.

The a_base2k != key_base2k case rides on the hoisted route (the shared pass 1 normalizes `a` into the key's base once): its note says so.
The workspace query needs a module, hence a device: its monotonicity is checked here, not in tests/test_rotations_host.py."""
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOISTED, LOOP = "rotations: hoisted", "rotations: per-rotation calls"
CAP = 8   # k_automorphism_t16_many takes this many Galois elements per launch (device_ops.hpp kAutoManyCap)


def inputs(n, rank, a_size, a_base2k, key_size, key_base2k, dnum, dsize, res_size, res_base2k, batch, gals, seed, wide=None):
    """Random ciphertext digits and one random key per rotation.  wide = (ciphertext, bits): that ciphertext's digits are drawn from
    +-2^(bits-1) (an un-normalized input)."""
    rng = seeded(seed)
    cols = rank + 1
    mats = [MatZnx(n, dnum, rank, cols, key_size).fill_uniform(key_base2k, rng) for _ in gals]
    a = np.empty((batch, a_size, cols, n), dtype=np.int64)
    for b in range(batch):
        a[b] = VecZnx(n, cols, a_size).fill_uniform(a_base2k, rng).data
        if wide is not None and b == wide[0]:
            a[b] = rng.integers(-(1 << (wide[1] - 1)), 1 << (wide[1] - 1), a[b].shape, dtype=np.int64)
    return SimpleNamespace(n=n, rank=rank, cols=cols, a_size=a_size, a_base2k=a_base2k, key_size=key_size, key_base2k=key_base2k, dnum=dnum,
                           dsize=dsize, res_size=res_size, res_base2k=res_base2k, batch=batch, gals=[g % (2 * n) for g in gals], mats=mats, a=a)


def simple(n, rank, limbs, base2k, batch, gals, seed, wide=None):
    """one base2k for input, keys and output; dnum = limbs, dsize 1"""
    return inputs(n, rank, limbs, base2k, limbs, base2k, limbs, 1, limbs, base2k, batch, gals, seed, wide=wide)


def oracle(ref, c, rots=None):
    """want[r][b] = glwe_automorphism(a[b], key r, gal r), computed once per case"""
    rots = range(len(c.gals)) if rots is None else rots
    want = np.empty((len(c.gals), c.batch, c.res_size, c.cols, c.n), dtype=np.int64)
    for r in rots:
        pr = ref.vmp_pmat_alloc(c.dnum, c.rank, c.cols, c.key_size)
        ref.vmp_prepare(pr, c.mats[r])
        for b in range(c.batch):
            a = VecZnx(c.n, c.cols, c.a_size, np.ascontiguousarray(c.a[b]))
            res = VecZnx(c.n, c.cols, c.res_size)
            ref.glwe_automorphism(res, c.res_base2k, a, c.a_base2k, pr, c.dsize, c.key_base2k, c.gals[r], "automorphism")
            want[r, b] = res.data
    return want


def params(c):
    from poulpy_amd.hal import GlweOpParams
    return GlweOpParams(rank=c.rank, dnum=c.dnum, dsize=c.dsize, key_size=c.key_size, key_base2k=c.key_base2k, a_size=c.a_size,
                        a_base2k=c.a_base2k, res_size=c.res_size, res_base2k=c.res_base2k, rank_out=c.rank)


def run_device(hip, c, chunk=0, fuse=(True, True), pin=(), probe=False, single=False):
    """One call on the case -> (outputs [rotation][ciphertext], notes, fwd_pass1 launches of the call, workspace query, workspace allocated).
    pin: the rotations whose key is pinned first.  single: nrot calls of glwe_automorphism_batched instead."""
    p = params(c)
    nrot = len(c.gals)
    shape = (nrot, c.batch, c.res_size, c.cols, c.n)
    nbytes = int(np.prod(shape)) * 8
    with on_device(hip, chunk=chunk, fuse=fuse) as dev:
        d_keys = []
        for m in c.mats:
            ph = hip.vmp_pmat_alloc(c.dnum, c.rank, c.cols, c.key_size)
            hip.vmp_prepare(ph, m)
            d_keys.append(dev.key(ph))
        d_a, d_res = dev.upload(c.a), dev.alloc(nbytes)
        for r in pin:
            dev.pin(d_keys[r], c.dnum, c.rank, c.cols, c.key_size)
        query = hip.glwe_automorphism_many_workspace_bytes(p, nrot, c.batch)
        hip.sync()
        hip.dispatch_notes(reset=True)
        with on_device(hip, timing=True, probe=probe):
            before = hip.kernel_stats()["fwd_pass1"][0]
            if single:
                for r in range(nrot):
                    hip.glwe_automorphism_batched(d_res.at(r * nbytes // nrot), d_a.ptr, d_keys[r].ptr, p, c.gals[r], "automorphism", c.batch)
            else:
                hip.glwe_automorphism_many_batched(d_res.ptr, d_a.ptr, c.gals, [k.ptr for k in d_keys], p, c.batch)
            hip.sync()
            pass1 = hip.kernel_stats()["fwd_pass1"][0] - before
            got = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
            notes = hip.dispatch_notes()
            used = hip.workspace_bytes()
    return got, notes, pass1, query, used


def main_inputs():
    """the shape most tests share: N = 8192, rank 1, 3 limbs, base2k 12, 4 ciphertexts; p = 1 and 3 mod 4, a large element, conjugation"""
    n = 8192
    return simple(n, 1, 3, 12, 4, [5, 3, 5 ** 7 % (2 * n), 2 * n - 1], seed=9001)


@pytest.fixture(scope="module")
def main(mods):
    """the shared case, its oracle (computed once) and its hoisted run in two waves"""
    c = main_inputs()
    ref, hip = mods(c.n)
    c.want = oracle(ref, c)
    c.got, c.notes, c.pass1, c.query, c.used = run_device(hip, c, chunk=2)
    return c


def test_hoisted_route_several_waves(main):
    assert np.array_equal(main.got, main.want)
    assert HOISTED in main.notes and LOOP not in main.notes, main.notes
    assert "PERM=1" in main.notes and "16-bit body operand" in main.notes, main.notes
    assert main.pass1 == 2, ("pass 1 once per wave, not once per rotation and wave", main.pass1)


@pytest.mark.parametrize("rank,base2k,batch", [(2, 13, 3), (1, 16, 4)], ids=["rank2-two-bodyless-columns", "key-base-16"])
def test_hoisted_route_rank_2_and_widest_base(mods, rank, base2k, batch):
    n = 8192
    ref, hip = mods(n)
    c = simple(n, rank, 3, base2k, batch, [5, 3, 5 ** 7 % (2 * n), 2 * n - 1], seed=9100 + base2k)
    got, notes, pass1, _, _ = run_device(hip, c, chunk=2)
    assert np.array_equal(got, oracle(ref, c))
    assert HOISTED in notes and pass1 == 2, (notes, pass1)


@pytest.mark.parametrize("wide", [(1, 20), (2, 17)], ids=["20-bit-wave0", "17-bit-wave1"])
def test_wide_inputs_take_the_i64_fallback_per_wave(mods, wide):
    """one ciphertext beyond 16 bits: its wave runs every rotation on the i64 fallback, the other wave on the copies"""
    n = 8192
    ref, hip = mods(n)
    c = simple(n, 1, 3, 12, 4, [5, 3, 2 * n - 1], seed=9200 + wide[1], wide=wide)
    got, notes, pass1, _, _ = run_device(hip, c, chunk=2)
    want = oracle(ref, c)
    for r in range(len(c.gals)):
        for b in range(c.batch):
            assert np.array_equal(got[r, b], want[r, b]), (wide, "rotation", r, "ciphertext", b)
    assert HOISTED in notes and pass1 == 2, (notes, pass1)


def test_large_ring(mods):
    n = 65536
    ref, hip = mods(n)
    c = simple(n, 1, 4, 12, 2, [5 ** 9 % (2 * n), 3], seed=9300)
    got, notes, pass1, _, _ = run_device(hip, c)
    assert np.array_equal(got, oracle(ref, c))
    assert HOISTED in notes and pass1 == 1, (notes, pass1)


def test_n4096_three_kernel_pipeline(mods):
    """more than 4 key limbs: not the two-kernel path.  This plan has no 16-bit-operand tail: pass 1 is shared, the body operand is i64 per rotation."""
    n = 4096
    ref, hip = mods(n)
    c = simple(n, 1, 5, 12, 3, [5, 3, 2 * n - 1], seed=9400)
    got, notes, pass1, _, _ = run_device(hip, c, chunk=2)
    assert np.array_equal(got, oracle(ref, c))
    assert HOISTED in notes and "k_mid128" in notes and pass1 == 2, (notes, pass1)


def test_key_slicing_pinned_unpinned_and_mixed(mods, main):
    ref, hip = mods(main.n)
    for pin in (range(len(main.gals)), (1, 3)):
        got, notes, _, _, _ = run_device(hip, main, chunk=2, pin=tuple(pin))
        assert np.array_equal(got, main.got), ("pinned", tuple(pin))
        assert HOISTED in notes, notes


def test_one_rotation_equals_the_single_call(mods):
    n = 8192
    ref, hip = mods(n)
    c = simple(n, 1, 3, 12, 3, [5 ** 5 % (2 * n)], seed=9500)
    many, notes, _, _, _ = run_device(hip, c, chunk=2)
    one, _, pass1, _, _ = run_device(hip, c, chunk=2, single=True)
    assert np.array_equal(many, one) and np.array_equal(many, oracle(ref, c))
    assert LOOP in notes and "one rotation" in notes and pass1 == 2, notes   # nothing to share: routed to the single call (measured)
    assert hip.glwe_automorphism_many_workspace_bytes(params(c), 1, c.batch) >= hip.glwe_op_workspace_bytes(params(c), c.batch, 2)


def test_more_rotations_than_one_launch_of_the_pre_pass_takes(mods):
    n = 8192
    ref, hip = mods(n)
    gals = [pow(5, k, 2 * n) for k in range(1, CAP + 1)] + [2 * n - 1]
    c = simple(n, 1, 2, 12, 2, gals, seed=9600)
    got, notes, pass1, _, _ = run_device(hip, c)
    want = oracle(ref, c)
    for r in range(len(gals)):
        assert np.array_equal(got[r], want[r]), ("rotation", r)
    assert HOISTED in notes and pass1 == 1, (notes, pass1)


def test_a_in_another_base_is_normalized_once(mods):
    """a_base2k = 15 against key_base2k = 12: the shared input step re-expresses `a` in the key's base a single time"""
    n = 8192
    ref, hip = mods(n)
    c = inputs(n, 1, 3, 15, 4, 12, 4, 1, 4, 12, 3, [5, 3], seed=9700)
    got, notes, pass1, _, _ = run_device(hip, c, chunk=2)
    assert np.array_equal(got, oracle(ref, c))
    assert HOISTED in notes and pass1 == 2, (notes, pass1)


FALLBACKS = {
    "n1024": dict(c=lambda: simple(1024, 1, 3, 12, 3, [5, 3], seed=9801)),
    "fusion-off": dict(c=lambda: simple(8192, 1, 3, 12, 3, [5, 3], seed=9802), fuse=(False, False)),
    "res-base-differs": dict(c=lambda: inputs(8192, 1, 3, 12, 3, 12, 3, 1, 3, 13, 3, [5, 3], seed=9803)),
    "dsize2": dict(c=lambda: inputs(8192, 1, 4, 13, 5, 13, 2, 2, 4, 13, 3, [5, 3], seed=9804)),
    "margin-probe": dict(c=lambda: simple(8192, 1, 3, 12, 3, [5, 3], seed=9805), probe=True),
    "key-base-17": dict(c=lambda: simple(8192, 1, 3, 17, 3, [5, 3], seed=9806)),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallback_routes(mods, name):
    spec = dict(FALLBACKS[name])
    c = spec.pop("c")()
    ref, hip = mods(c.n)
    got, notes, pass1, _, _ = run_device(hip, c, chunk=2, **spec)
    assert np.array_equal(got, oracle(ref, c)), name
    assert LOOP in notes and HOISTED not in notes, (name, notes)


def test_workspace_query_is_monotone(mods, main):
    _, hip = mods(main.n)
    p = params(main)
    q = hip.glwe_automorphism_many_workspace_bytes
    assert 0 < q(p, 1, 4) <= q(p, 2, 4) <= q(p, 8, 4) <= q(p, 9, 4)
    assert q(p, 4, 1) <= q(p, 4, 2) <= q(p, 4, 64)
    assert q(p, 1, 4) >= hip.glwe_op_workspace_bytes(p, 4, 2)
    assert q(p, 0, 4) == 0


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from poulpy_amd.hal import Module
from tests import test_gpu_rotations as t
c = t.main_inputs()
hip = Module(c.n, device=0)
got, notes, pass1, query, used = t.run_device(hip, c, chunk=2)
np.save(sys.argv[1], got)
print(json.dumps(dict(notes=notes, pass1=pass1, query=query, used=used)), flush=True)
"""


def _child(tmp_path, **env_add):
    env = dict(os.environ)
    for k in ("POULPY_DBG_ROT_HOIST", "POULPY_DBG_CANARY"):
        env.pop(k, None)
    env.update(env_add)
    out = tmp_path / "got.npy"
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(out)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return np.load(out), json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_switch_forces_the_loop_with_the_same_bits(main, tmp_path):
    got, info, _ = _child(tmp_path, POULPY_DBG_ROT_HOIST="0")
    assert np.array_equal(got, main.got)
    assert "per-rotation" in info["notes"] and HOISTED not in info["notes"], info
    assert info["pass1"] == 2 * len(main.gals)


def test_hoisted_route_under_workspace_guards(main, tmp_path):
    got, info, err = _child(tmp_path, POULPY_DBG_CANARY="1")
    assert "WORKSPACE OVERRUN" not in err
    assert np.array_equal(got, main.got)
    assert HOISTED in info["notes"], info
    assert 0 < info["used"] <= info["query"], info


def test_argument_errors_launch_nothing(mods):
    n = 8192
    _, hip = mods(n)
    c = simple(n, 1, 3, 12, 2, [5, 3], seed=9900)
    p = params(c)
    ct = c.n * c.cols * c.res_size * 8
    with on_device(hip) as dev:
        d_a = dev.alloc(c.a.nbytes + ct, poison=False).upload(np.ascontiguousarray(c.a))
        d_res = dev.alloc(2 * c.batch * ct)
        d_key = dev.alloc(c.n * 8 * c.dnum * c.rank * c.cols * c.key_size, poison=False)
        hip.sync()

        def call(res, gals, keys):
            g = (C.c_int64 * max(len(gals), 1))(*gals)
            k = (C.c_void_p * max(len(keys), 1))(*keys)
            st = hip.lib.pz_glwe_automorphism_many_batched(hip.handle, res, d_a.ptr, len(gals), g, k, C.byref(p), c.batch)
            return st, hip.lib.pz_last_error().decode()

        key = d_key.ptr.value
        tail = C.c_void_p(d_a.ptr.value + c.a.nbytes - ct)     # the last ciphertext of `a`
        for label, args in (("nrot = 0", (d_res.ptr, [], [])), ("even element", (d_res.ptr, [5, 4], [key, key])),
                            ("null key", (d_res.ptr, [5, 3], [key, 0])), ("res == a", (d_a.ptr, [5, 3], [key, key])),
                            ("res overlaps the tail of a", (tail, [5, 3], [key, key]))):
            st, msg = call(*args)
            assert st < 0 and msg, (label, st, msg)
        hip.sync()
        assert np.all(d_res.download(np.uint8, d_res.nbytes) == 0x5A)
        assert np.array_equal(d_a.download(np.int64, c.a.size).reshape(c.a.shape), c.a)
