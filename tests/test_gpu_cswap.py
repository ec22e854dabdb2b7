"""pz_glwe_cswap_batched and pz_glwe_blind_retrieval_batched against tests/cswap_oracle.py, bit for bit, on every route.

Every swap case is a batch of 3 pairs in waves of 2 (a wave boundary inside the batch), each pair with its own a and b; both are operand and
result.  Routes, with the dispatch note asserted: the one-kernel and two-kernel small-ring forms whose forward stage reads both sources and
whose inverse stage runs both carry chains (N = 1024 / 2048 / 4096), and the materialised difference on the three-kernel pipeline (N = 4096
small path off, N = 8192: two tails over one big value), the five-kernel path (N = 8192 fusion off, N = 256) and - under
POULPY_DBG_CMUX_FUSED=0, in a child process - on the small rings.  Then: dsize 2, un-normalized digits, the rounding margin (printed with
`-s`), the argument checks that need a module, the butterfly network as one composite call (graph replay included), and encrypt / retrieve /
decrypt under real keys with its negative control."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import cmux_oracle as co
from tests import cswap_oracle as cs
from tests import fhe_sk
from tests import unnormalized as un
from tests.cmux_oracle import GRAPHS
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import MARGIN_MAX, seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, TWO, MAT = cs.NOTE_ONE, cs.NOTE_TWO, cs.NOTE_MAT
BATCH, CHUNK = 3, 2


class Case:
    """One call: `batch` pairs (a, b) of a_size / b_size limbs under one GGSW of key_size limbs."""

    def __init__(self, n, rank, a_size=3, b_size=3, key_size=3, dnum=3, dsize=1, base2k=12, seed=0, fill=None, fuse=(True, True), small_path=True,
                 batch=BATCH):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.cols = rank + 1

    def inputs(self):
        rng = seeded(self.seed)
        self.mat = MatZnx(self.n, self.dnum, self.cols, self.cols, self.key_size).fill_uniform(self.base2k, rng)
        self.a = np.empty((self.batch, self.a_size, self.cols, self.n), dtype=np.int64)
        self.b = np.empty((self.batch, self.b_size, self.cols, self.n), dtype=np.int64)
        for i in range(self.batch):
            for arr in (self.a, self.b):
                arr[i] = VecZnx(self.n, self.cols, arr.shape[1]).fill_uniform(self.base2k, rng).data
                if self.fill is not None:
                    self.fill(i, arr[i], rng)
        return self

    def params(self):
        from poulpy_amd.hal import GlweOpParams
        return GlweOpParams(rank=self.rank, dnum=self.dnum, dsize=self.dsize, key_size=self.key_size, key_base2k=self.base2k,
                            a_size=max(self.a_size, self.b_size), a_base2k=self.base2k, res_size=self.a_size, res_base2k=self.base2k, rank_out=self.rank)

    def oracle(self, ref, pr):
        wa, wb = np.empty_like(self.a), np.empty_like(self.b)
        for i in range(self.batch):
            a = VecZnx(self.n, self.cols, self.a_size, self.a[i].copy())
            b = VecZnx(self.n, self.cols, self.b_size, self.b[i].copy())
            cs.cswap(ref, a, b, pr, self.base2k, self.dsize)
            wa[i], wb[i] = a.data, b.data
        return wa, wb

    def device(self, hip, ph, probe=False):
        """-> (a', b', dispatch notes of the call[, rounding margin])"""
        with on_device(hip, chunk=CHUNK, fuse=self.fuse, small_path=self.small_path) as dev:
            d_a, d_b, d_key = dev.upload(self.a), dev.upload(self.b), dev.key(ph)
            hip.sync()

            def run():
                d_a.upload(self.a)
                d_b.upload(self.b)
                hip.glwe_cswap_batched(d_a.ptr, d_b.ptr, d_key.ptr, self.params(), self.batch, a_size=self.a_size, b_size=self.b_size)
                hip.sync()

            def fetch():
                return (d_a.download(np.int64, self.a.size).reshape(self.a.shape), d_b.download(np.int64, self.b.size).reshape(self.b.shape))
            hip.dispatch_notes(reset=True)
            run()
            notes = hip.dispatch_notes()
            ga, gb = fetch()
            if not probe:
                return ga, gb, notes
            margin = hip.rounding_margin_of(run)
            ga2, gb2 = fetch()
            assert np.array_equal(ga2, ga) and np.array_equal(gb2, gb), "differs under the margin probe"
            return ga, gb, notes, margin


def check(mods, c, note, also=(), absent=()):
    ref, hip = mods(c.n)
    c.inputs()
    pr, ph = prepared_key(ref, hip, c.mat)
    ga, gb, notes = c.device(hip, ph)
    wa, wb = c.oracle(ref, pr)
    label = (c.n, c.rank, c.a_size, c.b_size, c.key_size, c.dsize, c.base2k)
    assert np.array_equal(ga, wa), (label, "a': device != oracle", notes)
    assert np.array_equal(gb, wb), (label, "b': device != oracle", notes)
    for s in (note,) + tuple(also):
        assert s in notes, (label, s, notes)
    for s in tuple(absent) + tuple(x for x in (ONE, TWO, MAT) if x != note):
        assert s not in notes, (label, s, notes)
    return ga, gb


# route id -> (n, rank, module switches, note, notes that must / must not accompany it)
ROUTES = {
    "n1024-r1-one": (1024, 1, {}, ONE, ("k_small_one",), ("k_mid128",)),
    "n1024-r2-two": (1024, 2, {}, TWO, (), ("k_small_one", "k_mid128")),
    "n2048-r1-one": (2048, 1, {}, ONE, ("k_small_one",), ("k_mid128",)),
    "n2048-r2-two": (2048, 2, {}, TWO, (), ("k_small_one", "k_mid128")),
    "n4096-small-on": (4096, 1, {}, TWO, (), ("k_mid128",)),
    "n4096-small-off": (4096, 1, dict(small_path=False), MAT, ("three-kernel pipeline", "k_mid128"), ()),
    "n8192-fused": (8192, 1, {}, MAT, ("three-kernel pipeline", "k_mid128"), ()),
    "n8192-unfused": (8192, 1, dict(fuse=(False, False)), MAT, ("five-kernel path",), ("k_mid128",)),
    "n256-general": (256, 1, {}, MAT, ("five-kernel path",), ("k_mid128",)),
}
FUSED_ROUTES = ("n1024-r1-one", "n1024-r2-two", "n2048-r1-one", "n2048-r2-two", "n4096-small-on")

# equal sizes; a longer than b and the reverse; a key longer than the operands (limbs of big beyond b enter its chain negated) and a shorter one
SIZES = [{}, dict(a_size=4, b_size=3), dict(a_size=3, b_size=4), dict(key_size=4), dict(key_size=2)]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_both_outputs_on_every_route(mods, route):
    n, rank, sw, note, also, absent = ROUTES[route]
    for i, sizes in enumerate(SIZES):
        check(mods, Case(n, rank, seed=21000 + 10 * n + i, **sizes, **sw), note, also, absent)


def test_four_limbs_at_n4096_stay_on_the_two_kernels(mods):
    """Rank 1, 4 limbs at N = 4096 (8 polynomials in, 8 out): the swap follows the CMUX's rule there (cmux_fused_route) - the two small-ring
    kernels; small path off: the pipeline."""
    sizes = dict(a_size=4, b_size=4, key_size=4, dnum=4)
    check(mods, Case(4096, 1, seed=21400, **sizes), TWO, (), ("k_mid128",))
    check(mods, Case(4096, 1, seed=21410, small_path=False, **sizes), MAT, ("three-kernel pipeline", "k_mid128"))


@pytest.mark.parametrize("n", [1024, 8192])
def test_dsize_two(mods, n):
    """dsize = 2: no small-ring kernel takes it (N = 1024: the five-kernel path), the three-kernel pipeline selects digits in its middle kernel."""
    for sizes in ({}, dict(a_size=5), dict(b_size=5)):
        check(mods, Case(n, 1, seed=21500 + n, **{**dict(a_size=4, b_size=4, key_size=5, dnum=2, dsize=2, base2k=13), **sizes}), MAT)


@pytest.mark.parametrize("base2k,s", [(12, 4), (12, 6), (17, 1)], ids=["k12-sum16", "k12-sum64", "k17-sum2"])
@pytest.mark.parametrize("route", FUSED_ROUTES)
def test_unnormalized_digits_on_the_fused_routes(mods, route, base2k, s):
    """Digits of tests/unnormalized.py on both operands: the difference spans s + 1 bits more than a normalized digit, and both chains take
    un-normalized operands.  64-bit integers everywhere on these routes, so base2k 12 and 17 and sums past 16 bits take the same code."""
    n, rank, sw, note, also, absent = ROUTES[route]
    fills = [un.sums(base2k, s), un.one_wide(2, base2k, s), un.wide_at("body", base2k, s), un.wide_at("bottom", base2k, s)]
    for i, fill in enumerate(fills):
        check(mods, Case(n, rank, base2k=base2k, fill=fill, seed=23000 + n + 7 * i + base2k, **sw), note, also, absent)


MARGIN_ROUTES = sorted(ROUTES)


@pytest.mark.parametrize("route", MARGIN_ROUTES)
def test_rounding_margin_on_uniform_inputs(mods, route):
    """Normalized uniform inputs with the module's rounding-margin probe on: below the suite's limit for uniform inputs; outputs unchanged."""
    n, rank, sw, note, _, _ = ROUTES[route]
    ref, hip = mods(n)
    c = Case(n, rank, seed=24000 + n, **sw).inputs()
    pr, ph = prepared_key(ref, hip, c.mat)
    ga, gb, notes, margin = c.device(hip, ph, probe=True)
    wa, wb = c.oracle(ref, pr)
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb) and note in notes, (route, notes)
    print(f"[margin] cswap {route}: {margin:.3g}")
    assert margin < MARGIN_MAX, (route, margin)


# ---- POULPY_DBG_CMUX_FUSED=0 in a child process ------------------------------------------------------------------------------------------
def switch_cases():
    out = []
    for route in FUSED_ROUTES:
        n, rank, sw, _, _, _ = ROUTES[route]
        out += [Case(n, rank, seed=25000 + n + rank, **sw), Case(n, rank, a_size=4, seed=25100 + n + rank, **sw),
                Case(n, rank, b_size=4, key_size=4, seed=25200 + n + rank, **sw)]
    return out


def run_switch_cases():
    """-> ([a' and b' flattened into one array per case], [notes]) of switch_cases() on fresh modules (parent and child run the same code)"""
    from oracle.ref import RefModule
    from poulpy_amd.hal import Module
    got, notes, pairs = [], [], {}
    for c in switch_cases():
        if c.n not in pairs:
            pairs[c.n] = (RefModule(c.n), Module(c.n, device=0))
        ref, hip = pairs[c.n]
        c.inputs()
        _, ph = prepared_key(ref, hip, c.mat)
        ga, gb, s = c.device(hip, ph)
        got.append(np.concatenate([ga.ravel(), gb.ravel()]))
        notes.append(s)
    for _, hip in pairs.values():
        hip.close()
    return got, notes


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_cswap as t
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
        label = (c.n, c.rank, c.a_size, c.b_size, c.key_size)
        assert (ONE in notes[i] or TWO in notes[i]) and MAT not in notes[i], (label, notes[i])
        assert MAT in child_notes[i] and "POULPY_DBG_CMUX_FUSED=0" in child_notes[i], (label, child_notes[i])
        assert ONE not in child_notes[i] and TWO not in child_notes[i], (label, child_notes[i])
        assert np.array_equal(child["arr_%d" % i], got[i]), (label, "materialised != fused")
        ref = refs.setdefault(c.n, RefModule(c.n))
        c.inputs()
        pr = ref.vmp_pmat_alloc(c.dnum, c.cols, c.cols, c.key_size)
        ref.vmp_prepare(pr, c.mat)
        wa, wb = c.oracle(ref, pr)
        assert np.array_equal(got[i], np.concatenate([wa.ravel(), wb.ravel()])), (label, "device != oracle")


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_overlaps_and_host_pointers_are_refused_and_launch_nothing(mods):
    from poulpy_amd import abi
    n = 1024
    _, hip = mods(n)
    c = Case(n, 1, seed=26000).inputs()
    ct = n * c.cols * 3 * 8
    with on_device(hip) as dev:
        d_a = dev.alloc(c.a.nbytes + ct, poison=False).upload(c.a)
        d_b = dev.upload(c.b)
        d_key = dev.alloc(n * 8 * c.dnum * c.cols * c.cols * c.key_size, poison=False)
        hip.sync()
        p = c.params()

        def call(a, b):
            st = hip.lib.pz_glwe_cswap_batched(hip.handle, a, 3, b, 3, d_key.ptr, C.byref(p), c.batch)
            return st, hip.lib.pz_last_error().decode()

        def off(buf, k):
            return C.c_void_p(buf.ptr.value + k * ct)
        # (one ciphertext apart: beyond what the pointers alone show at the smallest ring degree - the check needs the module's n)
        for label, args in (("b overlaps the tail of a", (d_a.ptr, off(d_a, 1))), ("a overlaps the tail of b's range", (off(d_a, 2), d_a.ptr)),
                            ("a == b", (d_a.ptr, d_a.ptr))):
            st, msg = call(*args)
            assert st == abi.PZ_ERR_ALIAS and "overlap" in msg, (label, st, msg)
        host = np.zeros(c.batch * ct // 8, dtype=np.int64)
        for args in ((host.ctypes.data_as(C.c_void_p), d_b.ptr), (d_a.ptr, host.ctypes.data_as(C.c_void_p))):
            st, msg = call(*args)
            assert st == abi.PZ_ERR_INVALID and "device pointers" in msg, (st, msg)
        hip.sync()
        assert np.array_equal(d_a.download(np.int64, c.a.size).reshape(c.a.shape), c.a)
        assert np.array_equal(d_b.download(np.int64, c.b.size).reshape(c.b.shape), c.b)
        q = hip.glwe_cswap_workspace_bytes
        assert 0 < q(p, 1) <= q(p, 8) <= q(p, 64) and q(p, 8) == hip.glwe_op_workspace_bytes(p, 8, 0)
        r = hip.glwe_blind_retrieval_workspace_bytes
        assert r(p, 5, 3, 2) == q(p, 2 * 2) and r(p, 8, 3, 2) == q(p, 4 * 2) and r(p, 1, 3, 2) == 0


def test_batch_zero_and_a_pinned_key(mods):
    n = 1024
    ref, hip = mods(n)
    c = Case(n, 1, seed=26100).inputs()
    pr, ph = prepared_key(ref, hip, c.mat)
    wa, wb = c.oracle(ref, pr)
    with on_device(hip, chunk=CHUNK) as dev:
        d_a, d_b, d_key = dev.alloc(c.a.nbytes), dev.alloc(c.b.nbytes), dev.key(ph)
        hip.glwe_cswap_batched(d_a.ptr, d_b.ptr, d_key.ptr, c.params(), 0, a_size=3, b_size=3)
        hip.sync()
        assert np.all(d_a.download(np.uint8, d_a.nbytes) == 0x5A) and np.all(d_b.download(np.uint8, d_b.nbytes) == 0x5A)
        d_a.upload(c.a)
        d_b.upload(c.b)
        dev.pin(d_key, c.dnum, c.cols, c.cols, c.key_size)
        hip.glwe_cswap_batched(d_a.ptr, d_b.ptr, d_key.ptr, c.params(), c.batch, a_size=3, b_size=3)
        hip.sync()
        assert np.array_equal(d_a.download(np.int64, wa.size).reshape(wa.shape), wa)
        assert np.array_equal(d_b.download(np.int64, wb.size).reshape(wb.shape), wb)


# ---- the butterfly network ------------------------------------------------------------------------------------------------------------------
RN, RRANK, RBASE2K, RSIZE, RDNUM, RBATCH, NBITS = 1024, 1, 12, 3, 3, 2, 3


def _rparams():
    from poulpy_amd.hal import GlweOpParams
    return GlweOpParams(rank=RRANK, dnum=RDNUM, dsize=1, key_size=RSIZE, key_base2k=RBASE2K, a_size=RSIZE, a_base2k=RBASE2K, res_size=RSIZE,
                        res_base2k=RBASE2K, rank_out=RRANK)


@pytest.fixture(scope="module")
def network(mods):
    """Three uniform prepared GGSWs (oracle and device form) shared by the network tests."""
    ref, hip = mods(RN)
    rng = seeded(27000)
    keys = [prepared_key(ref, hip, MatZnx(RN, RDNUM, RRANK + 1, RRANK + 1, RSIZE).fill_uniform(RBASE2K, rng)) for _ in range(NBITS)]
    return ref, hip, keys


def _oracle_network(ref, keys, slots, reverse):
    """slots: (nslots, batch, size, cols, n) -> the same after the reference loops on every vector of the batch"""
    want = slots.copy()
    for v in range(slots.shape[1]):
        lst = [VecZnx(RN, RRANK + 1, RSIZE, want[s, v].copy()) for s in range(slots.shape[0])]
        (cs.glwe_blind_retrieval_rev if reverse else cs.glwe_blind_retrieval)(ref, lst, lambda i: keys[i][0], 0, NBITS, RBASE2K)
        for s in range(slots.shape[0]):
            want[s, v] = lst[s].data
    return want


@pytest.mark.parametrize("nslots", [1, 2, 5, 8])
def test_network_equals_the_oracle_and_the_single_calls(network, nslots):
    """Forward, then reverse on the result: bit-identical to the oracle network and to issuing the per-level pz_glwe_cswap_batched calls; a
    slot no level touches is unchanged (nslots = 1: every slot; the oracle comparison covers the rest)."""
    ref, hip, keys = network
    rng = seeded(27100 + nslots)
    slots = np.stack([np.stack([VecZnx(RN, RRANK + 1, RSIZE).fill_uniform(RBASE2K, rng).data for _ in range(RBATCH)]) for _ in range(nslots)])
    p = _rparams()
    slot_bytes = slots[0].nbytes
    with on_device(hip, chunk=CHUNK, graphs=False) as dev:
        d_keys = [dev.key(ph) for _, ph in keys]
        d_net, d_one = dev.upload(slots), dev.upload(slots)
        state = slots
        for reverse in (False, True):
            hip.dispatch_notes(reset=True)
            hip.glwe_blind_retrieval_batched(d_net.ptr, nslots, [k.ptr for k in d_keys], reverse, p, RBATCH)
            hip.sync()
            notes = hip.dispatch_notes()
            for t, bit, cnt in cs.retrieval_levels(nslots, NBITS, reverse):
                if cnt:
                    hip.glwe_cswap_batched(d_one.ptr, C.c_void_p(d_one.ptr.value + t * slot_bytes), d_keys[bit].ptr, p, cnt * RBATCH, a_size=RSIZE, b_size=RSIZE)
            hip.sync()
            got = d_net.download(np.int64, slots.size).reshape(slots.shape)
            state = _oracle_network(ref, keys, state, reverse)
            assert np.array_equal(got, state), (nslots, reverse, "device != oracle")
            assert np.array_equal(d_one.download(np.int64, slots.size).reshape(slots.shape), got), (nslots, reverse, "composite != single calls")
            levels = sum(1 for _, _, cnt in cs.retrieval_levels(nslots, NBITS, reverse) if cnt)
            assert (ONE in notes) == (levels > 0) and TWO not in notes and MAT not in notes, (nslots, notes)   # (a level with cnt == 0 launches nothing)
        if nslots == 1:
            assert np.array_equal(got, slots)


def test_network_nothing_to_do(network):
    """nslots == 0 / nbits == 0 / batch == 0: PZ_OK, the poisoned buffer untouched."""
    _, hip, keys = network
    with on_device(hip) as dev:
        d_keys = [dev.key(ph) for _, ph in keys]
        d = dev.alloc(2 * RBATCH * RSIZE * (RRANK + 1) * RN * 8)
        hip.glwe_blind_retrieval_batched(d.ptr, 0, [k.ptr for k in d_keys], False, _rparams(), RBATCH)
        hip.glwe_blind_retrieval_batched(d.ptr, 2, [], True, _rparams(), RBATCH)
        hip.glwe_blind_retrieval_batched(d.ptr, 2, [k.ptr for k in d_keys], False, _rparams(), 0)
        hip.sync()
        assert np.all(d.download(np.uint8, d.nbytes) == 0x5A)


def test_repeated_network_calls_replay_a_graph_with_new_contents(mods):
    """Four calls with new contents in the same buffers on a module of the test's own: every output bit-exact, and the repeats are served by a
    HIP graph (the first call of a module sizes its workspaces, which are part of the key: the capture may fall on the third call).  Graphs off
    or the canary on: every call plain."""
    from poulpy_amd.hal import Module
    ref, _ = mods(RN)
    hip = Module(RN)
    hip.set_graphs(True)
    rng = seeded(27300)
    keys = [prepared_key(ref, hip, MatZnx(RN, RDNUM, RRANK + 1, RRANK + 1, RSIZE).fill_uniform(RBASE2K, rng)) for _ in range(NBITS)]
    nslots = 5
    with on_device(hip, chunk=CHUNK) as dev:
        d_keys = [dev.key(ph) for _, ph in keys]
        d = dev.alloc(nslots * RBATCH * RSIZE * (RRANK + 1) * RN * 8, poison=False)
        first = hip.graph_launches()
        after = []
        for call in range(4):
            slots = np.stack([np.stack([VecZnx(RN, RRANK + 1, RSIZE).fill_uniform(RBASE2K, rng).data for _ in range(RBATCH)]) for _ in range(nslots)])
            d.upload(slots)
            hip.glwe_blind_retrieval_batched(d.ptr, nslots, [k.ptr for k in d_keys], False, _rparams(), RBATCH)
            hip.sync()
            got = d.download(np.int64, slots.size).reshape(slots.shape)
            assert np.array_equal(got, _oracle_network(ref, keys, slots, False)), ("call", call)
            after.append(hip.graph_launches())
        if GRAPHS:
            assert after[0] == first and after[2] > after[0] and after[3] == after[2] + 1, (first, after)
        else:
            assert after[3] == first
    hip.close()


# ---- under real keys -----------------------------------------------------------------------------------------------------------------------
def test_retrieval_decrypts_on_the_device(mods):
    """swap.rs:93-153 at N = 1024 with 5 slots through poulpy_amd.bdd.glwe_blind_retrieval: for every index slot 0 decrypts to data[idx] and the
    reverse call restores all slots; with one selector bit flipped (to an index that is still in the vector) slot 0 decrypts to that other
    element, not to data[idx]."""
    from poulpy_amd import bdd
    ref, hip = mods(RN)
    rng = seeded(28000)
    k_pt, nslots = 6, 5
    sk = fhe_sk.ternary_secret(RN, RRANK, rng)
    ggsw = {}
    for v in (0, 1):
        msg = np.zeros(RN, dtype=np.int64)
        msg[0] = v
        mat = MatZnx(RN, RDNUM, RRANK + 1, RRANK + 1, RSIZE, np.ascontiguousarray(fhe_sk.ggsw_encrypt(sk, msg, RBASE2K, RSIZE * RBASE2K, RDNUM, 1, rng)))
        ggsw[v] = prepared_key(ref, hip, mat)
    msgs = rng.integers(-30, 30, (nslots, RBATCH, RN), dtype=np.int64)
    slots = np.stack([np.stack([fhe_sk.glwe_encrypt(sk, fhe_sk.encode(msgs[s, v], RBASE2K, k_pt, RSIZE), RBASE2K, RSIZE * RBASE2K, rng)
                                for v in range(RBATCH)]) for s in range(nslots)])
    p = _rparams()

    def dec(ct):
        return co.decode_i64(fhe_sk.glwe_phase(ct, sk), RBASE2K, k_pt)
    with on_device(hip, chunk=CHUNK) as dev:
        d_bit = {v: dev.key(ggsw[v][1]) for v in (0, 1)}
        d = dev.alloc(slots.nbytes, poison=False)
        for idx in range(nslots):
            for flip in [None] + [f for f in range(NBITS) if idx ^ (1 << f) < nslots][:1]:
                k = idx if flip is None else idx ^ (1 << flip)
                bit_ptrs = [d_bit[(k >> i) & 1].ptr for i in range(NBITS)]
                d.upload(slots)
                out = bdd.glwe_blind_retrieval(hip, d.ptr, nslots, bit_ptrs, p, RBATCH)
                hip.sync()
                assert out.value == d.ptr.value
                got = d.download(np.int64, slots.size).reshape(slots.shape)
                want = _oracle_network(ref, [ggsw[(k >> i) & 1] for i in range(NBITS)], slots, False)
                assert np.array_equal(got, want), (idx, flip, "device != oracle")
                for v in range(RBATCH):
                    if flip is None:
                        assert np.array_equal(dec(got[0, v]), msgs[idx, v]), (idx, v)
                    else:   # negative control: the element of the flipped index, not data[idx]
                        assert not np.array_equal(dec(got[0, v]), msgs[idx, v]), (idx, flip, v)
                        assert np.array_equal(dec(got[0, v]), msgs[k, v]), (idx, flip, v)
                if flip is None:
                    bdd.glwe_blind_retrieval(hip, d.ptr, nslots, bit_ptrs, p, RBATCH, reverse=True)
                    hip.sync()
                    back = d.download(np.int64, slots.size).reshape(slots.shape)
                    for s in range(nslots):
                        for v in range(RBATCH):
                            assert np.array_equal(dec(back[s, v]), msgs[s, v]), (idx, s, v, "not restored")
