"""pz_bdd_circuit_execute_batched against tests/bdd_oracle.py, bit for bit, on every route.

The circuit of most tests is bdd_oracle.hand_circuit(): every node kind, stale slots, hi == lo, outputs of depth 1, 2 and 5 and a zero output,
run with one output slot more than the circuit has.  Every input of a batch has its own GGSWs (uniform digits), except that one input shares
a pointer with another.  Routes, with the dispatch note asserted: one gathered launch per level on the one-kernel and the two-kernel
small-ring forms (N = 1024 / 2048 / 4096) and the gate-by-gate walk on the existing kernels (N = 256, N = 8192, and - under
POULPY_DBG_BDD_GATHER=0, in a child process - the small rings).  Then: pinned, unpinned and host keys; graph replay with new keys behind
the same arguments; the rounding margin (printed with `-s`); the refusals; and an encrypted 3-bit addition decrypted under real keys."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from poulpy_amd import bdd
from poulpy_amd.layouts import MatZnx
from tests import bdd_oracle as bo
from tests import cmux_oracle as co
from tests import fhe_sk
from tests.cmux_oracle import GRAPHS
from tests.device import mods, on_device, prepared_key  # noqa: F401
from tests.helpers import MARGIN_MAX, seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, TWO, GATE = bo.NOTE_ONE, bo.NOTE_TWO, bo.NOTE_GATE
CHUNK = 4          # gates x inputs per wave: level 0 of the hand-made circuit at batch 3 is 3 waves, the last one short
NKEYS = 6          # distinct GGSWs of a case
HAND = bo.hand_circuit()
ADDER2 = bdd.from_truth_table(lambda x: (x & 3) + (x >> 2), 4, 3, [0, 2, 1, 3])

# route id -> (n, rank, base2k, dnum, note)
SHAPES = {
    "n1024-r1-one": (1024, 1, 12, 3, ONE),
    "n1024-r2-two": (1024, 2, 12, 3, TWO),
    "n2048-r1-one": (2048, 1, 12, 3, ONE),
    "n4096-small-on": (4096, 1, 12, 3, TWO),
    "n256-general": (256, 1, 12, 3, GATE),
    "n256-r2-k13-dnum2": (256, 2, 13, 2, GATE),   # rank, base and rows of the reference's own test of the evaluator
    "n8192-fused": (8192, 1, 12, 3, GATE),
}
GATHERED = ("n1024-r1-one", "n1024-r2-two", "n2048-r1-one", "n4096-small-on")
SIZE = 3


def key_of(b, i, variant=0):
    """which of the NKEYS GGSWs is input bit i of input b: every input its own mix; input 2 shares bit 0 with input 0"""
    return (5 * b + 2 * i + 3 * variant + (b * i) % 3) % NKEYS if not (b == 2 and i == 0) else key_of(0, 0, variant)


class Case:
    """One shape: NKEYS uniform GGSWs prepared for the oracle and the device, and the oracle's outputs, computed once per (circuit, batch)."""

    def __init__(self, route, ref, hip):
        self.route = route
        self.n, self.rank, self.base2k, self.dnum, self.note = SHAPES[route]
        self.cols = self.rank + 1
        self.ref, self.hip = ref, hip
        rng = seeded(31000 + sorted(SHAPES).index(route))
        self.keys = [prepared_key(ref, hip, MatZnx(self.n, self.dnum, self.cols, self.cols, SIZE).fill_uniform(self.base2k, rng)) for _ in range(NKEYS)]
        self._want = {}

    def params(self, **kw):
        from poulpy_amd.hal import GlweOpParams
        d = dict(rank=self.rank, dnum=self.dnum, dsize=1, key_size=SIZE, key_base2k=self.base2k, a_size=SIZE, a_base2k=self.base2k, res_size=SIZE,
                 res_base2k=self.base2k, rank_out=self.rank)
        d.update(kw)
        return GlweOpParams(**d)

    def table(self, circuit, batch, variant=0):
        return [[key_of(b, i, variant) for i in range(circuit.input_size)] for b in range(batch)]

    def want(self, name, circuit, batch, n_out, variant=0):
        key = (name, batch, n_out, variant)
        if key not in self._want:
            bits = [[self.keys[k][0] for k in row] for row in self.table(circuit, batch, variant)]
            self._want[key] = bo.execute_batch(self.ref, circuit, bits, n_out, self.cols, SIZE, self.base2k)
            self._want[key].setflags(write=False)
        return self._want[key]

    def device(self, circuit, batch, n_out, variant=0, pin=False, host_keys=False, probe=False, **switches):
        """-> (out (n_out, batch, size, cols, n), dispatch notes[, rounding margin])"""
        hip = self.hip
        switches.setdefault("chunk", CHUNK)
        with on_device(hip, **switches) as dev:
            if host_keys:
                ptrs = [C.c_void_p(ph.data.ctypes.data) for _, ph in self.keys]
            else:
                d_keys = [dev.key(ph) for _, ph in self.keys]
                ptrs = [k.ptr for k in d_keys]
                if pin:
                    for k in d_keys:
                        dev.pin(k, self.dnum, self.cols, self.cols, SIZE)
            h = hip.bdd_circuit_new(circuit)
            try:
                p = self.params()
                d_out = dev.alloc(n_out * batch * SIZE * self.cols * self.n * 8)
                d_tmp = dev.alloc(max(hip.bdd_circuit_execute_tmp_bytes(h, p, batch), 8))
                bits = [[ptrs[k] for k in row] for row in self.table(circuit, batch, variant)]
                hip.sync()

                def run():
                    hip.bdd_circuit_execute_batched(h, d_out.ptr, n_out, bits, p, d_tmp.ptr, d_tmp.nbytes, batch)
                    hip.sync()

                def fetch():
                    return d_out.download(np.int64, d_out.nbytes // 8).reshape(n_out, batch, SIZE, self.cols, self.n)
                hip.dispatch_notes(reset=True)
                run()
                notes = hip.dispatch_notes()
                got = fetch()
                if not probe:
                    return got, notes
                margin = hip.rounding_margin_of(run)
                assert np.array_equal(fetch(), got), "differs under the margin probe"
                return got, notes, margin
            finally:
                hip.bdd_circuit_free(h)


@pytest.fixture(scope="module")
def cases(mods):
    cache = {}

    def get(route):
        if route not in cache:
            cache[route] = Case(route, *mods(SHAPES[route][0]))
        return cache[route]
    return get


def assert_route(notes, note, label):
    assert note in notes, (label, note, notes)
    for other in (ONE, TWO, GATE):
        if other != note:
            assert other not in notes, (label, other, notes)


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("route", sorted(SHAPES))
def test_parity_on_every_route(cases, route, batch):
    c = cases(route)
    circuits = [("hand", HAND)] + ([("adder2", ADDER2)] if c.n < 4096 else [])
    for name, circuit in circuits:
        n_out = circuit.output_size + 1
        got, notes = c.device(circuit, batch, n_out)
        want = c.want(name, circuit, batch, n_out)
        assert np.array_equal(got, want), (route, name, batch, "device != oracle", notes, [int(np.any(got[o] != want[o])) for o in range(n_out)])
        assert_route(notes, c.note, (route, name, batch))
        assert not got[n_out - 1].any() and (name != "hand" or not got[1].any())      # the slot beyond output_size and the zero output
        assert hip_clean(c.hip)


def hip_clean(hip):
    """the workspace guards are intact (POULPY_DBG_CANARY arms them; a clean call returns PZ_OK either way)"""
    return hip.lib.pz_debug_workspace_overrun(hip.handle, 1 << 12, 0) == 0


def test_compare_notices_one_swapped_selector(cases):
    """Negative control of the parity test: the oracle's walk of the same circuit with ONE gate's selector exchanged for another input bit gives
    other digits than the device - on the output that gate feeds, and on no other."""
    c = cases("n1024-r1-one")
    n_out = HAND.output_size + 1
    got, _ = c.device(HAND, 3, n_out)
    nodes, s = HAND.outputs[3]
    swapped = list(nodes)
    assert swapped[1] == (bdd.CMUX, 1, 1, 0)
    swapped[1] = (bdd.CMUX, 2, 1, 0)
    other = bdd.Circuit(HAND.input_size, HAND.outputs[:3] + [(swapped, s)])
    bits = [[c.keys[k][0] for k in row] for row in c.table(HAND, 3)]
    want = bo.execute_batch(c.ref, other, bits, n_out, c.cols, SIZE, c.base2k)
    assert not np.array_equal(got, want) and not np.array_equal(got[3], want[3])
    assert np.array_equal(got[:3], want[:3]) and np.array_equal(got, c.want("hand", HAND, 3, n_out))


# ---- POULPY_DBG_BDD_GATHER=0 in a child process ----------------------------------------------------------------------------------------------
def run_switch_cases():
    """-> ([out per gathered shape], [notes]) on fresh modules (parent and child run the same code)"""
    from oracle.ref import RefModule
    from poulpy_amd.hal import Module
    got, notes = [], []
    for route in GATHERED:
        n = SHAPES[route][0]
        ref, hip = RefModule(n), Module(n, device=0)
        g, s = Case(route, ref, hip).device(HAND, 3, HAND.output_size + 1)
        got.append(g)
        notes.append(s)
        hip.close()
    return got, notes


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_bdd as t
got, notes = t.run_switch_cases()
np.savez(sys.argv[1], *got)
print(json.dumps(notes), flush=True)
"""


def test_switch_sends_every_shape_to_the_per_gate_route_with_the_same_digits(cases, tmp_path):
    env = dict(os.environ)
    env.pop("POULPY_DBG_CANARY", None)
    env["POULPY_DBG_BDD_GATHER"] = "0"
    out = tmp_path / "got.npz"
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(out)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    child_notes = json.loads(r.stdout.strip().splitlines()[-1])
    child = np.load(out)
    for i, route in enumerate(GATHERED):
        c = cases(route)
        got, notes = c.device(HAND, 3, HAND.output_size + 1)
        assert_route(notes, c.note, route)
        assert_route(child_notes[i], GATE, route)
        assert "POULPY_DBG_BDD_GATHER=0" in child_notes[i], (route, child_notes[i])
        assert np.array_equal(child["arr_%d" % i], got), (route, "per-gate != gathered")
        assert np.array_equal(got, c.want("hand", HAND, 3, HAND.output_size + 1)), (route, "device != oracle")


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["n1024-r1-one", "n4096-small-on", "n256-general"])
def test_pinned_unpinned_and_host_keys_give_the_same_digits(cases, route):
    c = cases(route)
    n_out = HAND.output_size + 1
    want = c.want("hand", HAND, 3, n_out)
    for kw in (dict(pin=True), dict(host_keys=True), dict()):
        got, notes = c.device(HAND, 3, n_out, **kw)
        assert np.array_equal(got, want), (route, kw)
        assert_route(notes, c.note, (route, kw))


def test_more_host_keys_than_a_module_mirrors_are_refused(cases):
    """A module mirrors at most 64 host-resident keys and frees the least recently used one beyond that.  xor(4) selects all 8 input bits: batch 8 with a
    host GGSW of its own per (input, bit) is 64 mirrors - it runs, and equals the oracle; batch 9 is 72, which cannot all stay mirrored while the call
    is issued - refused with PZ_ERR_UNSUPPORTED, out untouched.  The same 72 keys on the device are fine."""
    from poulpy_amd import abi
    c = cases("n1024-r1-one")
    hip, ref = c.hip, c.ref
    circuit = bdd.xor(4)
    nbits, n_out = circuit.input_size, circuit.output_size
    rng = seeded(33000)
    keys = [prepared_key(ref, hip, MatZnx(c.n, c.dnum, c.cols, c.cols, SIZE).fill_uniform(c.base2k, rng)) for _ in range(9 * nbits)]
    p = c.params()
    want = bo.execute_batch(ref, circuit, [[keys[b * nbits + i][0] for i in range(nbits)] for b in range(9)], n_out, c.cols, SIZE, c.base2k)
    ct = SIZE * c.cols * c.n
    with on_device(hip, chunk=CHUNK) as dev:
        h = hip.bdd_circuit_new(circuit)
        d_out = dev.alloc(n_out * 9 * ct * 8)
        d_tmp = dev.alloc(hip.bdd_circuit_execute_tmp_bytes(h, p, 9))
        host = [[C.c_void_p(keys[b * nbits + i][1].data.ctypes.data) for i in range(nbits)] for b in range(9)]

        def fetch(batch):
            return d_out.download(np.int64, n_out * batch * ct).reshape(n_out, batch, SIZE, c.cols, c.n)
        flat = (C.c_void_p * (9 * nbits))(*[k.value for row in host for k in row])
        st = hip.lib.pz_bdd_circuit_execute_batched(hip.handle, h, d_out.ptr, n_out, flat, nbits, C.byref(p), d_tmp.ptr, d_tmp.nbytes, 9)
        msg = hip.lib.pz_last_error().decode()
        assert st == abi.PZ_ERR_UNSUPPORTED and "72 distinct host-resident GGSWs" in msg, (st, msg)
        hip.sync()
        assert np.all(d_out.download(np.uint8, d_out.nbytes) == 0x5A), "the refused call wrote to out"
        hip.bdd_circuit_execute_batched(h, d_out.ptr, n_out, host[:8], p, d_tmp.ptr, d_tmp.nbytes, 8)
        hip.sync()
        assert np.array_equal(fetch(8), want[:, :8]), "64 host keys"
        on_dev = [[dev.key(keys[b * nbits + i][1]).ptr for i in range(nbits)] for b in range(9)]
        hip.bdd_circuit_execute_batched(h, d_out.ptr, n_out, on_dev, p, d_tmp.ptr, d_tmp.nbytes, 9)
        hip.sync()
        assert np.array_equal(fetch(9), want), "72 device keys"
        hip.bdd_circuit_free(h)


# ---- graph -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["n1024-r1-one", "n1024-r2-two", "n256-general"])
def test_repeated_calls_replay_a_graph_and_new_keys_are_picked_up(mods, route):
    """A module of the test's own.  Calls 0 - 3 repeat one argument set: every output exact, the repeats served by a HIP graph (the first call
    sizes the workspaces, which are part of the key: the capture may fall on the third call).  Call 4: OTHER GGSWs behind a fresh bits array, same
    out and tmp - on the gathered routes the same graph, fed through tmp.  Call 5: another out.  Then graphs off: the same digits."""
    from poulpy_amd.hal import Module
    n = SHAPES[route][0]
    ref, _ = mods(n)
    hip = Module(n)
    hip.set_graphs(True)
    c = Case(route, ref, hip)
    batch, n_out = 3, HAND.output_size + 1
    want0, want1 = c.want("hand", HAND, batch, n_out), c.want("hand", HAND, batch, n_out, variant=1)
    assert not np.array_equal(want0, want1)
    shape = want0.shape
    with on_device(hip, chunk=CHUNK) as dev:
        ptrs = [dev.key(ph).ptr for _, ph in c.keys]
        h = hip.bdd_circuit_new(HAND)
        p = c.params()
        d_out, d_out2 = dev.alloc(want0.nbytes), dev.alloc(want0.nbytes)
        d_tmp = dev.alloc(hip.bdd_circuit_execute_tmp_bytes(h, p, batch))

        def call(out, variant):
            hip.lib.pz_memset_d(hip.handle, out.ptr, 0x5A, out.nbytes)
            bits = [[ptrs[k] for k in row] for row in c.table(HAND, batch, variant)]
            hip.bdd_circuit_execute_batched(h, out.ptr, n_out, bits, p, d_tmp.ptr, d_tmp.nbytes, batch)
            hip.sync()
            return out.download(np.int64, want0.size).reshape(shape)
        first = hip.graph_launches()
        after = []
        for i in range(4):
            assert np.array_equal(call(d_out, 0), want0), (route, "call", i)
            after.append(hip.graph_launches())
        assert np.array_equal(call(d_out, 1), want1), (route, "other keys behind a fresh bits array")
        other_keys = hip.graph_launches()
        assert np.array_equal(call(d_out2, 0), want0), (route, "another out")
        assert np.array_equal(call(d_out, 0), want0), (route, "back to the first argument set")
        if GRAPHS:
            assert after[0] == first and after[2] > after[0] and after[3] == after[2] + 1, (first, after)
            if c.note != GATE:
                assert other_keys == after[3] + 1, "the gathered route's graph does not depend on the keys"
        else:
            assert hip.graph_launches() == first
        hip.bdd_circuit_free(h)                      # freeing the circuit before the module is safe
        hip.set_graphs(False)
        before = hip.graph_launches()
        h2 = hip.bdd_circuit_new(HAND)
        bits = [[ptrs[k] for k in row] for row in c.table(HAND, batch, 1)]
        hip.bdd_circuit_execute_batched(h2, d_out.ptr, n_out, bits, p, d_tmp.ptr, d_tmp.nbytes, batch)
        hip.sync()
        assert np.array_equal(d_out.download(np.int64, want0.size).reshape(shape), want1) and hip.graph_launches() == before
        hip.bdd_circuit_free(h2)
        hip.set_graphs(True)
    hip.close()


# ---- rounding margin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", GATHERED)
def test_rounding_margin_on_uniform_inputs(cases, route):
    """Uniform GGSWs, normalized state: the module's rounding-margin probe stays below the suite's limit for uniform inputs; outputs unchanged."""
    c = cases(route)
    n_out = HAND.output_size + 1
    got, notes, margin = c.device(HAND, 3, n_out, probe=True)
    assert np.array_equal(got, c.want("hand", HAND, 3, n_out)) and c.note in notes, (route, notes)
    print(f"[margin] bdd {route}: {margin:.3g}")
    assert margin < MARGIN_MAX, (route, margin)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cases):
    from poulpy_amd import abi
    c = cases("n1024-r1-one")
    hip = c.hip
    batch, n_out = 2, HAND.output_size + 1
    ct = SIZE * c.cols * c.n * 8
    with on_device(hip) as dev:
        ptrs = [dev.key(ph).ptr.value for _, ph in c.keys]
        h = hip.bdd_circuit_new(HAND)
        p = c.params()
        need = hip.bdd_circuit_execute_tmp_bytes(h, p, batch)
        assert 0 < hip.bdd_circuit_execute_tmp_bytes(h, p, 1) < need < hip.bdd_circuit_execute_tmp_bytes(h, p, 3) < hip.bdd_circuit_execute_tmp_bytes(h, p, 64)
        # one buffer: tmp first, out behind it (so that an out inside tmp can be named)
        d = dev.alloc(need + n_out * batch * ct)
        tmp, out = d.ptr.value, d.ptr.value + need
        hip.sync()

        def call(out=out, n_out=n_out, nbits=4, p=p, tmp=tmp, tmp_bytes=need, hole=None):
            flat = [ptrs[k] for row in c.table(HAND, batch) for k in row][:batch * nbits]
            if hole is not None:
                flat[hole] = None
            arr = (C.c_void_p * len(flat))(*flat)
            st = hip.lib.pz_bdd_circuit_execute_batched(hip.handle, h, out, n_out, arr, nbits, C.byref(p), tmp, tmp_bytes, batch)
            return st, hip.lib.pz_last_error().decode()
        for label, kw, code, msg in (
                ("a short tmp", dict(tmp_bytes=need - 1), abi.PZ_ERR_INVALID, "tmp too small"),
                ("nbits < input_size", dict(nbits=3), abi.PZ_ERR_INVALID, "nbits 3 < input_size 4"),
                ("a selected null bit", dict(hole=4 + 1), abi.PZ_ERR_INVALID, "input bit 1 of input 1 is null"),
                ("mixed base2k", dict(p=c.params(key_base2k=13)), abi.PZ_ERR_INVALID, "one base2k"),
                ("a_size != res_size", dict(p=c.params(a_size=2)), abi.PZ_ERR_INVALID, "a_size == p->res_size"),
                ("n_out < output_size", dict(n_out=3), abi.PZ_ERR_INVALID, "n_out 3 < output_size 4"),
                ("out overlapping tmp", dict(out=tmp + need - ct), abi.PZ_ERR_ALIAS, "out overlaps tmp"),
                ("out overlapping a key", dict(out=ptrs[0]), abi.PZ_ERR_ALIAS, "out overlaps the GGSW")):
            st, text = call(**kw)
            assert st == code and msg in text, (label, st, text)
        hip.sync()
        assert np.all(d.download(np.uint8, d.nbytes) == 0x5A), "a refused call wrote to out or tmp"
        st, text = call()
        assert st == 0, text
        hip.sync()
        got = d.download(np.int64, n_out * batch * ct // 8, offset_bytes=need).reshape(n_out, batch, SIZE, c.cols, c.n)
        assert np.array_equal(got, c.want("hand", HAND, batch, n_out))
        assert hip_clean(hip)
        hip.bdd_circuit_free(h)


def test_nothing_to_do(cases):
    """batch == 0: PZ_OK, nothing written.  A circuit of zero outputs only: out is zeroed, no GGSW is needed."""
    c = cases("n1024-r1-one")
    hip = c.hip
    ct = SIZE * c.cols * c.n * 8
    with on_device(hip) as dev:
        h = hip.bdd_circuit_new(HAND)
        d_out = dev.alloc(5 * 2 * ct)
        hip.bdd_circuit_execute_batched(h, d_out.ptr, 5, [], c.params(), None, 0, 0)
        hip.sync()
        assert np.all(d_out.download(np.uint8, d_out.nbytes) == 0x5A)
        hip.bdd_circuit_free(h)
        z = hip.bdd_circuit_new(bdd.Circuit(3, [([], 0), ([], 0)]))
        hip.bdd_circuit_execute_batched(z, d_out.ptr, 5, [[None] * 3, [None] * 3], c.params(), None, 0, 2)
        hip.sync()
        assert not d_out.download(np.uint8, d_out.nbytes).any()
        hip.bdd_circuit_free(z)


# ---- under real keys ----------------------------------------------------------------------------------------------------------------------------
def test_encrypted_addition_decrypts_on_the_device(mods):
    """N = 1024, rank 1: GGSW encryptions of the bits of (a, b), another pair per input of the batch, through poulpy_amd.bdd.execute_bdd_circuit -
    the outputs of the 3-bit adder (with carry) decrypt, at k = 2, to the bits of a + b."""
    n, rank, base2k, dnum, w, batch = 1024, 1, 12, 3, 3, 2
    ref, hip = mods(n)
    rng = seeded(32000)
    sk = fhe_sk.ternary_secret(n, rank, rng)
    circuit = bdd.adder(w, carry_out=True)
    from poulpy_amd.hal import GlweOpParams
    p = GlweOpParams(rank=rank, dnum=dnum, dsize=1, key_size=SIZE, key_base2k=base2k, a_size=SIZE, a_base2k=base2k, res_size=SIZE, res_base2k=base2k,
                     rank_out=rank)
    ggsw = {}
    for v in (0, 1):
        msg = np.zeros(n, dtype=np.int64)
        msg[0] = v
        mat = MatZnx(n, dnum, rank + 1, rank + 1, SIZE, np.ascontiguousarray(fhe_sk.ggsw_encrypt(sk, msg, base2k, SIZE * base2k, dnum, 1, rng)))
        ggsw[v] = prepared_key(ref, hip, mat)[1]
    n_out = circuit.output_size
    with on_device(hip) as dev:
        d_bit = {v: dev.key(ggsw[v]).ptr for v in (0, 1)}
        d_out = dev.alloc(n_out * batch * SIZE * (rank + 1) * n * 8)
        for pairs in (((5, 6), (7, 1)), ((0, 0), (7, 7))):
            bits = [[d_bit[v] for v in bdd.word_bits(a, b, w)] for a, b in pairs]
            bdd.execute_bdd_circuit(hip, circuit, (d_out.ptr, n_out), bits, p, batch)
            got = d_out.download(np.int64, d_out.nbytes // 8).reshape(n_out, batch, SIZE, rank + 1, n)
            for v, (a, b) in enumerate(pairs):
                dec = [int(co.decode_i64(fhe_sk.glwe_phase(got[o, v], sk), base2k, 2)[0]) & 3 for o in range(n_out)]
                assert all(d in (0, 1) for d in dec) and sum(d << o for o, d in enumerate(dec)) == a + b, (a, b, dec)
