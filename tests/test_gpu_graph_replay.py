"""HIP-graph replay of the composite calls against the oracle, on every route.

pz_blind_rotation_execute_batched, pz_glwe_trace_batched and pz_circuit_bootstrapping_execute_to_constant_batched run through
with_graph (poulpy_amd/csrc/api_glwe.hpp): the first call with an argument set runs plainly, the next one is captured, every later one is
one hipGraphLaunch.  The key is the argument values (addresses, shapes, workspaces, knobs), never the buffer contents - so here every
call gets NEW contents in the SAME buffers (new inputs every call, a new lookup table on call 4, new key contents in the same key buffer
on call 5) and every output of every call is compared bit-exactly with the oracle.  Each case owns a fresh Module, so the graph cache and
the launch counter are its own.  Then: what must invalidate a captured graph (knobs, pins, the margin probe, workspace growth, a freed
and re-allocated buffer, sibling modules), and least-recently-used eviction while evicted graphs may still be running.

Under POULPY_DBG_GRAPHS=0 (graphs off) or POULPY_DBG_CANARY=1 (guarded workspaces: every call plain) the counter must not move instead.
"""
import os

import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import unnormalized as un
from tests.device import prepared_key
from tests.helpers import MARGIN_MAX, seeded

pytestmark = pytest.mark.gpu

GRAPHS = os.environ.get("POULPY_DBG_GRAPHS") != "0" and os.environ.get("POULPY_DBG_CANARY") != "1"

_refs = {}


def _ref(n):
    from oracle.ref import RefModule
    if n not in _refs:
        _refs[n] = RefModule(n)
    return _refs[n]


def _fresh(n):
    """A module of this test's own: its graph cache, launch counter and dispatch notes start empty."""
    from poulpy_amd.hal import Module
    hip = Module(n)
    hip.set_graphs(True)
    return hip


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _call(mod, case, graph, label):
    """New input contents, one call on `mod`, every output against the oracle.  graph: True = served by a HIP graph (one more launch),
    False = run plainly (no launch), None = not asserted."""
    case.new_input()
    before = mod.graph_launches()
    case.run(mod)
    mod.sync()
    if graph is not None:
        want = 1 if graph and GRAPHS else 0
        assert mod.graph_launches() - before == want, (label, "graph launches", mod.graph_launches() - before, "expected", want)
    case.check(label)


def _protocol(hip, case, notes_in=(), notes_out=(), calls=5):
    """Calls 1..calls with new contents each (case.vary: what else changes before a call); the route's dispatch notes from calls 1-3;
    calls 4.. served by a graph, which records no notes."""
    hip.dispatch_notes(reset=True)
    for call in range(1, calls + 1):
        case.vary(call)
        # (calls 1-2 are not asserted: the first call of a module sizes its workspaces and tables, which are part of the key)
        _call(hip, case, True if call >= 4 else None, (case.label, "call", call))
        if call == 3:
            notes = hip.dispatch_notes(reset=True)
            for s in notes_in:
                assert s in notes, (case.label, s, notes)
            for s in notes_out:
                assert s not in notes, (case.label, s, notes)
    if GRAPHS:
        assert hip.dispatch_notes() == "", (case.label, "a replayed call recorded notes", hip.dispatch_notes())


def _live(hip, case, label):
    """A live graph for the case's argument set: three calls, and a fourth that must be a replay."""
    for i in range(3):
        _call(hip, case, None, (label, "warm-up", i))
    _call(hip, case, True, (label, "live"))


def _after_change(mod, case, label, note=None):
    """The call after a change runs plainly (no graph launch; `note` among its dispatch notes), the two after it are served by a graph."""
    mod.dispatch_notes(reset=True)
    _call(mod, case, False, (label, "first call after the change"))
    if note is not None:
        assert note in mod.dispatch_notes(), (label, note, mod.dispatch_notes())
    _call(mod, case, True, (label, "capture"))
    _call(mod, case, True, (label, "replay"))


def _prepared(hip, ref, n, rows, cols_in, cols_out, size, base2k, rng):
    pr, ph = prepared_key(ref, hip, MatZnx(n, rows, cols_in, cols_out, size).fill_uniform(base2k, rng))
    hip.sync()
    return pr, ph


def _brk(hip, ref, n, n_lwe, dnum, cols, size, base2k, rng):
    """blind-rotation key: the oracle's and the device's prepared GGSWs, (n_lwe, doubles) each"""
    brk_r = np.empty((n_lwe, n * dnum * cols * cols * size), dtype=np.float64)
    brk_h = np.empty_like(brk_r)
    for i in range(n_lwe):
        pr, ph = _prepared(hip, ref, n, dnum, cols, cols, size, base2k, rng)
        brk_r[i], brk_h[i] = pr.data.reshape(-1), ph.data.reshape(-1)
    return brk_r, brk_h


class _Rotation:
    """One blind-rotation argument set: device buffers allocated once, contents replaced between calls.  A pool of distinct LWE ciphertexts
    replicated over the batch (tests/test_gpu_scale.py _br_pool_parity): the oracle computes the pool, every output is checked against its
    pool entry.  Both key contents and both lookup tables are prepared up front: between calls only their bytes are written."""

    def __init__(self, hip, shape, batch, seed, pool=7, label="blind rotation"):
        from poulpy_amd.hal import BlindRotationParams
        self.n, self.rank, self.n_lwe, self.blk, self.dnum, self.bsz, self.rsz, self.k = shape
        n, cols = self.n, self.rank + 1
        self.hip, self.ref, self.batch, self.pool, self.label = hip, _ref(n), batch, min(batch, pool), label
        self.rng = seeded(seed)
        self.keys = [_brk(hip, self.ref, n, self.n_lwe, self.dnum, cols, self.bsz, self.k, self.rng) for _ in range(2)]
        self.luts = [VecZnx(n, 1, self.rsz).fill_uniform(self.k, self.rng) for _ in range(2)]
        self.xpa = self.ref.blind_rotation_x_pow_a() if self.blk > 1 else np.zeros((1, 1))
        self.out_shape = (batch, self.rsz, cols, n)
        self.d_res = hip.device_alloc(8 * int(np.prod(self.out_shape)))
        self.d_lwe = hip.device_alloc(8 * batch * (self.n_lwe + 1))
        self.d_lut = hip.device_alloc(self.luts[0].data.nbytes)
        self.d_brk = hip.device_alloc(self.keys[0][1].nbytes)
        self.p = BlindRotationParams(rank=self.rank, n_lwe=self.n_lwe, block_size=self.blk, dnum=self.dnum, brk_size=self.bsz, base2k=self.k,
                                     res_size=self.rsz, lut_size=self.rsz)
        self.use_keys(0)
        self.use_lut(0)

    def use_keys(self, i):
        self.key = i
        self.d_brk.upload(self.keys[i][1])

    def use_lut(self, i):
        self.lut = i
        self.d_lut.upload(self.luts[i].data)

    def vary(self, call):
        if call == 4:
            self.use_lut(1)
        if call == 5:
            self.use_keys(1)

    def new_input(self):
        n = self.n
        lwe = self.rng.integers(-n, n, (self.pool, self.n_lwe + 1), dtype=np.int64)   # mod_switch_2n output range
        lwe[0, 1] = 0
        lwe[-1, 0] = n - 1
        self.d_lwe.upload(lwe[np.arange(self.batch) % self.pool])
        self.want = np.empty((self.pool,) + self.out_shape[1:], dtype=np.int64)
        for b in range(self.pool):
            r = VecZnx(n, self.rank + 1, self.rsz)
            self.ref.blind_rotation_execute(r, self.k, np.ascontiguousarray(lwe[b]), self.luts[self.lut], self.keys[self.key][0], self.dnum,
                                            self.bsz, self.blk, self.xpa)
            self.want[b] = r.data

    def run(self, mod=None):
        (mod or self.hip).blind_rotation_execute_batched(self.d_res.ptr, self.d_lwe.ptr, self.d_lut.ptr, self.d_brk.ptr, self.p, self.batch)

    def check(self, label):
        got = self.d_res.download(np.int64, int(np.prod(self.out_shape))).reshape(self.out_shape)
        bad = np.flatnonzero((got != self.want[np.arange(self.batch) % self.pool]).reshape(self.batch, -1).any(axis=1))
        assert bad.size == 0, (label, "mismatching ciphertexts", bad.size, "of", self.batch, "first", bad[:8].tolist())

    def free(self):
        for d in (self.d_res, self.d_lwe, self.d_lut, self.d_brk):
            d.free()


class _Trace:
    """One glwe_trace argument set (in place on the batch): one prepared key per step, every key pinned but step 0's; call 5 writes new
    contents into that unpinned key.  fills[i]: the input of call i + 1 (tests/unnormalized.py fills; None = normalized digits)."""

    def __init__(self, hip, n, k, seed, rank=1, size=None, nsteps=None, batch=None, pin=True, fills=None, label="trace"):
        from poulpy_amd.hal import GlweOpParams
        dsize, dstep = (3, 3) if n < 65536 else (4, 2)
        self.n, self.k, self.rank = n, k, rank
        self.size = size or dsize
        nsteps = nsteps or dstep
        self.batch = batch or (3 if n < 65536 else 2)
        self.hip, self.ref, self.label, self.fills, self.calls = hip, _ref(n), label, fills or [], 0
        self.rng = seeded(seed)
        cols, dnum = rank + 1, self.size
        self.gals = [-1] + [pow(5, 1 << i, 2 * n) for i in range(nsteps - 1)]
        self.key_shape = (dnum, rank, cols, self.size)
        self.keys = [_prepared(hip, self.ref, n, *self.key_shape, k, self.rng) for _ in self.gals]
        self.key0_next = _prepared(hip, self.ref, n, *self.key_shape, k, self.rng)   # the contents call 5 writes into step 0's key
        self.d_keys = [hip.device_alloc(ph.data.nbytes).upload(ph.data) for _, ph in self.keys]
        self.pinned = set()
        if pin:
            for s in range(1, len(self.gals)):
                self.pin(s)
        self.out_shape = (self.batch, self.size, cols, n)
        self.d_res = hip.device_alloc(8 * int(np.prod(self.out_shape)))
        self.p = GlweOpParams(rank=rank, dnum=dnum, dsize=1, key_size=self.size, key_base2k=k, a_size=self.size, a_base2k=k,
                              res_size=self.size, res_base2k=k, rank_out=rank)

    def pin(self, s):
        self.hip.pin_key(self.d_keys[s].ptr, *self.key_shape)
        self.pinned.add(s)

    def unpin(self, s):
        self.hip.unpin_key(self.d_keys[s].ptr)
        self.pinned.discard(s)

    def set_key(self, s, prepared):
        assert s not in self.pinned    # a pinned key's contents are promised not to change
        self.keys[s] = prepared
        self.d_keys[s].upload(prepared[1].data)

    def vary(self, call):
        if call == 5:
            self.set_key(0, self.key0_next)

    def new_input(self):
        fill = self.fills[self.calls] if self.calls < len(self.fills) else None
        self.calls += 1
        cols = self.rank + 1
        cts = np.empty(self.out_shape, dtype=np.int64)
        self.want = np.empty_like(cts)
        for b in range(self.batch):
            ct = VecZnx(self.n, cols, self.size).fill_uniform(self.k, self.rng)
            if fill is not None:
                fill(b, ct.data, self.rng)
            cts[b] = ct.data
            self.ref.glwe_trace_assign(ct, self.k, self.gals, [pr for pr, _ in self.keys])
            self.want[b] = ct.data
        self.d_res.upload(cts)

    def run(self, mod=None):
        (mod or self.hip).glwe_trace_batched(self.d_res.ptr, self.gals, [d.ptr for d in self.d_keys], self.p, self.batch)

    def check(self, label):
        got = self.d_res.download(np.int64, int(np.prod(self.out_shape))).reshape(self.out_shape)
        bad = np.flatnonzero((got != self.want).reshape(self.batch, -1).any(axis=1))
        assert bad.size == 0, (label, "mismatching ciphertexts", bad.tolist())

    def free(self):
        for s in list(self.pinned):
            self.unpin(s)
        for d in self.d_keys + [self.d_res]:
            d.free()


class _CircuitBootstrap:
    """circuit bootstrapping to a constant (tests/test_gpu_parity.py test_circuit_bootstrapping_to_constant's set-up): new LWEs every call,
    a new lookup table on call 4, new blind-rotation key contents in the same buffer on call 5; tmp allocated once."""

    def __init__(self, hip, n, rank, n_lwe, blk, brk_dnum, glwe_size, res_dnum, res_size, batch, seed):
        from poulpy_amd.hal import BlindRotationParams, CircuitBootstrappingParams
        base2k, atk_dnum, tsk_dnum = 13, 3, 2
        self.n, self.rank, self.n_lwe, self.blk, self.batch, self.base2k = n, rank, n_lwe, blk, batch, base2k
        self.brk_dnum, self.glwe_size = brk_dnum, glwe_size
        self.hip, self.ref, self.label = hip, _ref(n), ("circuit bootstrapping", n, rank, blk)
        self.rng = rng = seeded(seed)
        cols = rank + 1
        log_n = n.bit_length() - 1
        self.gap = 2 * int(rng.integers(1, n // 8))
        self.keys = [_brk(hip, self.ref, n, n_lwe, brk_dnum, cols, glwe_size, base2k, rng) for _ in range(2)]
        self.luts = [VecZnx(n, 1, glwe_size).fill_uniform(base2k, rng) for _ in range(2)]
        tmp_size = max(glwe_size, res_size)
        self.gals = [-1] + [pow(5, 1 << i, 2 * n) for i in range(log_n - 1)]
        self.atk = [_prepared(hip, self.ref, n, atk_dnum, rank, cols, tmp_size, base2k, rng) for _ in self.gals]
        self.tsk = [_prepared(hip, self.ref, n, tsk_dnum, rank, cols, res_size + 1, base2k, rng) for _ in range(rank)]
        self.xpa = self.ref.blind_rotation_x_pow_a() if blk > 1 else np.zeros((1, 1))
        self.out_shape = (batch, res_dnum, cols, res_size, cols, n)
        self.res_dnum, self.res_size = res_dnum, res_size
        self.d_res = hip.device_alloc(8 * int(np.prod(self.out_shape)))
        self.d_lwe = hip.device_alloc(8 * batch * (n_lwe + 1))
        self.d_lut = hip.device_alloc(self.luts[0].data.nbytes)
        self.d_brk = hip.device_alloc(self.keys[0][1].nbytes)
        self.d_atk = [hip.device_alloc(ph.data.nbytes).upload(ph.data) for _, ph in self.atk]
        self.d_tsk = [hip.device_alloc(ph.data.nbytes).upload(ph.data) for _, ph in self.tsk]
        self.p = CircuitBootstrappingParams(
            br=BlindRotationParams(rank=rank, n_lwe=n_lwe, block_size=blk, dnum=brk_dnum, brk_size=glwe_size, base2k=base2k, res_size=glwe_size,
                                   lut_size=glwe_size),
            atk_dnum=atk_dnum, atk_size=tmp_size, tsk_dnum=tsk_dnum, tsk_size=res_size + 1, res_dnum=res_dnum, res_size=res_size, gap=self.gap)
        self.tmp_bytes = hip.circuit_bootstrapping_tmp_bytes(self.p, batch)
        self.d_tmp = hip.device_alloc(self.tmp_bytes)
        self.key, self.lut = 0, 0
        self.d_brk.upload(self.keys[0][1])
        self.d_lut.upload(self.luts[0].data)

    def vary(self, call):
        if call == 4:
            self.lut = 1
            self.d_lut.upload(self.luts[1].data)
        if call == 5:
            self.key = 1
            self.d_brk.upload(self.keys[1][1])

    def new_input(self):
        n, cols = self.n, self.rank + 1
        lwe = self.rng.integers(-n, n, (self.batch, self.n_lwe + 1), dtype=np.int64)
        self.d_lwe.upload(lwe)
        self.want = np.empty(self.out_shape, dtype=np.int64)
        for b in range(self.batch):
            g = MatZnx(n, self.res_dnum, cols, cols, self.res_size)
            self.ref.circuit_bootstrap_to_constant(g, self.base2k, np.ascontiguousarray(lwe[b]), self.luts[self.lut], self.keys[self.key][0],
                                                   self.brk_dnum, self.glwe_size, self.glwe_size, self.blk, self.xpa, self.gals,
                                                   [a[0] for a in self.atk], [t[0] for t in self.tsk], self.gap)
            self.want[b] = g.data

    def run(self, mod=None):
        (mod or self.hip).circuit_bootstrapping_execute_to_constant_batched(
            self.d_res.ptr, self.d_lwe.ptr, self.d_lut.ptr, self.d_brk.ptr, self.gals, [d.ptr for d in self.d_atk], [d.ptr for d in self.d_tsk],
            self.p, self.d_tmp.ptr, self.tmp_bytes, self.batch)

    def check(self, label):
        got = self.d_res.download(np.int64, int(np.prod(self.out_shape))).reshape(self.out_shape)
        bad = np.flatnonzero((got != self.want).reshape(self.batch, -1).any(axis=1))
        assert bad.size == 0, (label, "mismatching ciphertexts", bad.tolist())

    def free(self):
        for d in [self.d_res, self.d_lwe, self.d_lut, self.d_brk, self.d_tmp] + self.d_atk + self.d_tsk:
            d.free()


# ---- every route, five calls -----------------------------------------------------------------------------------------------------------

SMALL_RING = (2048, 1, 6, 3, 2, 2, 2, 13)
BR_ROUTES = [
    # id, (n, rank, n_lwe, blk, dnum, bsz, rsz, base2k), batch = a * ncu + b, fusion, notes present, notes absent
    ("fused-CT1", (512, 3, 7, 3, 1, 2, 1, 18), (0, 5), (True, True), ("k_br_fused<", "CT=1,NT=512"), ()),
    ("fused-CT2-A32", (512, 3, 7, 3, 1, 2, 3, 18), (1, 45), (True, True), ("k_br_fused<", "CT=2,NT=512", "A32=1"), ()),
    ("fused-NT256", (512, 3, 7, 3, 1, 2, 1, 18), (2, 91), (True, True), ("k_br_fused<", "CT=1,NT=256"), ()),
    ("fused-STD", (512, 1, 7, 1, 2, 3, 2, 19), (0, 3), (True, True), ("k_br_fused<", "STD=1"), ()),
    ("standard", (512, 1, 7, 1, 2, 3, 2, 19), (0, 3), (True, False), (), ("k_br_fused",)),
    ("small-ring", SMALL_RING, (0, 3), (True, True), ("k_br_block_lds<",), ("k_br_fused", "k_mid128")),
    ("small-ring-two-streams", SMALL_RING, (0, 512), (True, True), ("k_br_block_lds<",), ("k_br_fused", "k_mid128")),
    ("pipeline-4096", (4096, 1, 6, 3, 2, 2, 2, 13), (0, 3), (True, True), ("k_mid128<", "BR=1"), ("k_br_fused",)),
    ("pipeline-16384", (16384, 1, 14, 7, 3, 3, 3, 13), (0, 2), (True, True), ("k_mid128<", "BR=1"), ("k_br_fused",)),
    ("composed", SMALL_RING, (0, 3), (False, False), (), ("k_br_fused", "k_br_block", "k_mid128")),
]


@pytest.mark.parametrize("route,shape,batch,fuse,notes_in,notes_out", BR_ROUTES, ids=[r[0] for r in BR_ROUTES])
def test_blind_rotation_replays_on_every_route(route, shape, batch, fuse, notes_in, notes_out):
    """The standard and composed routes record no note: they are told apart by the notes they must not have."""
    batch = batch[0] * (_ncu() if batch[0] else 0) + batch[1]
    hip = _fresh(shape[0])
    hip.set_fusion(*fuse)
    case = _Rotation(hip, shape, batch, seed=7100 + shape[0] + batch + shape[3], label=(route, batch))
    _protocol(hip, case, notes_in, notes_out)
    case.free()
    hip.close()


# (the small-ring kernels record no note; the pipeline at 8192 and the spectral form at 65536 record the same middle kernel)
TRACE_NOTES = {1024: ((), ("k_mid128",)), 8192: (("k_mid128<", "PERM=1", "BR=0"), ()), 65536: (("k_mid128<", "PERM=1", "BR=0"), ())}


@pytest.mark.parametrize("k", [12, 14])
@pytest.mark.parametrize("n", [1024, 8192, 65536])
def test_glwe_trace_replays_on_every_route(n, k):
    """N = 1024: the small-ring kernels with the automorphism / shifted store (k_small_inv<.., AU>); 8192: the fused pipeline;
    65536: the spectral automorphism form (shifted store in the tail, 16-bit body operand at base2k <= 14).  Step 0's key unpinned."""
    hip = _fresh(n)
    case = _Trace(hip, n, k, seed=7200 + n + k, label=("trace", n, k))
    _protocol(hip, case, *TRACE_NOTES[n])
    case.free()
    hip.close()


@pytest.mark.parametrize("k", [12, 14])
@pytest.mark.parametrize("n", [8192, 65536])
def test_glwe_trace_replays_with_wide_digits(n, k):
    """The 16-bit body operand's wide-digit flag is decided on the device: captured with normalized input, replayed with digits of 2^15 and
    more (a graph that baked the decision in would take the 16-bit copies), then normalized again."""
    hip = _fresh(n)
    wide = un.sums(k, 17 - k)
    case = _Trace(hip, n, k, seed=7300 + n + k, fills=[None, None, None, wide, None, wide], label=("trace, wide digits", n, k))
    _protocol(hip, case, calls=6)
    case.free()
    hip.close()


@pytest.mark.parametrize("n,rank,n_lwe,blk,brk_dnum,glwe_size,res_dnum,res_size,batch,notes_in", [
    (256, 1, 6, 3, 2, 3, 2, 2, 2, ("k_br_fused<", "CT=1,NT=512")),
    (512, 1, 4, 1, 2, 2, 3, 3, 2, ("k_br_fused<", "STD=1")),
])
def test_circuit_bootstrapping_replays(n, rank, n_lwe, blk, brk_dnum, glwe_size, res_dnum, res_size, batch, notes_in):
    """tests/test_gpu_parity.py test_circuit_bootstrapping_to_constant's shapes (the rotation inside: the one-kernel block-binary and standard forms)."""
    hip = _fresh(n)
    case = _CircuitBootstrap(hip, n, rank, n_lwe, blk, brk_dnum, glwe_size, res_dnum, res_size, batch, seed=7400 + n)
    _protocol(hip, case, notes_in)
    case.free()
    hip.close()


# ---- what must invalidate a captured graph ---------------------------------------------------------------------------------------------

def test_fusion_change_invalidates():
    hip = _fresh(2048)
    case = _Rotation(hip, SMALL_RING, 3, seed=7500)
    _live(hip, case, "fusion")
    hip.set_fusion(False, False)
    _call(hip, case, False, ("fusion off", "composed route"))
    hip.set_fusion(True, True)
    _after_change(hip, case, "fusion back on", note="k_br_block_lds<")
    case.free()
    hip.close()


def test_small_path_change_invalidates():
    hip = _fresh(4096)
    case = _Trace(hip, 4096, 12, seed=7510)
    _live(hip, case, "small path")
    hip.set_small_path(False)
    _after_change(hip, case, "small path off", note="k_mid128")
    hip.set_small_path(True)
    _after_change(hip, case, "small path on")
    case.free()
    hip.close()


def test_chunk_change_invalidates():
    hip = _fresh(8192)
    case = _Trace(hip, 8192, 12, seed=7520)
    _live(hip, case, "chunk")
    hip.set_chunk(2)
    _after_change(hip, case, "chunk 2", note="k_mid128")
    hip.set_chunk(0)
    _after_change(hip, case, "chunk 0", note="k_mid128")
    case.free()
    hip.close()


def test_pin_changes_invalidate():
    """pin_key of the trace's unpinned key; then unpin it, write new contents into it and pin it again."""
    hip = _fresh(8192)
    case = _Trace(hip, 8192, 14, seed=7530)
    _live(hip, case, "pin")
    case.pin(0)
    _after_change(hip, case, "pinned", note="k_mid128")
    case.unpin(0)
    case.set_key(0, _prepared(hip, case.ref, 8192, *case.key_shape, case.k, case.rng))
    case.pin(0)
    _after_change(hip, case, "unpinned, rewritten, pinned again", note="k_mid128")
    case.free()
    hip.close()


def test_margin_probe_between_replays():
    """The probe is part of the key: the probed call runs plainly (the probing kernels), the calls after it replay the graph it left alone."""
    hip = _fresh(2048)
    case = _Rotation(hip, SMALL_RING, 3, seed=7540)
    _live(hip, case, "probe")
    case.new_input()
    before = hip.graph_launches()
    margin = hip.rounding_margin_of(lambda: case.run())
    assert hip.graph_launches() == before, "the probed call was served by a graph"
    assert margin < MARGIN_MAX, margin
    case.check("probed call")
    _call(hip, case, True, ("probe off", 1))
    _call(hip, case, True, ("probe off", 2))
    case.free()
    hip.close()


def test_workspace_growth_invalidates():
    """A call at 8x the batch on other buffers grows the workspaces between replays: the next call of the first set runs plainly."""
    hip = _fresh(2048)
    case = _Rotation(hip, SMALL_RING, 3, seed=7550)
    _live(hip, case, "workspace")
    big = _Rotation(hip, SMALL_RING, 24, seed=7551, label="8x batch")
    _call(hip, big, False, "8x batch, first sight")
    _after_change(hip, case, "after workspace growth", note="k_br_block_lds<")
    big.free()
    case.free()
    hip.close()


def test_reallocated_input_buffer():
    """An input buffer freed and allocated again at the same size between replays: a new address runs plainly, the same address may replay
    (the graph's pointers are valid again) - either way the output follows the new contents."""
    hip = _fresh(2048)
    case = _Rotation(hip, SMALL_RING, 3, seed=7560)
    _live(hip, case, "realloc")
    old = case.d_lwe.ptr.value
    nbytes = case.d_lwe.nbytes
    case.d_lwe.free()
    case.d_lwe = hip.device_alloc(nbytes)
    same = case.d_lwe.ptr.value == old
    _call(hip, case, same, ("re-allocated input", "same address" if same else "new address"))
    _call(hip, case, True, ("re-allocated input", 2))
    _call(hip, case, True, ("re-allocated input", 3))
    case.free()
    hip.close()


def test_sibling_modules_alternate_on_the_same_buffers():
    """Two clones, each with its own stream and graph cache, take turns with the same call on the same buffers."""
    base = _fresh(2048)
    sibs = [base.clone(), base.clone()]
    for s in sibs:
        s.set_graphs(True)
    case = _Rotation(base, SMALL_RING, 3, seed=7570)
    for rnd in range(5):
        for i, s in enumerate(sibs):
            _call(s, case, True if rnd >= 3 else None, ("sibling", i, "round", rnd))
    case.free()
    for s in sibs:
        s.close()
    base.close()


# ---- eviction --------------------------------------------------------------------------------------------------------------------------

def test_eviction_of_graphs_in_flight():
    """16 live argument sets (the cache's size), replayed back to back, then at once - no host sync - the first calls of 4 new sets, which
    evict the least-recently-used graphs while they may still be running.  Every output, then 4 of the evicted sets once more."""
    hip = _fresh(2048)
    sets = [_Rotation(hip, SMALL_RING, 3, seed=7600 + i, label=("set", i)) for i in range(20)]
    # (shared keys and table: each set its own LWE and result buffers)
    for s in sets[1:]:
        s.d_brk.free()
        s.d_lut.free()
        s.d_brk, s.d_lut, s.keys, s.luts = sets[0].d_brk, sets[0].d_lut, sets[0].keys, sets[0].luts
    _call(hip, sets[0], None, "first call of the module")   # sizes the workspaces: a key of its own
    for s in sets[:16]:
        for i in range(3):
            _call(hip, s, None, (s.label, "call", i))
    for s in sets:
        s.new_input()        # (uploads synchronize the stream: all of them before the burst)
    before = hip.graph_launches()
    for s in sets[:16]:
        s.run()
    mid = hip.graph_launches()
    for s in sets[16:]:
        s.run()
    hip.sync()
    assert mid - before == (16 if GRAPHS else 0), "the 16 live sets were not all replayed"
    assert hip.graph_launches() == mid, "a first call was served by a graph"
    for s in sets:
        s.check((s.label, "burst"))
    for s in sets[:4]:
        _call(hip, s, False, (s.label, "evicted, called again"))
    for s in sets[1:]:
        s.d_res.free()
        s.d_lwe.free()
    sets[0].free()
    hip.close()
