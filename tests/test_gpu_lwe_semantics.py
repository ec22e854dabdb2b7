"""The LWE-side cases of tests/lwe_cases.py through the batched device entry points: pz_lwe_mod_switch_2n_batched, pz_lwe_keyswitch_batched,
pz_glwe_from_lwe_batched, pz_lwe_from_glwe_batched, pz_blind_rotation_execute_batched and its extended form.

Every case is a batch of 3 inputs with their own messages.  Per case: device == oracle bit for bit, then the decryption under the real
keys (tests/fhe_sk.py) against what the exact arithmetic says and the derived bound, then the dispatch note of the route.  The negative
controls go through the same calls: device == oracle, and the decryption misses.  The shapes are the reference's own (tests/test_lwe_semantics.py)
and one small case per route of DESIGN.md section 4.7; where a route's shape leaves no room for the reference's 16-value table at its
noise the case shrinks the message modulus and says so in its noise line (`-s`)."""
import numpy as np
import pytest

from tests import lwe_cases as lc
from tests.device import mods, on_device  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- conversions ----
def _conversion_device(hip, c):
    from poulpy_amd.hal import GlweOpParams
    rows, cols_in, ksz, cols_out, n = c.key.shape
    ph = lc.prepare(hip, c.key)
    batch = len(c.a)
    a_size = c.glwe_size if c.op == "glwe_from_lwe" else c.a.shape[1]
    a_base2k = c.key_base2k if c.op == "glwe_from_lwe" else c.a_base2k
    p = GlweOpParams(rank=c.rank, dnum=rows, dsize=c.dsize, key_size=ksz, key_base2k=c.key_base2k, a_size=a_size, a_base2k=a_base2k,
                     res_size=c.res_size, res_base2k=c.res_base2k, rank_out=c.rank_out)
    if c.op == "glwe_from_lwe":
        shape = (batch, c.res_size, c.rank_out + 1, n)
    else:
        shape = (batch, c.res_size, (c.n_out if c.op == "lwe_ks" else c.n_lwe) + 1)
    with on_device(hip) as dev:
        d_a, d_k = dev.upload(c.a), dev.key(ph)
        d_r = dev.alloc(int(np.prod(shape)) * 8)
        hip.dispatch_notes(reset=True)
        if c.op == "lwe_ks":
            hip.lwe_keyswitch_batched(d_r.ptr, c.n_out, d_a.ptr, c.n_in, d_k.ptr, p, batch)
        elif c.op == "glwe_from_lwe":
            hip.glwe_from_lwe_batched(d_r.ptr, d_a.ptr, c.n_lwe, c.a.shape[1], c.a_base2k, d_k.ptr, p, batch)
        else:
            hip.lwe_from_glwe_batched(d_r.ptr, c.n_lwe, d_a.ptr, c.a_idx, d_k.ptr, p, batch)
        hip.sync()
        got = d_r.download(np.int64, int(np.prod(shape))).reshape(shape)
        notes = hip.dispatch_notes()
    return got, notes


def _run_conversion(ref, hip, label, c, fail=False):
    got, notes = _conversion_device(hip, c)
    assert np.array_equal(got, lc.run_conversion_oracle(ref, c)), (label, "device != oracle")
    lc.check_conversion(label, c, got, fail=fail)
    return notes


def test_reference_conversions_on_device(mods):
    """The reference's three tests at N = 256 with their three bases (the five-kernel path)."""
    ref, hip = mods(lc.N)
    for label, c in lc.reference_conversions():
        notes = _run_conversion(ref, hip, label, c)
        assert "k_mid128" not in notes, (label, notes)


def test_conversion_controls_fail_on_device(mods):
    ref, hip = mods(lc.N)
    for label, c in lc.conversion_controls():
        _run_conversion(ref, hip, label, c, fail=True)


# (N, input / key / output base2k, limbs of the input, small-ring path): the shapes of tests/test_gpu_lwe.py - N = 4096 on the two-kernel path and
# on the fused pipeline, N = 8192 with three different bases
CONVERSION_SHAPES = [(4096, (13, 13, 13), 3, True), (4096, (13, 13, 13), 3, False), (8192, (17, 12, 15), 2, True)]


@pytest.mark.parametrize("n,bases,limbs,small_path", CONVERSION_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_conversions_on_the_pipeline(mods, n, bases, limbs, small_path):
    ref, hip = mods(n)
    pipeline = n >= 8192 or not small_path
    with on_device(hip, small_path=small_path):
        for label, c in lc.shape_conversions(n, bases, limbs):
            notes = _run_conversion(ref, hip, (n, label), c)
            assert ("k_mid128" in notes) == pipeline, (n, label, notes)


# ---- blind rotation ----
def _rotation_device(hip, ref, c, fuse=(True, True)):
    """mod_switch_2n, the rotation and (c.ksk) the key switch back, every step on the device: (lwe_2n, acc, lwe_out or None, notes)."""
    from poulpy_amd.hal import BlindRotationParams, GlweOpParams
    batch, cols = len(c.lwe), c.rank + 1
    brk = lc.brk_prepared(hip, c)
    p = BlindRotationParams(rank=c.rank, n_lwe=c.n_lwe, block_size=c.block_size, dnum=c.dnum, brk_size=c.brk_size, base2k=c.base2k,
                            res_size=c.res_size, lut_size=c.lut.shape[1])
    out = None
    with on_device(hip, fuse=fuse) as dev:
        d_lwe, d_lut, d_brk = dev.upload(c.lwe), dev.upload(c.lut), dev.upload(brk)
        d_2n = dev.alloc(batch * (c.n_lwe + 1) * 8)
        d_acc = dev.alloc(batch * c.res_size * cols * c.n * 8)
        hip.lwe_mod_switch_2n_batched(d_2n.ptr, d_lwe.ptr, c.n_lwe, c.lwe.shape[1], c.lwe_base2k, c.n2, c.negate, batch)
        hip.dispatch_notes(reset=True)
        if c.ext > 1:
            nbytes = hip.blind_rotation_extended_tmp_bytes(p, c.ext, batch)
            d_tmp = dev.alloc(nbytes, poison=False)
            hip.blind_rotation_execute_extended_batched(d_acc.ptr, d_2n.ptr, d_lut.ptr, d_brk.ptr, p, c.ext, d_tmp.ptr, nbytes, batch)
        else:
            hip.blind_rotation_execute_batched(d_acc.ptr, d_2n.ptr, d_lut.ptr, d_brk.ptr, p, batch)
        hip.sync()
        notes = hip.dispatch_notes()
        if hasattr(c, "ksk"):
            ksk = lc.prepare(hip, c.ksk)
            d_ksk = dev.key(ksk)
            d_out = dev.alloc(batch * c.res_size * (c.n_lwe + 1) * 8)
            kp = GlweOpParams(rank=c.rank, dnum=ksk.rows, dsize=1, key_size=ksk.size, key_base2k=c.base2k, a_size=c.res_size, a_base2k=c.base2k,
                              res_size=c.res_size, res_base2k=c.base2k, rank_out=1)
            hip.lwe_from_glwe_batched(d_out.ptr, c.n_lwe, d_acc.ptr, 0, d_ksk.ptr, kp, batch)
            hip.sync()
            out = d_out.download(np.int64, batch * c.res_size * (c.n_lwe + 1)).reshape(batch, c.res_size, c.n_lwe + 1)
        lwe_2n = d_2n.download(np.int64, batch * (c.n_lwe + 1)).reshape(batch, c.n_lwe + 1)
        acc = d_acc.download(np.int64, batch * c.res_size * cols * c.n).reshape(batch, c.res_size, cols, c.n)
    return lwe_2n, acc, out, notes


def _run_rotation(ref, hip, label, c, fail=False, fuse=(True, True)):
    lwe_2n, acc, out, notes = _rotation_device(hip, ref, c, fuse=fuse)
    want_2n, want_acc = lc.run_rotation_oracle(ref, c)
    assert np.array_equal(lwe_2n, want_2n), (label, "mod_switch_2n: device != oracle")
    assert np.array_equal(acc, want_acc), (label, "rotation: device != oracle")
    lc.check_rotation(label, c, lwe_2n, acc, fail=fail)
    if out is not None:
        assert np.array_equal(out, lc.run_gate_oracle(ref, c, want_acc)), (label, "lwe_from_glwe: device != oracle")
        lc.check_gate((label, "LWE"), c, out, fail=fail)
    print(f"[route] {label}: {notes}")
    return notes


def _assert_route(route, label, notes):
    if route == "one kernel":
        assert "k_br_fused" in notes, (label, notes)
    elif route == "small ring":
        assert "k_br_block" in notes and "k_br_fused" not in notes, (label, notes)
    elif route == "pipeline":
        assert "BR=1" in notes, (label, notes)
    else:   # composed, and the extended rotation: per-op kernels, none of the three fused forms
        assert route in ("composed", "extended") and "k_br_fused" not in notes and "k_br_block" not in notes and "BR=1" not in notes, (label, notes)


# route of DESIGN.md section 4.7, (N, rank, n_lwe, block, dnum, key limbs, result limbs, base2k), fusion switches
ROUTES = [
    ("one kernel", (512, 1, 224, 1, 2, 3, 2, 19), (True, True)),        # the reference's `standard`
    ("one kernel", (512, 1, 224, 7, 2, 3, 2, 19), (True, True)),        # the reference's `block_binary`
    ("one kernel", (1024, 1, 28, 7, 2, 2, 2, 17), (True, True)),        # BASELINE configs[3]: key limbs = result limbs, room for 8 values
    ("small ring", (1024, 2, 6, 3, 3, 3, 3, 13), (True, True)),
    ("small ring", (2048, 1, 14, 7, 3, 3, 3, 13), (True, True)),
    ("pipeline", (4096, 1, 14, 7, 3, 3, 3, 13), (True, True)),          # 16-bit accumulator digits between blocks (base2k <= 15)
    ("pipeline", (4096, 1, 6, 3, 2, 2, 2, 17), (True, True)),           # 32-bit accumulator digits
    ("composed", (256, 1, 6, 3, 2, 3, 2, 14), (False, False)),
    ("composed", (4096, 1, 6, 3, 2, 2, 2, 17), (False, False)),
]


@pytest.mark.parametrize("route,shape,fuse", ROUTES, ids=[f"{r[0]}-n{r[1][0]}-b{r[1][3]}-k{r[1][7]}-{'fused' if r[2][0] else 'unfused'}".replace(" ", "_")
                                                         for r in ROUTES])
def test_routes_decrypt(mods, route, shape, fuse):
    n, rank, n_lwe, block_size, dnum, brk_size, res_size, base2k = shape
    ref, hip = mods(n)
    c = lc.blind_rotation_case(n, rank, n_lwe, block_size, dnum, brk_size, res_size, base2k, seed=n + n_lwe + base2k)
    notes = _run_rotation(ref, hip, (route,) + shape, c, fuse=fuse)
    _assert_route(route, shape, notes)


def test_reference_extended_rotation_on_device(mods):
    """fft64_ref.rs:36-40 `block_binary_extended`: extension factor 2, the table over two polynomials."""
    ref, hip = mods(lc.REF_ROTATION["n"])
    c = lc.blind_rotation_case(block_size=7, ext=2, seed=100 + 7 + 2, **lc.REF_ROTATION)
    _assert_route("extended", 2, _run_rotation(ref, hip, ("extended", 2), c))


@pytest.mark.parametrize("label,kw,fail", lc.ROTATION_CONTROLS, ids=[c[0] for c in lc.ROTATION_CONTROLS])
def test_rotation_controls_on_device(mods, label, kw, fail):
    ref, hip = mods(lc.SMALL["n"])
    c = lc.blind_rotation_case(**{**lc.SMALL, **kw}, seed=300)
    _run_rotation(ref, hip, label, c, fail=fail)


@pytest.mark.parametrize("n,brk_size", [(1024, 3), (2048, 3)])
def test_gate_bootstrap_chain_decrypts(mods, n, brk_size):
    """LWE encrypt -> device mod_switch_2n -> rotation -> lwe_from_glwe at coefficient 0 under a real GLWE -> LWE key -> LWE decrypt = f(x)."""
    ref, hip = mods(n)
    c = lc.blind_rotation_case(n, 1, 28, 7, 2, brk_size, 2, 17, seed=400 + n, gate=True)
    _run_rotation(ref, hip, ("gate", n), c)


def test_headline_control_fails_on_device(mods):
    """At BASELINE configs[3]'s shape too: the key's rows in reversed LWE order give device == oracle and a failed decryption; its twin decrypts."""
    ref, hip = mods(1024)
    shape = dict(n=1024, rank=1, n_lwe=28, block_size=7, dnum=2, brk_size=2, res_size=2, base2k=17)
    _run_rotation(ref, hip, "configs[3]: key rows reversed", lc.blind_rotation_case(**shape, seed=77, reverse_rows=True), fail=True)
    _run_rotation(ref, hip, "configs[3]: twin", lc.blind_rotation_case(**shape, seed=77, gate=True))


# ---- circuit bootstrapping ----
def _cbt_device(hip, c):
    """mod_switch_2n and the circuit bootstrap on the device: (lwe_2n, GGSWs (batch, res_dnum, cols, res_size, cols, n))."""
    from poulpy_amd.hal import BlindRotationParams, CircuitBootstrappingParams
    batch, cols = len(c.lwe), c.rank + 1
    brk_b, atk_b, tsk_b, res_b = c.bases
    brk = lc.brk_prepared(hip, c)
    atk = [lc.prepare(hip, k) for k in c.atk]
    tsk = [lc.prepare(hip, k) for k in c.tsk]
    shape = (batch, c.res_dnum, cols, c.res_size, cols, c.n)
    p = CircuitBootstrappingParams(
        br=BlindRotationParams(rank=c.rank, n_lwe=c.n_lwe, block_size=c.block_size, dnum=c.brk_dnum, brk_size=c.sh["glwe_size"], base2k=brk_b,
                               res_size=c.sh["glwe_size"], lut_size=c.lut.shape[1]),
        atk_dnum=c.atk_dnum, atk_size=atk[0].size, tsk_dnum=c.tsk_dnum, tsk_size=tsk[0].size, res_dnum=c.res_dnum, res_size=c.res_size,
        gap=c.gap, atk_base2k=atk_b, tsk_base2k=tsk_b, res_base2k=res_b, atk_glwe_size=c.sh["atk_glwe_size"], trace_size=c.sh["trace_size"])
    with on_device(hip) as dev:
        d_lwe, d_lut, d_brk = dev.upload(c.lwe), dev.upload(c.lut), dev.upload(brk)
        d_atk, d_tsk = [dev.key(k) for k in atk], [dev.key(k) for k in tsk]
        d_2n = dev.alloc(batch * (c.n_lwe + 1) * 8)
        d_res = dev.alloc(int(np.prod(shape)) * 8)
        hip.lwe_mod_switch_2n_batched(d_2n.ptr, d_lwe.ptr, c.n_lwe, c.lwe.shape[1], c.lwe_base2k, c.n2, c.negate, batch)
        if c.to_exponent:
            nbytes = hip.circuit_bootstrapping_to_exponent_tmp_bytes(p, c.log_domain, batch)
            d_tmp = dev.alloc(nbytes, poison=False)
            hip.circuit_bootstrapping_execute_to_exponent_batched(d_res.ptr, d_2n.ptr, d_lut.ptr, d_brk.ptr, c.gals, [k.ptr for k in d_atk],
                                                                  [k.ptr for k in d_tsk], p, c.log_gap_in, c.log_gap_out, c.log_domain, d_tmp.ptr,
                                                                  nbytes, batch)
        else:
            nbytes = hip.circuit_bootstrapping_tmp_bytes(p, batch)
            d_tmp = dev.alloc(nbytes, poison=False)
            hip.circuit_bootstrapping_execute_to_constant_batched(d_res.ptr, d_2n.ptr, d_lut.ptr, d_brk.ptr, c.gals, [k.ptr for k in d_atk],
                                                                  [k.ptr for k in d_tsk], p, d_tmp.ptr, nbytes, batch)
        hip.sync()
        lwe_2n = d_2n.download(np.int64, batch * (c.n_lwe + 1)).reshape(batch, c.n_lwe + 1)
        got = d_res.download(np.int64, int(np.prod(shape))).reshape(shape)
    return lwe_2n, got


def _cbt_end_device(hip, c, ggsw, cts):
    """The end check's external products, each element by its own GGSW: pz_glwe_external_product_batched."""
    from poulpy_amd.hal import GlweOpParams
    res_b = c.bases[3]
    p = GlweOpParams(rank=c.rank, dnum=c.res_dnum, dsize=1, key_size=c.res_size, key_base2k=res_b, a_size=c.res_size, a_base2k=res_b,
                     res_size=c.res_size, res_base2k=res_b, rank_out=c.rank)
    out = np.empty_like(cts)
    with on_device(hip) as dev:
        for b in range(len(cts)):
            d_a, d_k = dev.upload(cts[b]), dev.key(lc.prepare(hip, ggsw[b]))
            d_r = dev.alloc(cts[b].nbytes)
            hip.glwe_external_product_batched(d_r.ptr, d_a.ptr, d_k.ptr, p, 1)
            hip.sync()
            out[b] = d_r.download(np.int64, cts[b].size).reshape(cts[b].shape)
    return out


def _run_cbt(ref, hip, label, c, fail=False):
    want_2n, want = lc.run_cbt_oracle(ref, c)

    def run(c):
        lwe_2n, got = _cbt_device(hip, c)
        assert np.array_equal(lwe_2n, want_2n), (label, "mod_switch_2n: device != oracle")
        assert np.array_equal(got, want), (label, "circuit bootstrap: device != oracle")
        return lwe_2n, got

    def run_end(c, ggsw, cts):
        end = _cbt_end_device(hip, c, ggsw, cts)
        assert np.array_equal(end, lc.run_cbt_end_oracle(ref, c, ggsw, cts)), (label, "external product: device != oracle")
        return end
    lc.check_cbt_on(run, run_end, label, c, fail=fail)


# (N, rank, n_lwe, block, bases): the reference's shape with its five bases, its one-base twin on a short LWE, rank 2 at N = 1024
CBT_SHAPES = [(256, 1, 77, 7, lc.REF_CBT_BASES), (256, 1, 14, 7, lc.ONE_BASE), (1024, 2, 14, 7, lc.ONE_BASE)]


@pytest.mark.parametrize("mode", ["constant", "exponent"])
@pytest.mark.parametrize("shape", CBT_SHAPES, ids=lambda s: f"n{s[0]}-rank{s[1]}-bases{'-'.join(map(str, s[4]))}")
def test_circuit_bootstrap_decrypts(mods, shape, mode):
    n, rank, n_lwe, block_size, bases = shape
    ref, hip = mods(n)
    _run_cbt(ref, hip, ("circuit bootstrap", mode) + shape, lc.cbt_case(n, rank, n_lwe, block_size, bases, mode, seed=600 + n + rank))


@pytest.mark.parametrize("label,kw,fail", lc.CBT_CONTROLS, ids=[c[0] for c in lc.CBT_CONTROLS])
def test_circuit_bootstrap_controls_on_device(mods, label, kw, fail):
    ref, hip = mods(kw["n"])
    _run_cbt(ref, hip, label, lc.cbt_case(**kw, seed=700), fail=fail)
