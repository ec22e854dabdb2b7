"""The census of kernel instantiations: for every form the hot path chooses among (the X-macro lists of mid_forms.hpp, tail_plan.hpp and
br_forms.hpp, printed by tests/cpp/list_forms.cpp), the call through a public batched entry point that lands on it.

CENSUS maps the form's dispatch note - up to its closing '>' for the middle kernel and the blind-rotation kernels, the whole note for the
fused tail - to the cases that run it, or to Unreachable(reason).  tests/test_form_census_host.py holds the keys against the printed list in
both directions and re-derives what the host choosers can (the middle-kernel form and the block-step form of every case);
tests/test_gpu_form_census.py runs every case on the device, asserts the note and compares the bytes with the oracle.  A new instantiation
comes with its row here.

Nothing in this file touches a GPU: the cases are data.  `batch=None` means the middle kernel's rule (mid_batch below)."""
from __future__ import annotations

import re
from collections import namedtuple

Unreachable = namedtuple("Unreachable", "reason")

# run: "glwe" (external product / key switch / automorphism family, tests.test_gpu_parity._run_glwe_op), "br" (_run_blind_rotation),
# "tensor" / "mulrelin" (tests.test_gpu_cnv._run_tensor / _run_mul_relinearize), "trace" (the runner of test_glwe_trace_shifted_stores);
# p: the runner's parameters; sw: module switches for the call (tests.device.on_device); probe: None, or the note the same call leaves under the
# rounding-margin probe where that is not `key + " PROBE"`
Case = namedtuple("Case", "run n p batch sw probe", defaults=(None, {}, None))

KR = 6   # PZ_MIDR_KR of a default build (device_mid.hpp); the 32-slot tile has its own, 3


def mid_batch(ct: int, m1: int, cu: int) -> int:
    """The smallest batch at which the persistent grid (one workgroup per CU) is smaller than the tile count m1 * n_ct - a workgroup walks two
    tiles - and the last tile holds exactly one ciphertext."""
    n_ct = -(-(cu + 1) // m1)
    return ct * n_ct - (ct - 1)


def m1_of(n: int) -> int:
    """rows of the four-step split on the 128-point-row plans (N = 2^12 .. 2^16)"""
    return n // 2 // 128


# ---------------------------------------------------------------------------------------------------------------------------------------
# the middle kernel: external product (ep), key switch under glwe_automorphism_batched with Galois element 5 (perm), dsize > 1 (ds)
# ---------------------------------------------------------------------------------------------------------------------------------------
def ep(a, key, dnum, rank=1, dsize=1, res=None, k=12, n=8192, batch=None, **kw):
    return Case("glwe", n, dict(ks=False, rank=rank, rank_out=rank, a=a, key=key, dnum=dnum, dsize=dsize, res=res or min(a, key), k=k, auto=None), batch, **kw)


def ks(a, key, dnum, rank=1, res=None, k=12, n=8192, batch=None, auto=None, **kw):
    return Case("glwe", n, dict(ks=True, rank=rank, rank_out=rank, a=a, key=key, dnum=dnum, dsize=1, res=res or min(a, key), k=k, auto=auto), batch, **kw)


def perm(a, key, dnum, rank=1, **kw):
    return ks(a, key, dnum, rank=rank, auto=(5, "automorphism"), **kw)


def br(rank, dnum, bsz, rsz, n=8192, blk=2, k=12, batch=None, span=None, **kw):
    """blind rotation: n_lwe = 2 blk + 1 (two whole blocks; the reference drops the trailing coefficient); span: mask coefficients in [0, span)"""
    return Case("br", n, dict(rank=rank, n_lwe=2 * blk + 1, blk=blk, dnum=dnum, bsz=bsz, rsz=rsz, k=k, span=span), batch, **kw)


def glwe_mid_shape(c: Case) -> tuple:
    """(npi, npo, nrows, ncols, ds_n, br_rm, perm, ds, br) as glwe_fused / br_pipeline_path hand them to launch_mid (api_glwe.hip, api_br.hip)"""
    p = c.p
    if c.run == "br":
        cols = p["rank"] + 1
        npi = cols * min(p["dnum"], p["rsz"])
        return (npi, cols * p["bsz"], p["dnum"] * cols, cols * p["bsz"], 0, p["dnum"] * cols, 0, 0, 1)
    cols_in = p["rank"] if p["ks"] else p["rank"] + 1
    cols_out = p["rank_out"] + 1
    npi, npo, nrows = cols_in * p["a"], cols_out * p["key"], p["dnum"] * cols_in
    ds_n = 0
    if p["dsize"] > 1:   # digit_terms (api_glwe.hip)
        d = p["dsize"]
        for l in range(p["a"]):
            di = (d - 1 - l) % d
            kk = (l - (d - 1 - di)) // d
            a_sz = (p["a"] + di) // d
            if p["ks"]:
                a_sz = min(a_sz, p["dnum"])
            if kk < 0 or kk >= a_sz or kk >= p["dnum"]:
                continue
            r_sz = p["key"] - max(d - di - 2, 0)
            off = di * cols_out
            if off < npo and min(cols_out * r_sz, npo - off) > 0:
                ds_n += cols_in
    return (npi, npo, nrows, npo, ds_n, 0, int(p["auto"] is not None), int(p["dsize"] > 1), 0)


_R = "k_mid128r<CT=%d,NP=%d,PERM=%d,NR=%d,HALFIN=%d,KR=%d>"
_M = "k_mid128<CT=%d,NP=%d,PERM=%d,DS=0,BR=0,SKIPW=%d>"

MID = {
    # k_mid128r: product rows = the tile's slots or half of them (HALFIN: no input in the upper half)
    _R % (8, 8, 0, 8, 0, KR): ep(4, 4, 4),
    _R % (8, 8, 1, 8, 0, KR): perm(8, 4, 8),
    _R % (4, 16, 0, 16, 0, KR): ep(8, 5, 8),
    _R % (4, 16, 0, 8, 1, KR): ep(4, 5, 4),
    _R % (4, 16, 0, 8, 0, KR): ep(5, 5, 4),
    _R % (4, 16, 1, 16, 0, KR): perm(16, 6, 16),
    _R % (4, 16, 1, 8, 1, KR): perm(8, 5, 8),
    _R % (4, 16, 1, 8, 0, KR): perm(10, 5, 8),
    _R % (2, 32, 0, 32, 0, 3): ep(16, 13, 16),
    _R % (2, 32, 0, 16, 1, 3): ep(8, 9, 8),
    _R % (2, 32, 0, 16, 0, 3): ep(13, 13, 8),
    _R % (2, 32, 1, 32, 0, 3): perm(16, 9, 16, rank=2),
    _R % (2, 32, 1, 16, 1, 3): perm(16, 9, 16),
    _R % (2, 32, 1, 16, 0, 3): perm(13, 9, 8, rank=2),
    "k_mid128r<CT=4,NP=16,NR=16,HALFIN=0,KR=%d,DS=1>" % KR: ep(8, 5, 4, dsize=2),          # 16 terms on 16 inputs
    "k_mid128r<CT=4,NP=16,NR=8,HALFIN=1,KR=%d,DS=1>" % KR: ep(4, 5, 2, dsize=4),           # 8 terms on 8 inputs
    "k_mid128r<CT=4,NP=16,PERM=0,NR=16,HALFIN=0,KR=%d,C2=1>" % KR: ep(8, 16, 8),           # 16 in, 32 out: two output-column passes
    "k_mid128r<CT=4,NP=16,PERM=1,NR=16,HALFIN=0,KR=%d,C2=1>" % KR: perm(16, 16, 16),
    # k_mid128: every other row count; SKIPW: a short side leaves waves idle
    _M % (8, 8, 0, 0): ep(3, 3, 3),
    _M % (8, 8, 1, 0): perm(4, 4, 4),
    _M % (4, 16, 0, 0): ep(5, 5, 3),
    _M % (4, 16, 1, 0): perm(10, 5, 6),
    _M % (4, 16, 0, 1): ep(2, 6, 2),
    _M % (4, 16, 1, 1): perm(4, 6, 4),
    _M % (2, 32, 0, 0): ep(13, 13, 5),
    _M % (2, 32, 1, 0): perm(13, 9, 5, rank=2),
    _M % (2, 32, 0, 1): ep(1, 9, 1, res=3),
    _M % (2, 32, 1, 1): perm(4, 9, 4),
    "k_mid128<CT=8,NP=8,DS=1>": ep(4, 4, 2, dsize=2),
    "k_mid128<CT=4,NP=16,DS=1>": ep(6, 6, 3, dsize=2),                                     # 12 terms
    "k_mid128<CT=2,NP=32,DS=1>": ep(9, 9, 5, dsize=2),
    # the blind-rotation block step on the pipeline: an even number of key rows per GGSW nests the product loop (not on the 32-slot tile),
    # six output columns in the 8-slot tile are 2 x 3 per thread
    "k_mid128<CT=8,NP=8,BR=1>": br(2, 1, 2, 2),
    "k_mid128<CT=4,NP=16,BR=1>": br(2, 3, 3, 3),
    "k_mid128<CT=2,NP=32,BR=1>": br(1, 2, 9, 2),
    "k_mid128<CT=8,NP=8,BR=1,BRNEST=2>": br(1, 2, 2, 2),
    "k_mid128<CT=4,NP=16,BR=1,BRNEST=2>": br(1, 3, 5, 3),
    "k_mid128<CT=8,NP=8,BR=1,BRNEST=2,NCO=3>": br(1, 3, 3, 3),
}
# every k_mid128r form and one k_mid128 form per tile geometry once more at the two ring degrees between the default and N = 2^16
MID_OTHER_RINGS = [k for k in MID if k.startswith("k_mid128r<")] + [_M % (8, 8, 0, 0), _M % (4, 16, 0, 0), _M % (2, 32, 0, 0)]

# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused tail: small batches (batch x columns no multiple of 8: the XCD padding), chunk 2 (a short last wave), 3 - 5 limbs
# ---------------------------------------------------------------------------------------------------------------------------------------
TAIL_RINGS = {(4, 8, 16): 8192, (8, 8, 16): 16384, (8, 16, 16): 32768, (16, 16, 16): 65536}   # PZ_RSH_CASES: the 128-point-row plans
_GATED = "tail_plan_whole_waves(f1b, cb) is false for this plan and every caller of the fused tail asks tail_supported() first"
_NO_RING = "make_plan (module.hpp) gives no ring degree this plan: "


def _t(plan, what):
    return "k_inv_tail<%d,%d,%d> %s" % (*plan, what)


def tensor(n, k, mode="apply"):
    return Case("tensor", n, dict(rank=1, a=3, b=4, res=4, k=k, off=2 * k, mode=mode), 3, dict(chunk=2))


def mulrelin(n, k=12):
    return Case("mulrelin", n, dict(rank=1, a=3, b=4, t=4, k=k, off=2 * k, key=4, dnum=4, res=4, mode="apply"), 3, dict(chunk=2))


def trace(n, k=12):
    return Case("trace", n, dict(size=3, key=4, gals=[5, 25], k=k), 2)


TAIL = {}
for _plan in [(4, 1, 4), (8, 1, 4), (8, 1, 16), (16, 1, 16)]:
    for _v in ("PLAIN(0,0)", "PLAIN(0,1)", "PLAIN(1,0)", "PLAIN(1,1)"):
        TAIL[_t(_plan, _v)] = Unreachable(_GATED)
for _v in ("PLAIN(0,0)", "PLAIN(0,1)", "PLAIN(1,0)", "PLAIN(1,1)"):
    TAIL[_t((8, 16, 8), _v)] = Unreachable(_NO_RING + "its column block is 16 wherever a row has 16 points or more, else 4")
# the pipeline (row-major T2') and, with the middle kernel's fusion off, the per-op product in front of the tail (standard layout); the key
# switch's body column is the one launch with an operand.  N = 512 / 2048 share the radices of N = 4096 / 8192
for _plan, _n_rm, _n_std, _sw in [((4, 4, 16), 4096, 512, dict(small_path=False)), ((4, 8, 16), 8192, 2048, {}), ((8, 8, 16), 16384, 16384, {}),
                                  ((8, 16, 16), 32768, 32768, {}), ((16, 16, 16), 65536, 65536, {})]:
    TAIL[_t(_plan, "PLAIN(1,0)")] = ep(3, 4, 3, res=5, k=13, n=_n_rm, batch=3, sw=dict(chunk=2, **_sw))
    TAIL[_t(_plan, "PLAIN(1,1)")] = ks(4, 3, 4, res=4, k=13, n=_n_rm, batch=3, sw=dict(chunk=2, **_sw))
    TAIL[_t(_plan, "PLAIN(0,0)")] = ep(3, 4, 3, res=5, k=13, n=_n_std, batch=3, sw=dict(chunk=2, fuse=(True, False)))
    TAIL[_t(_plan, "PLAIN(0,1)")] = ks(4, 3, 4, res=4, k=13, n=_n_std, batch=3, sw=dict(chunk=2, fuse=(True, False)))
    # 32-bit accumulator digits between the blocks of a blind rotation (base2k 16 .. 31).  The rotation amounts are the middle kernel's
    # business (its BR rows draw them from the whole range): from N = 2^14 on, where the oracle's monomial table passes a GiB, they stay below 64
    TAIL[_t(_plan, "ACC32")] = [br(1, 2, 2, 2, n=_n_rm, k=16, batch=3, span=64 if _n_rm >= 16384 else None)]
for _plan, _n in TAIL_RINGS.items():
    # the steps of a trace: the one-bit shift rides on the store; the body column's operand as 16-bit copies (base2k <= 14).  The probe keeps the
    # i64 operand (spectral_body16, api_glwe.hip), so no call reaches the probing instantiations of the two 16-bit-operand forms
    TAIL[_t(_plan, "RSH")] = trace(_n)
    TAIL[_t(_plan, "SGN16R")] = trace(_n)._replace(probe=_t(_plan, "RSH") + " PROBE")
    # the plain spectral automorphism: signs only on the mask columns, the 16-bit operand on the body column
    TAIL[_t(_plan, "SGN")] = ks(3, 4, 3, res=4, k=13, n=_n, batch=3, auto=(5, "automorphism"), sw=dict(chunk=2))
    TAIL[_t(_plan, "SGN16")] = ks(3, 4, 3, res=4, k=13, n=_n, batch=3, auto=(5, "automorphism"), sw=dict(chunk=2), probe=_t(_plan, "PLAIN(1,1)") + " PROBE")
    # tensoring: diagonal (NZ1) and pairwise (NZ2) launches; above 16 bits no side copies, up to 16 the diagonal launch writes 16-bit copies (W)
    # that the pairwise one reads (R); the one-call product with the relinearization keeps the tensor as 16-bit digits only (O, base2k <= 14)
    # and its tail adds them (ACC32's 16-bit operand)
    TAIL[_t(_plan, "NZ1")] = tensor(_n, 17)
    TAIL[_t(_plan, "NZ2")] = tensor(_n, 17)
    TAIL[_t(_plan, "NZ1W")] = tensor(_n, 12)
    TAIL[_t(_plan, "NZ2R")] = tensor(_n, 12)
    TAIL[_t(_plan, "NZ1O")] = mulrelin(_n)
    TAIL[_t(_plan, "NZ2O")] = mulrelin(_n)
    TAIL[_t(_plan, "ACC32")].append(mulrelin(_n))

# ---------------------------------------------------------------------------------------------------------------------------------------
# blind rotation as one kernel (N = 256 / 512 / 1024 for R0 = 2 / 4 / 8): "cu+1" / "2cu+1" are batches relative to the device's CU count
# ---------------------------------------------------------------------------------------------------------------------------------------
_F = "k_br_fused<R0=%d,CT=%d,NT=512,PJ=%d,MR=%d,CG=%d,A32=%d>"
_H = "k_br_fused<R0=4,CT=1,NT=256,PJ=2,MR=%d,CG=%d,A32=0>"
_S = "k_br_fused<R0=%d,CT=1,NT=512,PJ=%d,MR=%d,CG=%d,A32=0,STD=1>"
BR_FUSED = {
    _F % (2, 1, 1, 4, 4, 0): br(1, 2, 2, 2, n=256, batch=3),
    _F % (2, 1, 1, 6, 3, 0): br(1, 3, 3, 3, n=256, batch=3),
    _F % (4, 1, 1, 4, 4, 0): br(1, 2, 2, 2, n=512, batch=3),
    _F % (4, 1, 1, 6, 3, 0): br(1, 3, 3, 3, n=512, batch=3),
    # two ciphertexts per workgroup above one ciphertext per CU; 32-bit accumulators (A32) where the 64-bit ones of two ciphertexts no longer fit LDS
    _F % (4, 2, 1, 4, 4, 0): br(1, 2, 2, 2, n=512, batch="cu+1"),
    _F % (4, 2, 1, 6, 3, 0): br(1, 3, 3, 3, n=512, batch="cu+1"),
    _F % (4, 2, 1, 4, 4, 1): br(1, 2, 2, 9, n=512, batch="cu+1"),
    _F % (4, 2, 1, 6, 3, 1): br(1, 3, 3, 7, n=512, batch="cu+1"),
    _F % (8, 1, 1, 4, 4, 0): br(1, 2, 2, 2, n=1024, batch=3),
    _F % (8, 1, 1, 6, 3, 0): br(2, 2, 1, 2, n=1024, batch=3),          # PJ = 1 with groups of 3: three output columns
    _F % (8, 1, 2, 4, 4, 0): br(1, 2, 4, 2, n=1024, batch=3),
    _F % (8, 1, 2, 6, 3, 0): br(1, 3, 3, 3, n=1024, batch=3),
    _F % (8, 2, 1, 4, 4, 0): br(1, 2, 2, 2, n=1024, batch="cu+1"),
    _F % (8, 2, 1, 6, 3, 0): br(2, 1, 1, 1, n=1024, batch="cu+1"),
    _F % (8, 2, 2, 6, 3, 0): br(1, 1, 3, 1, n=1024, batch="cu+1"),
    _F % (8, 2, 1, 4, 4, 1): br(1, 2, 2, 3, n=1024, batch="cu+1"),
    _F % (8, 2, 1, 6, 3, 1): br(2, 1, 1, 3, n=1024, batch="cu+1"),
    _F % (8, 2, 2, 6, 3, 1): br(1, 2, 3, 2, n=1024, batch="cu+1"),
    # 256 threads, one ciphertext per workgroup: a last wave of two-ciphertext workgroups at most half full (batch mod 2 CUs in 1 .. CUs)
    _H % (4, 4): br(1, 2, 4, 2, n=512, batch="2cu+1"),
    _H % (6, 3): br(1, 3, 3, 3, n=512, batch="2cu+1"),
    # execute_standard (block size 1)
    _S % (2, 1, 4, 4): br(1, 2, 2, 2, n=256, blk=1, batch=3),
    _S % (2, 1, 6, 3): br(1, 3, 3, 3, n=256, blk=1, batch=3),
    _S % (4, 1, 4, 4): br(1, 2, 2, 2, n=512, blk=1, batch=3),
    _S % (4, 1, 6, 3): br(1, 3, 3, 3, n=512, blk=1, batch=3),
    _S % (8, 1, 4, 4): br(1, 2, 2, 2, n=1024, blk=1, batch=3),
    _S % (8, 1, 6, 3): br(2, 2, 1, 2, n=1024, blk=1, batch=3),
    _S % (8, 2, 4, 4): br(1, 2, 4, 2, n=1024, blk=1, batch=3),
    _S % (8, 2, 6, 3): br(1, 2, 3, 2, n=1024, blk=1, batch=3),
}

# the block step of the composed path: keys staged in LDS on rings with m % 64 == 0 (N = 128: no one-kernel form), from HBM below (N = 64)
_BLOCK_SHAPES = {(12, 2): (2, 4, 1, 4), (9, 3): (2, 3, 1, 3), (9, 4): (2, 3, 4, 3), (6, 3): (1, 3, 3, 3), (8, 3): (1, 4, 3, 4), (4, 4): (1, 2, 2, 2),
                 (8, 4): (1, 4, 2, 4)}   # (MR, CG): rank, dnum, key limbs, result limbs
BR_BLOCK = {}
for (_mr, _cg), _s in _BLOCK_SHAPES.items():
    BR_BLOCK["k_br_block_lds<2,MR=%d,CG=%d>" % (_mr, _cg)] = br(*_s, n=128, batch=3)
    if (_mr, _cg) != (9, 4):   # (without LDS the form is not built: br_block_form reports none and the composed loop runs)
        BR_BLOCK["k_br_block<2,MR=%d,CG=%d>" % (_mr, _cg)] = br(*_s, n=64, batch=3)


def block_shape(c: Case) -> tuple:
    """(row_max, ncols) as br_composed_path hands them to br_block_step (api_br.hip)"""
    cols = c.p["rank"] + 1
    return cols * min(c.p["dnum"], c.p["rsz"]), cols * c.p["bsz"]


CENSUS = {}
for _d in (MID, TAIL, BR_FUSED, BR_BLOCK):
    for _k, _v in _d.items():
        assert _k not in CENSUS, _k
        CENSUS[_k] = _v if isinstance(_v, (list, Unreachable)) else [_v]


def ct_of(key: str) -> int:
    return int(re.search(r"CT=(\d+)", key).group(1))


def device_cases():
    """[(id, key, case)]: every reachable entry's cases, then the middle-kernel forms of MID_OTHER_RINGS at N = 2^14 and 2^15"""
    out = []
    for key, cases in CENSUS.items():
        if isinstance(cases, Unreachable):
            continue
        for i, c in enumerate(cases):
            out.append(("%s%s" % (key, "" if len(cases) == 1 else "#%d" % i), key, c))
    for n in (16384, 32768):
        for key in MID_OTHER_RINGS:
            out.append(("%s@%d" % (key, n), key, MID[key]._replace(n=n)))
    return out
