#!/usr/bin/env python3
"""Secondary measurement: GLWE x plaintext (glwe_mul_plain, poulpy-core/src/operations/glwe.rs:184-247) and GLWE x constant (glwe_mul_const
:66-96, or poulpy-ckks's complex constant leveled/default/mul.rs:342-377 with --complex) per second on one MI355X.  Device-resident
ciphertexts in and out; a few outputs are compared bit for bit with the oracle's composition (tests/plain_oracle.py).

    python tools/bench_mul_plain.py --op plain|const [--n 65536] [--limbs 16] [--pt-limbs 3] [--base2k 12] [--batch 256] [--shared]
                                    [--complex] [--cnv-offset K] [--path fused|composed] [--steps 10] [--warmup 2]

Shapes: CKKS (default): N = 2^16, rank 1, 16 limbs, base2k 12, a 3-limb plaintext / 3-digit constant, cnv_offset = b.max_k (get_mul_pt_params,
mul.rs:480-496, with res_offset = 0).  poulpy-bench's: --pt-limbs 16 --cnv-offset 0 (the plaintext has the ciphertext's layout).
--path fused: pz_glwe_mul_plain_batched / pz_glwe_mul_const_batched, one call for the batch.  --path composed: the per-op C ABI sequence the
reference's default composes, one ciphertext and one column at a time (cnv_prepare_left / right, cnv_apply_dft, idft_apply_consume,
big_normalize; cnv_by_const_apply + big_normalize), on the same device buffers.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=("plain", "const"), default="plain")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--pt-limbs", type=int, default=3)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shared", action="store_true", help="plain: one plaintext for the whole batch")
    ap.add_argument("--complex", action="store_true", help="const: re + i im (poulpy-ckks ckks_mul_pt_const_znx_into_default)")
    ap.add_argument("--cnv-offset", type=int, default=None)
    ap.add_argument("--path", choices=("fused", "composed"), default="fused")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parity-samples", type=int, default=2)
    args = ap.parse_args()
    import torch
    from poulpy_amd.hal import GlweMulConstParams, GlweTensorParams, Module
    from poulpy_amd.layouts import VecZnx
    from tests import plain_oracle as po

    n, size, bs, k, rank, B = args.n, args.limbs, args.pt_limbs, args.base2k, 1, args.batch
    cols = rank + 1
    off = bs * k if args.cnv_offset is None else args.cnv_offset
    dev = torch.device("cuda:0")
    mod = Module(n, device=0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x9a11)
    half = 1 << (k - 1)
    a = torch.randint(-half, half, (B, size, cols, n), dtype=torch.int64, device=dev, generator=g)
    res = torch.zeros((B, size, cols, n), dtype=torch.int64, device=dev)
    npt = 1 if args.shared else B
    pt = torch.randint(-half, half, (npt, bs, 1, n), dtype=torch.int64, device=dev, generator=g)
    rng = np.random.default_rng(7)
    re = rng.integers(-half, half, bs, dtype=np.int64)
    im = rng.integers(-half, half, bs, dtype=np.int64) if args.complex else None
    torch.cuda.synchronize()
    if args.path == "composed" and args.op == "const" and args.complex:
        raise SystemExit("--path composed measures glwe_mul_const (the re arm); --complex goes with --path fused")
    tp = GlweTensorParams(rank=rank, a_size=size, b_size=bs, ab_base2k=k, a_effective_k=size * k, b_effective_k=bs * k, res_size=size, res_base2k=k,
                          cnv_offset=off)
    cp = GlweMulConstParams(rank=rank, a_size=size, a_base2k=k, res_size=size, res_base2k=k, cnv_offset=off)
    hi, lo = po.offset_split(off, k)
    dft = size + bs - hi
    lib, h = mod.lib, mod.handle
    vp, sz = C.c_void_p, C.c_size_t
    ct_b, pt_b = size * cols * n * 8, bs * n * 8
    pa = torch.empty(cols * size * n, dtype=torch.float64, device=dev)
    pb = torch.empty(bs * n, dtype=torch.float64, device=dev)
    rd = torch.empty(max(dft, 1) * n, dtype=torch.float64, device=dev)
    bconst = np.ascontiguousarray(re)

    def run():
        if args.path == "fused":
            if args.op == "plain":
                mod.glwe_mul_plain_batched(vp(res.data_ptr()), vp(a.data_ptr()), vp(pt.data_ptr()), args.shared, tp, "into", B)
            else:
                mod.glwe_mul_const_batched(vp(res.data_ptr()), vp(a.data_ptr()), re, im, cp, "into", B)
            return
        for t in range(B):
            ra, rr = a.data_ptr() + t * ct_b, res.data_ptr() + t * ct_b
            if args.op == "plain":
                mod._ck(lib.pz_cnv_prepare_left(h, vp(pa.data_ptr()), sz(cols), sz(size), vp(ra), sz(cols), sz(size), C.c_int64(-1)))
                mod._ck(lib.pz_cnv_prepare_right(h, vp(pb.data_ptr()), sz(1), sz(bs), vp(pt.data_ptr() + (0 if args.shared else t * pt_b)), sz(1), sz(bs),
                                                 C.c_int64(-1)))
                for c in range(cols):
                    mod._ck(lib.pz_cnv_apply_dft(h, sz(hi), vp(rd.data_ptr()), sz(1), sz(dft), sz(0), vp(pa.data_ptr()), sz(cols), sz(size), sz(c),
                                                 vp(pb.data_ptr()), sz(1), sz(bs), sz(0)))
                    mod._ck(lib.pz_vec_znx_idft_apply_consume(h, vp(rd.data_ptr()), sz(1), sz(dft)))
                    mod._ck(lib.pz_vec_znx_big_normalize(h, vp(rr), sz(cols), sz(size), sz(k), C.c_int64(lo), sz(c), vp(rd.data_ptr()), sz(1), sz(dft),
                                                         sz(k), sz(0)))
            else:
                for c in range(cols):
                    mod._ck(lib.pz_cnv_by_const_apply(h, sz(hi), vp(rd.data_ptr()), sz(1), sz(dft), sz(0), vp(ra), sz(cols), sz(size), sz(c),
                                                      bconst.ctypes.data_as(vp), sz(bs)))
                    mod._ck(lib.pz_vec_znx_big_normalize(h, vp(rr), sz(cols), sz(size), sz(k), C.c_int64(lo), sz(c), vp(rd.data_ptr()), sz(1), sz(dft),
                                                         sz(k), sz(0)))

    for _ in range(args.warmup):
        run()
    mod.sync()
    mod.dispatch_notes(reset=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    mod.sync()
    dt = (time.perf_counter() - t0) / args.steps
    notes = mod.dispatch_notes()
    mod.set_kernel_timing(True)
    run()
    mod.sync()
    stats = {kname: [c, round(ms, 3)] for kname, (c, ms) in mod.kernel_stats().items() if c}
    mod.set_kernel_timing(False)
    margin = mod.rounding_margin_of(run) if args.op == "plain" else 0.0
    ok = None
    if args.parity_samples:
        from oracle.ref import RefModule
        ref = RefModule(n)
        ok = True
        got = res.cpu().numpy()
        for t in sorted(set(np.linspace(0, B - 1, args.parity_samples).astype(int).tolist())):
            av = VecZnx(n, cols, size, a[t].cpu().numpy().copy())
            want = VecZnx(n, cols, size)
            if args.op == "plain":
                pv = VecZnx(n, 1, bs, pt[0 if args.shared else t].cpu().numpy().copy())
                po.glwe_mul_plain(ref, off, want, k, av, size * k, pv, bs * k, k)
            else:
                po.ckks_mul_pt_const_into(ref, off, want, k, av, k, re, im)
            ok = ok and bool(np.array_equal(got[t], want.data))
    # algorithmic bytes per ciphertext: a read once, res written once, the plaintext read once per ciphertext (or once per call when shared)
    nbytes = 2 * ct_b + (0 if (args.op == "const" or args.shared) else pt_b) + (pt_b / B if args.op == "plain" and args.shared else 0)
    rate = B / dt
    print(json.dumps({
        "metric": f"GLWE x {'plaintext' if args.op == 'plain' else 'constant'} / s ({args.path})", "value": rate, "unit": "calls/s",
        "ms_per_call": dt * 1e3, "batch": B, "parity_ok": ok, "rounding_margin": margin,
        "config": {"op": args.op, "path": args.path, "n": n, "rank": rank, "limbs": size, "pt_limbs": bs, "base2k": k, "cnv_offset": off,
                   "shared": args.shared, "complex": args.complex},
        "kernel_classes_launches_ms": stats, "dispatch_notes": notes,
        "knobs": {k_: v_ for k_, v_ in os.environ.items() if k_.startswith("POULPY_DBG_")},
        "roofline": {"bound": "hbm", "algorithmic_bytes_per_unit": nbytes, "achieved": rate * nbytes / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": rate * nbytes / 1e9 / 8000.0}}), flush=True)
    if ok is False:
        raise SystemExit(3)   # a fast wrong answer is not a result


if __name__ == "__main__":
    main()
