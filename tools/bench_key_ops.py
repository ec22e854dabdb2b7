#!/usr/bin/env python3
"""Secondary measurement: the key-level forms of key switching per second on one MI355X - automorphism-key compositions
(glwe_automorphism_key_automorphism, poulpy-core automorphism/gglwe_atk.rs:42-155), GGSW key switches (keyswitching/ggsw.rs:37-85) and GGSW
automorphisms (automorphism/ggsw_ct.rs:32-82).  Device-resident keys in and out; the first GGLWE / GGSW is compared bit for bit with the
oracle's composition (tests/key_ops_cases.py).

    python tools/bench_key_ops.py --op atk|ggsw_ks|ggsw_auto [--path batched|per-entry] [--n 65536] [--limbs 16] [--dnum 16] [--base2k 12]
                                  [--count 1] [--gal -5] [--steps 10] [--warmup 2]

--path batched: one call of the new entry point for `count` keys (POULPY_DBG_KEYAUTO_SPECTRAL=1 / =0 in the environment chooses the key switch by
the permuted key / the composition behind pz_glwe_automorphism_key_automorphism_batched on the same build).  --path per-entry: the route a caller had before these entry points:
atk: pz_vec_znx_automorphism per column of every entry, one pz_glwe_keyswitch_batched over the entries, pz_vec_znx_automorphism_assign per
column again; ggsw_*: pz_glwe_keyswitch_batched / pz_glwe_automorphism_batched once per (row, 0) entry, then pz_ggsw_expand_row_batched.
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
    ap.add_argument("--op", choices=("atk", "ggsw_ks", "ggsw_auto"), default="atk")
    ap.add_argument("--path", choices=("batched", "per-entry"), default="batched")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--dnum", type=int, default=16)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--count", type=int, default=1)
    ap.add_argument("--gal", type=int, default=-5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    import torch
    from poulpy_amd.hal import GlweOpParams, Module
    from poulpy_amd.layouts import MatZnx
    from tests import key_ops_cases as kc

    n, size, dnum, k, rank, count, gal = args.n, args.limbs, args.dnum, args.base2k, 1, args.count, args.gal
    cols = rank + 1
    cols_in = rank if args.op == "atk" else cols
    dev = torch.device("cuda:0")
    mod = Module(n, device=0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x6b65)
    half = 1 << (k - 1)
    a = torch.randint(-half, half, (count, dnum, cols_in, size, cols, n), dtype=torch.int64, device=dev, generator=g)
    res = torch.zeros_like(a)
    rng = np.random.default_rng(11)
    keys_np = [rng.integers(-half, half, (dnum, rank, size, cols, n), dtype=np.int64) for _ in range(1 + rank)]
    pms = [kc.prepare(mod, kk) for kk in keys_np]
    d_keys = [mod.device_alloc(p.data.nbytes).upload(p.data) for p in pms]
    key, tsk = d_keys[0].ptr, [d.ptr for d in d_keys[1:]]
    p = GlweOpParams(rank=rank, dnum=dnum, dsize=1, key_size=size, key_base2k=k, a_size=size, a_base2k=k, res_size=size, res_base2k=k, rank_out=rank)
    lib, h = mod.lib, mod.handle
    vp, sz = C.c_void_p, C.c_size_t
    ct_b = size * cols * n * 8
    ginv = pow(gal % (2 * n), -1, 2 * n)
    tmp = torch.empty_like(a)

    def run():
        if args.path == "batched":
            if args.op == "atk":
                mod.glwe_automorphism_key_automorphism_batched(vp(res.data_ptr()), dnum, vp(a.data_ptr()), dnum, gal, key, -5, p, count)
            elif args.op == "ggsw_ks":
                mod.ggsw_keyswitch_batched(vp(res.data_ptr()), vp(a.data_ptr()), dnum, key, tsk, p, p, count)
            else:
                mod.ggsw_automorphism_batched(vp(res.data_ptr()), dnum, vp(a.data_ptr()), dnum, key, gal, tsk, p, p, count)
            return
        ents = count * dnum * cols_in
        if args.op == "atk":
            for e in range(ents):
                for c in range(cols):
                    mod._ck(lib.pz_vec_znx_automorphism(h, C.c_int64(gal), vp(tmp.data_ptr() + e * ct_b), sz(cols), sz(size), sz(c),
                                                        vp(a.data_ptr() + e * ct_b), sz(cols), sz(size), sz(c)))
            mod.glwe_keyswitch_batched(vp(res.data_ptr()), vp(tmp.data_ptr()), key, p, ents)
            for e in range(ents):
                for c in range(cols):
                    mod._ck(lib.pz_vec_znx_automorphism_assign(h, C.c_int64(ginv), vp(res.data_ptr() + e * ct_b), sz(cols), sz(size), sz(c)))
            return
        for e in range(0, ents, cols):   # the entries (row, 0), one call each: they are not contiguous
            ra, rr = vp(a.data_ptr() + e * ct_b), vp(res.data_ptr() + e * ct_b)
            if args.op == "ggsw_ks":
                mod.glwe_keyswitch_batched(rr, ra, key, p, 1)
            else:
                mod.glwe_automorphism_batched(rr, ra, key, p, gal % (2 * n), "automorphism", 1)
        mod.ggsw_expand_row_batched(vp(res.data_ptr()), dnum, tsk, p, count)

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
    ok = None
    if not args.no_parity:
        from oracle.ref import RefModule
        ref = RefModule(n)
        rp = [kc.prepare(ref, kk) for kk in keys_np]
        a0 = a[0].cpu().numpy()
        if args.op == "atk":
            want = kc.key_composition(ref, a0, k, gal, rp[0], 1, k, dnum, size)
        elif args.op == "ggsw_ks":
            want = kc.ggsw_keyswitch(ref, a0, k, rp[0], 1, k, rp[1:], size)
        else:
            want = kc.ggsw_automorphism(ref, a0, k, rp[0], 1, k, gal, rp[1:], dnum, size)
        ok = bool(np.array_equal(res[0].cpu().numpy(), want))
    glwes = count * dnum * cols_in if args.op == "atk" else count * dnum * cols
    print(json.dumps({
        "metric": {"atk": "automorphism-key compositions", "ggsw_ks": "GGSW key switches", "ggsw_auto": "GGSW automorphisms"}[args.op] + f" / s ({args.path})",
        "value": count / dt, "unit": "keys/s", "glwe_per_s": glwes / dt, "ms_per_call": dt * 1e3, "count": count, "parity_ok": ok,
        "config": {"op": args.op, "path": args.path, "n": n, "rank": rank, "limbs": size, "dnum": dnum, "base2k": k, "gal": gal},
        "dispatch_notes": notes, "knobs": {k_: v_ for k_, v_ in os.environ.items() if k_.startswith("POULPY_DBG_")}}), flush=True)
    if ok is False:
        raise SystemExit(3)   # a fast wrong answer is not a result


if __name__ == "__main__":
    main()
