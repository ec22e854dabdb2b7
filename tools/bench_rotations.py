#!/usr/bin/env python3
"""Secondary measurement: rotations of ONE ciphertext batch by many Galois elements per second on one MI355X - the hoisted call
(pz_glwe_automorphism_many_batched) against `nrot` calls of pz_glwe_automorphism_batched on the same inputs, in the same
process, keys pinned in both.  Rotation 0 of ciphertext 0 is compared bit for bit with the oracle, and the two routes with each other.

    python tools/bench_rotations.py [--n 65536] [--limbs 16] [--base2k 12] [--batch 512] [--nrot 8] [--gpus 1] [--steps 5] [--warmup 2]

Prints one JSON line: rotations/s of both routes, their ratio, the dispatch notes and the per-class kernel times (kernel_stats) of one
extra, event-timed execution of each route.  POULPY_DBG_ROT_HOIST=0 in the environment makes the first figure the loop inside the call.
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
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--nrot", type=int, default=8)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_rotations.py measures one device (--gpus 1)")
    import torch
    from poulpy_amd.hal import GlweOpParams, Module
    from poulpy_amd.layouts import MatZnx, VecZnx

    n, size, k, batch, nrot, rank = args.n, args.limbs, args.base2k, args.batch, args.nrot, 1
    cols = rank + 1
    dev = torch.device("cuda:0")
    mod = Module(n, device=0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x726f74)
    half = 1 << (k - 1)
    a = torch.randint(-half, half, (batch, size, cols, n), dtype=torch.int64, device=dev, generator=g)
    res = torch.zeros((nrot, batch, size, cols, n), dtype=torch.int64, device=dev)
    res2 = torch.zeros((batch, size, cols, n), dtype=torch.int64, device=dev)   # the single calls' result, one rotation at a time
    # the baby steps of a baby-step / giant-step transform: 5^1 .. 5^(nrot-1), and conjugation last
    gals = [pow(5, r + 1, 2 * n) for r in range(nrot - 1)] + [2 * n - 1] if nrot > 1 else [5]
    rng = np.random.default_rng(17)
    # one set of key digits prepared once, in nrot device buffers of their own: every rotation streams (and has pinned) a different key
    mat = MatZnx(n, size, rank, cols, size).fill_uniform(k, rng)
    pm = mod.vmp_pmat_alloc(size, rank, cols, size)
    mod.vmp_prepare(pm, mat)
    d_keys = []
    for r in range(nrot):
        d_keys.append(mod.device_alloc(pm.data.nbytes).upload(pm.data))
        mod.pin_key(d_keys[-1].ptr, size, rank, cols, size)
    keys = [d.ptr for d in d_keys]
    p = GlweOpParams(rank=rank, dnum=size, dsize=1, key_size=size, key_base2k=k, a_size=size, a_base2k=k, res_size=size, res_base2k=k, rank_out=rank)
    vp = C.c_void_p

    def many():
        mod.glwe_automorphism_many_batched(vp(res.data_ptr()), vp(a.data_ptr()), gals, keys, p, batch)

    def loop():
        for r in range(nrot):
            mod.glwe_automorphism_batched(vp(res2.data_ptr()), vp(a.data_ptr()), keys[r], p, gals[r], "automorphism", batch)

    def measure(run):
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
        before = mod.kernel_stats()
        run()
        mod.sync()
        after = mod.kernel_stats()
        mod.set_kernel_timing(False)
        classes = {c: {"launches": after[c][0] - before[c][0], "ms": round(after[c][1] - before[c][1], 4)} for c in after if after[c][0] != before[c][0]}
        return dt, notes, classes

    # interleaved A / B / A / B so that a drift of the device shows in both
    dt_many, notes_many, cls_many = measure(many)
    dt_loop, notes_loop, cls_loop = measure(loop)
    dt_many2, _, _ = measure(many)
    dt_loop2, _, _ = measure(loop)
    same = True
    for r in range(nrot):
        mod.glwe_automorphism_batched(vp(res2.data_ptr()), vp(a.data_ptr()), keys[r], p, gals[r], "automorphism", batch)
        mod.sync()
        same = same and bool(torch.equal(res[r], res2))
    ok = None
    if not args.no_parity:
        from oracle.ref import RefModule
        ref = RefModule(n)
        pr = ref.vmp_pmat_alloc(size, rank, cols, size)
        ref.vmp_prepare(pr, mat)
        a0 = VecZnx(n, cols, size, np.ascontiguousarray(a[0].cpu().numpy()))
        want = VecZnx(n, cols, size)
        ref.glwe_automorphism(want, k, a0, k, pr, 1, k, gals[0], "automorphism")
        ok = bool(np.array_equal(res[0, 0].cpu().numpy(), want.data))
    rots = nrot * batch
    print(json.dumps({
        "metric": "rotations of one batch / s (hoisted call vs nrot single calls)", "unit": "rotations/s",
        "value": rots / min(dt_many, dt_many2), "hoisted_rotations_per_s": [rots / dt_many, rots / dt_many2],
        "loop_rotations_per_s": [rots / dt_loop, rots / dt_loop2], "hoisted_over_loop": min(dt_loop, dt_loop2) / min(dt_many, dt_many2),
        "ms_per_call": {"hoisted": [dt_many * 1e3, dt_many2 * 1e3], "loop": [dt_loop * 1e3, dt_loop2 * 1e3]},
        "routes_bit_identical": same, "parity_ok": ok,
        "config": {"n": n, "rank": rank, "limbs": size, "base2k": k, "batch": batch, "nrot": nrot, "gals": gals, "steps": args.steps, "warmup": args.warmup},
        "dispatch_notes": {"hoisted": notes_many, "loop": notes_loop}, "kernel_ms": {"hoisted": cls_many, "loop": cls_loop},
        "knobs": {k_: v_ for k_, v_ in os.environ.items() if k_.startswith("POULPY_DBG_")}}), flush=True)
    if ok is False or not same:
        raise SystemExit(3)   # a fast wrong answer is not a result


if __name__ == "__main__":
    main()
