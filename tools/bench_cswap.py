#!/usr/bin/env python3
"""Secondary measurement: conditional swaps per second on one MI355X (pz_glwe_cswap_batched), an A/B in one process on one device.

    A  pz_glwe_cswap_batched(a, b)                                       the gate: ONE product of b - a, both results from its big value, in place
    B  pz_glwe_cmux_batched(ta, t = b, f = a) and pz_glwe_cmux_batched(tb, t = a, f = b)   the same pairs into two temporaries: TWO products
    A' A again                                                            the run-to-run spread of the identical leg

B is the only composition the library offered before this entry point.  It is NOT bit-identical to the swap (two products of +-D, other
digits), so only rates are compared.  The legs alternate (A B A' B ...) `--rounds` times, every leg warmed, every window at least `--window`
seconds of device work ending in a synchronise.  Reported per shape: every window's rate, the medians, A / B, and the spread of each leg over
the alternations ((max - min) / median).  The swap works in place, so leg A's inputs are its previous outputs - normalized digits again; its
first call, on fresh inputs, is compared bit for bit with the oracle on pair 0 and with the materialised route (POULPY_DBG_CMUX_FUSED=0, set
between calls in this process), which is timed in the same rounds.

    python tools/bench_cswap.py [--shapes 1024:3,2048:3,4096:4] [--batch 4096] [--rounds 5] [--window 0.5] [--gpus 1]
    python tools/bench_cswap.py --network [--batch 128]     a 5-level retrieval over 32 slots at N = 1024: one composite call against its 5 single calls

Prints one JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_cmux import setup, timed  # noqa: E402

VP = C.c_void_p


def spread(x):
    return (max(x) - min(x)) / statistics.median(x)


def oracle_cswap(n, cols, size, k, mat, a0, b0):
    from oracle.ref import RefModule
    from poulpy_amd.layouts import VecZnx
    from tests import cswap_oracle as cs
    ref = RefModule(n)
    pr = ref.vmp_pmat_alloc(mat.rows, cols, cols, size)
    ref.vmp_prepare(pr, mat)
    a, b = VecZnx(n, cols, size, np.ascontiguousarray(a0)), VecZnx(n, cols, size, np.ascontiguousarray(b0))
    cs.cswap(ref, a, b, pr, k)
    return a.data, b.data


def bench_gate(n, size, args):
    import torch
    k, batch = args.base2k, args.batch
    mod, a0, b0, mats, keys, p = setup(n, size, k, batch)
    cols = 2
    a, b = a0.clone(), b0.clone()
    ta, tb = torch.zeros_like(a0), torch.zeros_like(a0)
    ma_, mb_ = a0.clone(), b0.clone()   # the same inputs for the materialised route
    torch.cuda.synchronize()            # (torch fills its tensors on its own stream, the module launches on another)
    key = keys[0].ptr

    def swap(x=a, y=b):
        mod.glwe_cswap_batched(VP(x.data_ptr()), VP(y.data_ptr()), key, p, batch, a_size=size, b_size=size)

    def two_cmux():
        mod.glwe_cmux_batched(VP(ta.data_ptr()), VP(b0.data_ptr()), VP(a0.data_ptr()), key, p, batch, t_size=size, f_size=size)
        mod.glwe_cmux_batched(VP(tb.data_ptr()), VP(a0.data_ptr()), VP(b0.data_ptr()), key, p, batch, t_size=size, f_size=size)

    # the first call of each route on fresh inputs: dispatch notes, and the digits that are compared
    mod.dispatch_notes(reset=True)
    swap()
    mod.sync()
    notes = mod.dispatch_notes()
    first_a, first_b = a.clone(), b.clone()
    torch.cuda.synchronize()
    os.environ["POULPY_DBG_CMUX_FUSED"] = "0"
    mod.dispatch_notes(reset=True)
    swap(ma_, mb_)
    mod.sync()
    notes_mat = mod.dispatch_notes()
    os.environ.pop("POULPY_DBG_CMUX_FUSED")
    same = bool(torch.equal(first_a, ma_)) and bool(torch.equal(first_b, mb_))
    ok = None
    if not args.no_parity:
        wa, wb = oracle_cswap(n, cols, size, k, mats[0], a0[0].cpu().numpy(), b0[0].cpu().numpy())
        ok = bool(np.array_equal(first_a[0].cpu().numpy(), wa)) and bool(np.array_equal(first_b[0].cpu().numpy(), wb))

    def materialised():
        os.environ["POULPY_DBG_CMUX_FUSED"] = "0"
        try:
            return timed(mod, lambda: swap(ma_, mb_), args.window) * batch
        finally:
            os.environ.pop("POULPY_DBG_CMUX_FUSED")

    for run in (swap, two_cmux):
        for _ in range(args.warmup):
            run()
    mod.sync()
    ra, rb, ra2, rm = [], [], [], []
    for _ in range(args.rounds):
        ra.append(timed(mod, swap, args.window) * batch)
        rb.append(timed(mod, two_cmux, args.window) * batch)
        ra2.append(timed(mod, swap, args.window) * batch)
        rm.append(materialised())
    ma, mb, ma2, mm = (statistics.median(x) for x in (ra, rb, ra2, rm))
    print(json.dumps({
        "metric": "conditional swaps / s (pz_glwe_cswap_batched vs two pz_glwe_cmux_batched calls into temporaries; rates only, the digits differ)",
        "unit": "swaps/s", "value": ma, "cswap_per_s": ra, "two_cmux_per_s": rb, "cswap_again_per_s": ra2, "materialised_route_per_s": rm,
        "cswap_over_two_cmux": ma / mb, "default_over_materialised": ma / mm, "spread_cswap": spread(ra + ra2), "spread_two_cmux": spread(rb),
        "spread_same_leg": abs(ma - ma2) / ma, "routes_bit_identical": same, "parity_ok": ok,
        "config": {"n": n, "rank": 1, "limbs": size, "base2k": k, "batch": batch, "rounds": args.rounds, "window_s": args.window, "warmup": args.warmup},
        "dispatch_notes": {"default": notes, "POULPY_DBG_CMUX_FUSED=0": notes_mat}}), flush=True)
    if ok is False or not same:
        raise SystemExit(3)   # a fast wrong answer is not a result
    mod.close()


def bench_network(args):
    import torch
    n, size, k, nbits, nslots = 1024, 3, args.base2k, 5, 32
    batch = args.batch
    mod, x0, _, mats, keys, p = setup(n, size, k, nslots * batch, nkeys=nbits)
    ptrs = [d.ptr for d in keys]
    net, one = x0.clone(), x0.clone()
    torch.cuda.synchronize()   # (torch fills its tensors on its own stream, the module launches on another)
    slot_bytes = batch * size * 2 * n * 8

    def composite(buf=net):
        mod.glwe_blind_retrieval_batched(VP(buf.data_ptr()), nslots, ptrs, False, p, batch)

    def singles(buf=one):
        for i in range(nbits):
            t = 1 << (nbits - 1 - i)
            mod.glwe_cswap_batched(VP(buf.data_ptr()), VP(buf.data_ptr() + t * slot_bytes), ptrs[nbits - 1 - i], p, min(t, nslots - t) * batch, a_size=size, b_size=size)

    composite()
    singles()
    mod.sync()
    same = bool(torch.equal(net, one))
    for run in (composite, singles):
        for _ in range(max(args.warmup, 3)):   # (the third identical call is the first HIP-graph replay)
            run()
    mod.sync()
    rc, rs, rc2 = [], [], []
    for _ in range(args.rounds):
        rc.append(timed(mod, composite, args.window) * batch)
        rs.append(timed(mod, singles, args.window) * batch)
        rc2.append(timed(mod, composite, args.window) * batch)
    mc, ms, mc2 = (statistics.median(x) for x in (rc, rs, rc2))
    print(json.dumps({
        "metric": "5-level blind retrievals over 32 slots / s (pz_glwe_blind_retrieval_batched vs 5 pz_glwe_cswap_batched calls)", "unit": "retrievals/s",
        "value": mc, "composite_per_s": rc, "single_calls_per_s": rs, "composite_again_per_s": rc2, "composite_over_singles": mc / ms,
        "spread_composite": spread(rc + rc2), "spread_singles": spread(rs), "spread_same_leg": abs(mc - mc2) / mc, "graph_launches": mod.graph_launches(),
        "routes_bit_identical": same,
        "config": {"n": n, "rank": 1, "limbs": size, "base2k": k, "vectors": batch, "nslots": nslots, "nbits": nbits, "rounds": args.rounds, "window_s": args.window}}),
        flush=True)
    if not same:
        raise SystemExit(3)
    mod.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024:3,2048:3,4096:4", help="N:limbs, comma separated (rank 1)")
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=None, help="pairs per call (default 4096); --network: vectors per call (default 128: 4096 ciphertexts)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--network", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_cswap.py measures one device (--gpus 1)")
    if args.rounds < 5:
        raise SystemExit("bench_cswap.py: at least 5 alternations (--rounds)")
    if args.network:
        args.batch = args.batch or 128
        return bench_network(args)
    args.batch = args.batch or 4096
    for spec in args.shapes.split(","):
        n, size = (int(x) for x in spec.split(":"))
        bench_gate(n, size, args)


if __name__ == "__main__":
    main()
