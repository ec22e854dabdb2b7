#!/usr/bin/env python3
"""Secondary measurement: CMUX gates per second on one MI355X (pz_glwe_cmux_batched), an A/B in one process on one device.

    A  pz_glwe_cmux_batched(res, t, f)                                  the gate: the difference, the product, + f, the carry chain
    B  pz_vec_znx_sub_batched(d, t, f) per column, then pz_glwe_external_product_batched(res, d)   on the same buffers
    A' A again                                                           the run-to-run spread of the identical leg

B is NOT a CMUX: it never adds f, so it does strictly less work - it is what a caller had before this entry point, minus the addition.
The legs alternate (A B A' B ...) `--rounds` times, every leg warmed, every window at least `--window` seconds of device work ending in a
synchronise.  Reported per shape: the median rate of each leg, A / B, and the spread |A - A'| / A.  The gate's output is compared bit for bit with
the oracle on ciphertext 0 and with the materialised route (POULPY_DBG_CMUX_FUSED=0, set between calls in this process), which is timed in the
same rounds; at N = 4096 so is the three-kernel pipeline on the materialised difference (small path off), the other candidate for the default.

    python tools/bench_cmux.py [--shapes 1024:3,2048:3,4096:4] [--batch 4096] [--rounds 5] [--window 0.5] [--gpus 1]
    python tools/bench_cmux.py --ladder [--batch 1024]      the 10-step blind-rotation ladder at N = 1024 against 10 single calls

Prints one JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
VP = C.c_void_p


def timed(mod, run, window):
    """calls of `run` per second over a window of at least `window` seconds (sized from a first timed call), ending in a synchronise"""
    mod.sync()
    t0 = time.perf_counter()
    run()
    mod.sync()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, int(window / one) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    mod.sync()
    return reps / (time.perf_counter() - t0)


def setup(n, size, k, batch, rank=1, nkeys=1):
    import torch
    from poulpy_amd.hal import GlweOpParams, Module
    from poulpy_amd.layouts import MatZnx
    cols = rank + 1
    dev = torch.device("cuda:0")
    mod = Module(n, device=0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x636d7578)
    half = 1 << (k - 1)
    t = torch.randint(-half, half, (batch, size, cols, n), dtype=torch.int64, device=dev, generator=g)
    f = torch.randint(-half, half, (batch, size, cols, n), dtype=torch.int64, device=dev, generator=g)
    rng = np.random.default_rng(23)
    mats, keys = [], []
    for _ in range(nkeys):
        mat = MatZnx(n, size, cols, cols, size).fill_uniform(k, rng)
        pm = mod.vmp_pmat_alloc(size, cols, cols, size)
        mod.vmp_prepare(pm, mat)
        d = mod.device_alloc(pm.data.nbytes).upload(pm.data)
        mod.pin_key(d.ptr, size, cols, cols, size)
        mats.append(mat)
        keys.append(d)
    p = GlweOpParams(rank=rank, dnum=size, dsize=1, key_size=size, key_base2k=k, a_size=size, a_base2k=k, res_size=size, res_base2k=k, rank_out=rank)
    return mod, t, f, mats, keys, p


def oracle_cmux(n, cols, size, k, mat, t0, f0, rot=None):
    from oracle.ref import RefModule
    from poulpy_amd.layouts import VecZnx
    from tests import cmux_oracle as co
    ref = RefModule(n)
    pr = ref.vmp_pmat_alloc(mat.rows, cols, cols, size)
    ref.vmp_prepare(pr, mat)
    res = VecZnx(n, cols, size)
    f = VecZnx(n, cols, size, np.ascontiguousarray(f0))
    if rot is None:
        co.cmux(ref, res, VecZnx(n, cols, size, np.ascontiguousarray(t0)), f, pr, k)
    else:
        co.cmux_rotated(ref, res, f, rot, pr, k)
    return res.data


def bench_gate(n, size, args):
    import torch
    k, batch = args.base2k, args.batch
    mod, t, f, mats, keys, p = setup(n, size, k, batch)
    cols = 2
    res = torch.zeros_like(t)
    res_b = torch.zeros_like(t)
    d = torch.zeros_like(t)
    key = keys[0].ptr

    def gate(out=res):
        mod.glwe_cmux_batched(VP(out.data_ptr()), VP(t.data_ptr()), VP(f.data_ptr()), key, p, batch, t_size=size, f_size=size)

    def two_calls():
        for c in range(cols):
            mod.lib.pz_vec_znx_sub_batched(mod.handle, batch, VP(d.data_ptr()), cols, size, c, VP(t.data_ptr()), cols, size, c, VP(f.data_ptr()), cols, size, c)
        mod.glwe_external_product_batched(VP(res_b.data_ptr()), VP(d.data_ptr()), key, p, batch)

    for run in (gate, two_calls):
        for _ in range(args.warmup):
            run()
    mod.sync()
    mod.dispatch_notes(reset=True)
    gate()
    mod.sync()
    notes = mod.dispatch_notes()

    def switched(enter, leave, out):
        """one window of the gate under a switch, the switch's dispatch notes and output kept"""
        enter()
        mod.dispatch_notes(reset=True)
        gate(out)
        mod.sync()
        got = mod.dispatch_notes()
        rate = timed(mod, lambda: gate(out), args.window) * batch
        leave()
        return rate, got

    # the materialised route (POULPY_DBG_CMUX_FUSED=0, read per call) and, at N = 4096, the three-kernel pipeline (small path off) on the same inputs
    mat_out, pipe_out = torch.zeros_like(t), torch.zeros_like(t)
    pipeline = n == 4096
    a, b, a2, m, pl = [], [], [], [], []
    notes_mat = notes_pipe = None
    for _ in range(args.rounds):
        a.append(timed(mod, gate, args.window) * batch)
        b.append(timed(mod, two_calls, args.window) * batch)
        a2.append(timed(mod, gate, args.window) * batch)
        rate, notes_mat = switched(lambda: os.environ.__setitem__("POULPY_DBG_CMUX_FUSED", "0"), lambda: os.environ.pop("POULPY_DBG_CMUX_FUSED"), mat_out)
        m.append(rate)
        if pipeline:
            rate, notes_pipe = switched(lambda: mod.set_small_path(False), lambda: mod.set_small_path(True), pipe_out)
            pl.append(rate)
    gate()
    mod.sync()
    same = bool(torch.equal(res, mat_out)) and (not pipeline or bool(torch.equal(res, pipe_out)))
    ok = None
    if not args.no_parity:
        ok = bool(np.array_equal(res[0].cpu().numpy(), oracle_cmux(n, cols, size, k, mats[0], t[0].cpu().numpy(), f[0].cpu().numpy())))
    ma, mb, ma2, mm = (statistics.median(x) for x in (a, b, a2, m))
    mp = statistics.median(pl) if pl else None
    print(json.dumps({
        "metric": "CMUX gates / s (pz_glwe_cmux_batched vs vec_znx_sub + external product, which omits the add of f)", "unit": "gates/s",
        "value": ma, "cmux_per_s": a, "two_call_per_s": b, "cmux_again_per_s": a2, "materialised_route_per_s": m, "pipeline_route_per_s": pl or None,
        "cmux_over_two_call": ma / mb, "default_over_materialised": ma / mm, "default_over_pipeline": ma / mp if mp else None, "spread_same_leg": abs(ma - ma2) / ma,
        "routes_bit_identical": same, "parity_ok": ok,
        "config": {"n": n, "rank": 1, "limbs": size, "base2k": k, "batch": batch, "rounds": args.rounds, "window_s": args.window, "warmup": args.warmup},
        "dispatch_notes": {"default": notes, "POULPY_DBG_CMUX_FUSED=0": notes_mat, "small path off": notes_pipe}}), flush=True)
    if ok is False or not same:
        raise SystemExit(3)   # a fast wrong answer is not a result
    mod.close()


def bench_ladder(args):
    import torch
    n, size, k, batch, nbits = 1024, 3, args.base2k, args.batch, 10
    mod, a, _, mats, keys, p = setup(n, size, k, batch, nkeys=nbits)
    res, tmp, ping, pong = (torch.zeros_like(a) for _ in range(4))
    ptrs = [d.ptr for d in keys]

    def ladder():
        mod.glwe_blind_rotation_batched(VP(res.data_ptr()), VP(a.data_ptr()), ptrs, True, 0, p, VP(tmp.data_ptr()), tmp.numel() * 8, batch)

    def singles():
        bufs = [a, ping, pong]
        src, dst = 0, 1
        for i in range(nbits):
            mod.glwe_cmux_batched(VP(bufs[dst].data_ptr()), None, VP(bufs[src].data_ptr()), ptrs[i], p, batch, t_size=size, f_size=size, t_rot=1 << i)
            src, dst = dst, (2 if dst == 1 else 1)

    for run in (ladder, singles):
        for _ in range(max(args.warmup, 3)):   # (the third identical call is the first HIP-graph replay)
            run()
    mod.sync()
    la, si, la2 = [], [], []
    for _ in range(args.rounds):
        la.append(timed(mod, ladder, args.window) * batch)
        si.append(timed(mod, singles, args.window) * batch)
        la2.append(timed(mod, ladder, args.window) * batch)
    singles()
    mod.sync()
    same = bool(torch.equal(res, ping if nbits % 2 else pong))
    ml, ms, ml2 = (statistics.median(x) for x in (la, si, la2))
    print(json.dumps({
        "metric": "10-step blind rotations by encrypted bits / s (pz_glwe_blind_rotation_batched vs 10 pz_glwe_cmux_batched calls)", "unit": "rotations/s",
        "value": ml, "ladder_per_s": la, "single_calls_per_s": si, "ladder_again_per_s": la2, "ladder_over_singles": ml / ms,
        "spread_same_leg": abs(ml - ml2) / ml, "graph_launches": mod.graph_launches(), "routes_bit_identical": same,
        "config": {"n": n, "rank": 1, "limbs": size, "base2k": k, "batch": batch, "nbits": nbits, "rounds": args.rounds, "window_s": args.window}}), flush=True)
    if not same:
        raise SystemExit(3)
    mod.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024:3,2048:3,4096:4", help="N:limbs, comma separated (rank 1)")
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--ladder", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_cmux.py measures one device (--gpus 1)")
    if args.ladder:
        return bench_ladder(args)
    for spec in args.shapes.split(","):
        n, size = (int(x) for x in spec.split(":"))
        bench_gate(n, size, args)


if __name__ == "__main__":
    main()
