#!/usr/bin/env python3
"""Secondary measurement: weighted sums of ciphertexts by constants (poulpy-ckks leveled/delegates/composite.rs: ckks_mul_add_pt_const_*,
ckks_dot_product_pt_const_znx) per second on one MI355X, on device-resident ciphertexts.

  leg A   ONE pz_glwe_lincomb_const_batched (poulpy_amd.ckks.LincombPlan, route "fused")
  leg A'  A again: the run-to-run spread the A / B ratio is read against
  leg B   the same sum term by term: pz_glwe_mul_const_batched into a scratch batch + pz_glwe_combine_batched (route "composed"), the best
          route without the one-pass call

All legs in one process, alternated round by round, every timing window at least --window seconds long.  A and B are compared byte for
byte before anything is timed.  Cases: nterms 1 (mul_add), 2, 8, 32 (dot products), each with real and with complex constants, equal
budgets.  Operands beyond the fourth reuse the first four batches (each batch is far larger than the caches).

    python tools/bench_ckks_lincomb.py [--n 65536] [--limbs 16] [--rank 1] [--base2k 12] [--batch 256] [--digits 3] [--rounds 3]
                                       [--window 0.5] [--terms 1,2,8,32] [--out profiles/ckks_lincomb_lines.jsonl]

Bytes are algorithmic for the one-pass form: every operand read once, res written once, plus res read where the sum starts from it.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY = 6.29e12   # measured float4 copy rate (B/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--rank", type=int, default=1)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--digits", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--terms", default="1,2,8,32")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from poulpy_amd import ckks
    from poulpy_amd.ckks import Cst, Ct
    from poulpy_amd.hal import Module

    n, L, B, K, cols = args.n, args.limbs, args.batch, args.base2k, args.rank + 1
    hip = Module(n)
    dev = torch.device("cuda")
    h = 1 << (K - 1)
    rng = np.random.default_rng(7)
    P = lambda t: C.c_void_p(t.data_ptr())
    nmax = max(int(x) for x in args.terms.split(","))
    pool = [torch.randint(-h, h, (B, L, cols, n), dtype=torch.int64, device=dev) for _ in range(min(nmax, 4))]
    res0 = torch.randint(-h, h, (B, L, cols, n), dtype=torch.int64, device=dev)
    res_a, res_b, tmp = torch.empty_like(res0), torch.empty_like(res0), torch.empty_like(res0)
    torch.cuda.synchronize()
    budget = L * K - 40 - 2 * K          # the operands: log_delta 40, two limbs of headroom used
    cmeta = (K, args.digits * K - K)     # the constants: min_k = digits * base2k

    def timed(fn, steps):
        hip.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        hip.sync()
        return (time.perf_counter() - t0) / steps

    lines, ok_all = [], True
    for nt in [int(x) for x in args.terms.split(",")]:
        for cplx in (False, True):
            csts = [Cst(cmeta[0], cmeta[1], rng.integers(-h, h, args.digits, dtype=np.int64),
                        rng.integers(-h, h, args.digits, dtype=np.int64) if cplx else None) for _ in range(nt)]
            ops = [Ct(K, L, 40, budget, cols, P(pool[i % len(pool)])) for i in range(nt)]
            if nt == 1:
                probe = ckks.plan_mul_pt_const_into(Ct(K, L, 0, 0, cols), ops[0], csts[0])
                dmeta = (40, probe.log_budget)                     # dst at the product's budget: a plain join
                plan = ckks.plan_mul_add_pt_const(Ct(K, L, *dmeta, cols), ops[0], csts[0])
            else:
                dmeta = (0, 0)
                plan = ckks.plan_dot_product_pt_const(Ct(K, L, 0, 0, cols), ops, csts)

            def leg(out, route):
                def run():
                    plan.launch(hip, Ct(K, L, dmeta[0], dmeta[1], cols, P(out)), B, ops, csts, tmp=P(tmp), route=route)
                return run
            a, b = leg(res_a, "fused"), leg(res_b, "composed")
            # mul_add accumulates into res: both legs start from the same content for the comparison; while timing they keep accumulating
            # (normalized digits in, normalized digits out: the work per call is the same)
            res_a.copy_(res0)
            res_b.copy_(res0)
            a()
            b()
            hip.sync()
            same = bool(torch.equal(res_a, res_b))
            ok_all &= same
            ta1, tb1 = timed(a, 2), timed(b, 2)
            sa, sb = max(3, math.ceil(args.window / ta1)), max(3, math.ceil(args.window / tb1))
            ta, ta2, tb = [], [], []
            for _ in range(args.rounds):
                ta.append(timed(a, sa))
                tb.append(timed(b, sb))
                ta2.append(timed(a, sa))
            ma, ma2, mb = statistics.median(ta), statistics.median(ta2), statistics.median(tb)
            ct_bytes = L * cols * n * 8
            nbytes = B * ct_bytes * (nt + 1 + (1 if plan.init_res else 0))
            line = {"op": plan.name, "nterms": nt, "complex": cplx, "n": n, "limbs": L, "rank": args.rank, "base2k": K, "batch": B, "digits": args.digits,
                    "a_ms_per_call": round(ma * 1e3, 4), "a2_ms_per_call": round(ma2 * 1e3, 4), "b_ms_per_call": round(mb * 1e3, 4),
                    "sums_per_s": round(B / ma, 1), "alg_bytes": nbytes, "alg_tbps": round(nbytes / ma / 1e12, 3),
                    "frac_copy_6_3tbs": round(nbytes / ma / COPY, 3), "a_over_b": round(ma / mb, 4), "b_over_a": round(mb / ma, 3),
                    "a_over_a2": round(ma / ma2, 4), "a_beats_b_beyond_spread": bool(ma / mb < 1 - abs(1 - ma / ma2)),
                    "same_bytes_a_b": same, "steps": [sa, sb], "a_rounds_ms": [round(x * 1e3, 4) for x in ta],
                    "a2_rounds_ms": [round(x * 1e3, 4) for x in ta2], "b_rounds_ms": [round(x * 1e3, 4) for x in tb]}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
