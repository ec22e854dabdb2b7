#!/usr/bin/env python3
"""Secondary measurement: normalized sums of ciphertexts (poulpy-ckks leveled/delegates/composite.rs: ckks_add_many, and the join of
ckks_dot_product_pt_vec_znx) per second on one MI355X, on device-resident ciphertexts.

  leg A   ONE pz_glwe_sum_batched (poulpy_amd.ckks.SumPlan, route "sum")
  leg A'  A again: the run-to-run spread the A / B ratio is read against
  leg B   the same sum as the chain of pz_glwe_combine_batched calls (route "chain"): the code as it stood before the one-pass call

All legs in one process, alternated round by round, every timing window at least --window seconds long.  A and B are compared byte for
byte before anything is timed.  Cases: n inputs of one budget for every n of --terms (plain joins), and one mixed case (--mixed inputs
whose budgets fall and rise: PZ_JOIN_LSH_ACC and PZ_JOIN_LSH_TERM).  Inputs beyond the fourth reuse the first four buffers 32 ciphertexts
further on each time: in the one-pass call a thread reads all its terms back to back, so no two terms may hand it the same address, and
32 ciphertexts (0.5 GiB of one term's traffic) is further apart than the caches reach.

Second table: ckks_dot_product_pt_vec_znx with shared plaintexts of --pt-limbs limbs and --slots scratch slots by both routes, and the joins
of the same call alone, for the share of the call spent in the join.

    python tools/bench_ckks_sum.py [--n 65536] [--limbs 16] [--rank 1] [--base2k 12] [--batch 256] [--rounds 3] [--window 0.5]
                                   [--terms 2,4,5,8,16,32] [--mixed 8] [--dot 4,16] [--pt-limbs 3] [--slots 4]
                                   [--out profiles/ckks_sum_lines.jsonl]

Bytes are algorithmic for the one-pass form: every input read once, res written once.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY = 6.29e12   # measured float4 copy rate (B/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--rank", type=int, default=1)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--terms", default="2,4,5,8,16,32")
    ap.add_argument("--mixed", type=int, default=8)
    ap.add_argument("--dot", default="4,16")
    ap.add_argument("--pt-limbs", type=int, default=3)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from poulpy_amd import ckks
    from poulpy_amd.ckks import Ct, Pt
    from poulpy_amd.hal import Module

    n, L, B, K, cols = args.n, args.limbs, args.batch, args.base2k, args.rank + 1
    hip = Module(n)
    dev = torch.device("cuda")
    h = 1 << (K - 1)
    P = lambda t: C.c_void_p(t.data_ptr())
    STRIDE = 32                          # ciphertexts between two inputs cut from the same buffer
    nmax = max([int(x) for x in args.terms.split(",") if x] + [args.mixed, 1])
    pool = [torch.randint(-h, h, (B + STRIDE * ((nmax - 1) // 4), L, cols, n), dtype=torch.int64, device=dev) for _ in range(4)]
    inp = lambda i: pool[i % 4][STRIDE * (i // 4):STRIDE * (i // 4) + B]
    res_a, res_b = torch.empty_like(inp(0)), torch.empty_like(inp(0))
    torch.cuda.synchronize()
    delta = 40
    full = L * K - delta                 # effective_k = max_k

    def timed(fn, steps):
        hip.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        hip.sync()
        return (time.perf_counter() - t0) / steps

    def measure(a, b):
        """A, B, A' alternated -> medians and rounds"""
        ta1, tb1 = timed(a, 2), timed(b, 2)
        sa, sb = max(3, math.ceil(args.window / ta1)), max(3, math.ceil(args.window / tb1))
        ta, ta2, tb = [], [], []
        for _ in range(args.rounds):
            ta.append(timed(a, sa))
            tb.append(timed(b, sb))
            ta2.append(timed(a, sa))
        return statistics.median(ta), statistics.median(ta2), statistics.median(tb), [sa, sb], ta, ta2, tb

    def verdict(ma, ma2, mb):
        return {"a_over_b": round(ma / mb, 4), "b_over_a": round(mb / ma, 3), "a_over_a2": round(ma / ma2, 4),
                "a_beats_b_beyond_spread": bool(ma / mb < 1 - abs(1 - ma / ma2))}

    lines, ok_all = [], True
    ct_bytes = L * cols * n * 8
    cases = [("equal", nt) for nt in (int(x) for x in args.terms.split(",") if x)]
    if args.mixed >= 3:
        cases.append(("mixed", args.mixed))
    for kind, nt in cases:
        # mixed: budgets that fall and rise - PZ_JOIN_LSH_ACC (once by more than a limb) and PZ_JOIN_LSH_TERM
        budgets = [full] * nt if kind == "equal" else [full - (7 * ((i * 5) % 4)) - (K if i == 2 else 0) for i in range(nt)]
        ins = [Ct(K, L, delta, budgets[i], cols, P(inp(i))) for i in range(nt)]
        plan = ckks.plan_add_many(Ct(K, L, 0, 0, cols), ins)

        def leg(out, route):
            def run():
                plan.launch(hip, Ct(K, L, 0, 0, cols, P(out)), B, ins, route=route)
            return run
        a, b = leg(res_a, "sum"), leg(res_b, "chain")
        a()
        b()
        hip.sync()
        same = bool(torch.equal(res_a, res_b))
        ok_all &= same
        ma, ma2, mb, steps, ta, ta2, tb = measure(a, b)
        nbytes = B * ct_bytes * (nt + 1)
        chain_calls = len(ckks.chain_calls(plan.terms))
        line = {"op": "add_many", "budgets": kind, "nterms": nt, "joins": [t.join for t in plan.terms], "n": n, "limbs": L, "rank": args.rank,
                "base2k": K, "batch": B, "a_ms_per_call": round(ma * 1e3, 4), "a2_ms_per_call": round(ma2 * 1e3, 4),
                "b_ms_per_call": round(mb * 1e3, 4), "b_launches": chain_calls, "b_passes": nt + 2 * chain_calls - 1,
                "sums_per_s": round(B / ma, 1), "alg_bytes": nbytes, "alg_tbps": round(nbytes / ma / 1e12, 3),
                "frac_copy_6_3tbs": round(nbytes / ma / COPY, 3), **verdict(ma, ma2, mb), "same_bytes_a_b": same, "steps": steps,
                "a_rounds_ms": [round(x * 1e3, 4) for x in ta], "a2_rounds_ms": [round(x * 1e3, 4) for x in ta2],
                "b_rounds_ms": [round(x * 1e3, 4) for x in tb]}
        print(json.dumps(line), flush=True)
        lines.append(line)

    # ---- the dot product by shared plaintext vectors: the whole call and its joins alone, by both routes ----
    S, PL = args.slots, args.pt_limbs
    dots = [int(x) for x in args.dot.split(",") if x]
    if dots:
        tmp = torch.empty((S,) + tuple(res_a.shape), dtype=torch.int64, device=dev)
        pts_dev = [torch.randint(-h, h, (1, PL, 1, n), dtype=torch.int64, device=dev) for _ in range(4)]
        torch.cuda.synchronize()
    for nt in dots:
        ops = [Ct(K, L, delta, full, cols, P(inp(i % 4))) for i in range(nt)]
        pts = [Pt(K, PL, PL * K - 4, P(pts_dev[i % len(pts_dev)]), log_budget=4) for i in range(nt)]
        plan = ckks.plan_dot_product_pt_vec_znx(Ct(K, L, 0, 0, cols), ops, pts)

        def leg(out, route):
            def run():
                plan.launch(hip, Ct(K, L, 0, 0, cols, P(out)), B, ops, pts, tmp=P(tmp), slots=S, pt_shared=range(nt), route=route)
            return run

        def joins(out, route):
            """the joins of the same call on whatever the slots hold"""
            dst = Ct(K, L, 0, 0, cols, P(out))
            slot_bytes = B * ct_bytes

            def run():
                for lo in range(0, nt, S):
                    chunk = plan.terms[lo:lo + S]
                    at = {id(t): tmp.data_ptr() + s * slot_bytes for s, t in enumerate(chunk)}
                    ckks._launch_joins(hip, dst, B, chunk, lambda t: (at[id(t)], L, False), route, continues=lo > 0)
            return run
        a, b = leg(res_a, "sum"), leg(res_b, "chain")
        a()
        b()
        hip.sync()
        same = bool(torch.equal(res_a, res_b))
        ok_all &= same
        ma, ma2, mb, steps, ta, ta2, tb = measure(a, b)
        ja, ja2, jb, _, _, _, _ = measure(joins(res_a, "sum"), joins(res_b, "chain"))
        line = {"op": "dot_product_pt_vec_znx", "nterms": nt, "slots": S, "pt_limbs": PL, "pt_shared": True, "n": n, "limbs": L, "rank": args.rank,
                "base2k": K, "batch": B, "a_ms_per_call": round(ma * 1e3, 4), "a2_ms_per_call": round(ma2 * 1e3, 4),
                "b_ms_per_call": round(mb * 1e3, 4), "a_join_ms": round(ja * 1e3, 4), "a2_join_ms": round(ja2 * 1e3, 4), "b_join_ms": round(jb * 1e3, 4),
                "a_join_share": round(ja / ma, 3), "b_join_share": round(jb / mb, 3), "dots_per_s": round(B / ma, 1), **verdict(ma, ma2, mb),
                "same_bytes_a_b": same, "steps": steps, "a_rounds_ms": [round(x * 1e3, 4) for x in ta],
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
