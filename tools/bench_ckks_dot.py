#!/usr/bin/env python3
"""Secondary measurement: the ciphertext dot product (poulpy-ckks leveled/delegates/composite.rs:563-703 ckks_dot_product_ct, fast branch) on
one MI355X, on device-resident ciphertexts, through pz_glwe_tensor_dot_relinearize_batched (poulpy_amd.ckks.plan_dot_product_ct).

Per pair count:
  leg A   ONE call: every pair tensored into the accumulated tensor of a wave in the module's workspace, one relinearization.  The line
          records the form of the accumulated tensor that ran (16-bit up to npairs 3 2^(base2k-1) <= 2^15 - 1, i64 beyond)
  leg A'  A again: the run-to-run spread the ratios are read against
  leg B   the entry points that exist without it and compute the same digits: npairs x pz_glwe_tensor_apply_batched (apply, then
          add_assign) into a caller-owned i64 tensor batch + pz_glwe_tensor_relinearize_batched.  Bytes compared with A before timing
  leg C   the chain ckks_mul_into + (npairs - 1) x ckks_mul_add_ct (one pz_glwe_tensor_mul_relinearize_acc_batched each): npairs
          relinearizations, other digits by construction - a rate comparison only

All legs in one process, alternated round by round, every timing window at least --window seconds long.  At the largest pair count of the
16-bit form the rounding margin is recorded (pz_module_set_margin_probe; 0.5 would be a wrong limb): of the whole call, and of the
relinearization alone on the accumulated digits (leg B's second call).  The operands are drawn from a pool of four batches per side.

    python tools/bench_ckks_dot.py [--n 65536] [--limbs 16] [--base2k 12] [--batch 256] [--pairs 2,4,5,8,15] [--rounds 3] [--window 0.5]
                                   [--out profiles/ckks_dot_lines.jsonl]
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

NOTE_T16 = "glwe_tensor_dot_relinearize: 16-bit accumulated tensor"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pairs", default="2,4,5,8,15")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from poulpy_amd import ckks
    from poulpy_amd.ckks import Ct
    from poulpy_amd.hal import Module

    n, L, B, K, rank = args.n, args.limbs, args.batch, args.base2k, 1
    cols, tcols = rank + 1, (rank + 1) * (rank + 2) // 2
    hip = Module(n)
    dev = torch.device("cuda")
    h = 1 << (K - 1)
    P = lambda t: C.c_void_p(t.data_ptr())
    rnd = lambda *shape: torch.randint(-h, h, shape, dtype=torch.int64, device=dev)
    pool_a, pool_b = [rnd(B, L, cols, n) for _ in range(4)], [rnd(B, L, cols, n) for _ in range(4)]
    res_a, res_b, res_c = (torch.empty((B, L, cols, n), dtype=torch.int64, device=dev) for _ in range(3))
    tensor = torch.empty((B, L, tcols, n), dtype=torch.int64, device=dev)     # leg B's caller-owned i64 tensor batch
    mat = rnd(n * L * 1 * cols * L)
    pmat = torch.empty(mat.numel(), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip._ck(hip.lib.pz_vmp_prepare(hip.handle, P(pmat), P(mat), C.c_size_t(L), C.c_size_t(1), C.c_size_t(cols), C.c_size_t(L)))
    hip.sync()
    del mat
    tsk = (L, 1, L, K)
    delta = 20
    full = L * K - delta                 # effective_k = max_k

    def timed(fn, steps):
        hip.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        hip.sync()
        return (time.perf_counter() - t0) / steps

    def measure(a, b, c):
        first = [timed(f, 2) for f in (a, b, c)]
        sa, sb, sc = (max(3, math.ceil(args.window / t)) for t in first)
        ta, ta2, tb, tc = [], [], [], []
        for _ in range(args.rounds):
            ta.append(timed(a, sa))
            tb.append(timed(b, sb))
            ta2.append(timed(a, sa))
            tc.append(timed(c, sc))
        return ta, ta2, tb, tc, [sa, sb, sc]

    ms = lambda xs: [round(x * 1e3, 4) for x in xs]
    lines, ok_all = [], True
    counts = [int(x) for x in args.pairs.split(",") if x]

    def legs(npairs):
        """the plans and the three legs of one pair count"""
        a_list = [Ct(K, L, delta, full, cols, P(pool_a[i % 4])) for i in range(npairs)]
        b_list = [Ct(K, L, delta, full, cols, P(pool_b[(i + i // 4) % 4])) for i in range(npairs)]
        dst_meta = Ct(K, L, 0, 0, cols)
        plan = ckks.plan_dot_product_ct(dst_meta, a_list, b_list)
        assert plan.branch in ("fast", "single") and not plan.rescales
        tp, rp = (plan.muls[0] if plan.branch == "single" else plan).params(dst_meta, tsk)
        # leg C: the chain's plans, dst's metadata running from product to product
        run = Ct(K, L, 0, 0, cols)
        chain = [ckks.plan_mul_into(run, a_list[0], b_list[0])]
        chain[0].apply_meta(run)
        for i in range(1, npairs):
            chain.append(ckks.plan_mul_add_ct(run, a_list[i], b_list[i]))
            chain[-1].apply_meta(run)

        def leg_a():
            plan.launch(hip, Ct(K, L, 0, 0, cols, P(res_a)), B, a_list, b_list, P(pmat), tsk)

        def leg_b():
            for i in range(npairs):
                hip.glwe_tensor_apply_batched(P(tensor), a_list[i].data, b_list[i].data, tp, "apply" if i == 0 else "add_assign", B)
            hip.glwe_tensor_relinearize_batched(P(res_b), P(tensor), P(pmat), rp, B)

        def leg_c():
            d = Ct(K, L, 0, 0, cols, P(res_c))
            for i, p in enumerate(chain):
                p.launch(hip, d, B, a_list[i], b_list[i], P(pmat), tsk)
        return tp, rp, leg_a, leg_b, leg_c

    t16_max = 0
    for npairs in counts:
        tp, rp, leg_a, leg_b, leg_c = legs(npairs)
        hip.dispatch_notes(reset=True)
        leg_a()
        hip.sync()
        form = "t16" if NOTE_T16 in hip.dispatch_notes() else "i64"
        leg_b()
        leg_c()
        hip.sync()
        same = bool(torch.equal(res_a, res_b))
        ok_all &= same
        ta, ta2, tb, tc, steps = measure(leg_a, leg_b, leg_c)
        ma, ma2, mb, mc = (statistics.median(x) for x in (ta, ta2, tb, tc))
        spread = abs(1 - ma / ma2)
        ws = hip.glwe_tensor_dot_relinearize_workspace_bytes(tp, rp, npairs, B)
        line = {"op": "dot_product_ct", "npairs": npairs, "form": form, "n": n, "limbs": L, "rank": rank, "base2k": K, "batch": B,
                "a_ms_per_call": round(ma * 1e3, 4), "a2_ms_per_call": round(ma2 * 1e3, 4), "b_ms_per_call": round(mb * 1e3, 4),
                "c_ms_per_call": round(mc * 1e3, 4), "a_ms_per_dot_product": round(ma * 1e3 / B, 5), "dot_products_per_s": round(B / ma, 1),
                "a_over_b": round(ma / mb, 4), "a_over_c": round(ma / mc, 4), "a_over_a2": round(ma / ma2, 4),
                "a_beats_b_beyond_spread": bool(ma / mb < 1 - spread), "a_beats_c_beyond_spread": bool(ma / mc < 1 - spread),
                "same_bytes_a_b": same, "steps": steps, "a_rounds_ms": ms(ta), "a2_rounds_ms": ms(ta2), "b_rounds_ms": ms(tb), "c_rounds_ms": ms(tc),
                "a_workspace_bytes": int(ws), "b_caller_tensor_bytes": int(tensor.numel() * 8)}
        if form == "t16":
            t16_max = max(t16_max, npairs)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if t16_max:
        # the accumulated digits are up to npairs times one product's: the margin of the relinearization that rounds them
        margins = {}
        for npairs in (t16_max, 1):
            tp, rp, leg_a, leg_b, _ = legs(npairs)
            leg_b()                                                   # leaves the accumulated i64 tensor of this pair count in `tensor`
            margins[npairs] = (hip.rounding_margin_of(leg_a),
                               hip.rounding_margin_of(lambda: hip.glwe_tensor_relinearize_batched(P(res_b), P(tensor), P(pmat), rp, B)))
        line = {"op": "dot_product_ct rounding margin", "npairs": t16_max, "form": "t16", "n": n, "limbs": L, "base2k": K, "batch": B,
                "margin_whole_call": margins[t16_max][0], "margin_relinearization_of_accumulated_tensor": margins[t16_max][1],
                "margin_whole_call_one_pair": margins[1][0], "margin_relinearization_of_one_product": margins[1][1]}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
