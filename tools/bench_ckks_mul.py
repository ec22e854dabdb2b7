#!/usr/bin/env python3
"""Secondary measurement: products of two ciphertexts (poulpy-ckks leveled/default/mul.rs, leveled/delegates/composite.rs: ckks_mul_add_ct_into,
ckks_mul_many) on one MI355X, on device-resident ciphertexts, through pz_glwe_tensor_mul_relinearize_acc_batched (poulpy_amd.ckks plans).

  (a) mul_add_ct   leg A   ONE call: the product of a wave kept in the module's workspace and joined to dst there
                   leg A'  A again: the run-to-run spread the A / B ratio is read against
                   leg B   the entry points that exist without it: pz_glwe_tensor_mul_relinearize_batched into a caller-owned scratch
                           batch, then ONE pz_glwe_combine_batched that joins and normalizes
  (b) strided      leg A   the product of two rescaled operands (containers of --limbs limbs, --used of them in use) read in place
                   leg B   pz_vec_znx_copy_batched per column and operand into compacted batches, then the existing call
  (c) mul_many     4 and 8 inputs: ms per call and products per second (no second leg: nothing else computes it)

All legs in one process, alternated round by round, every timing window at least --window seconds long.  A and B are compared byte for
byte before anything is timed.

    python tools/bench_ckks_mul.py [--n 65536] [--limbs 16] [--used 14] [--base2k 12] [--batch 256] [--rounds 3] [--window 0.5]
                                   [--many 4,8] [--out profiles/ckks_mul_lines.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--used", type=int, default=14)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--many", default="4,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from poulpy_amd import ckks
    from poulpy_amd.ckks import LSH, RAW, Ct
    from poulpy_amd.hal import Module

    n, L, U, B, K, rank = args.n, args.limbs, args.used, args.batch, args.base2k, 1
    cols = rank + 1
    hip = Module(n)
    dev = torch.device("cuda")
    h = 1 << (K - 1)
    P = lambda t: C.c_void_p(t.data_ptr())
    rnd = lambda *shape: torch.randint(-h, h, shape, dtype=torch.int64, device=dev)
    a_t, b_t, d0 = rnd(B, L, cols, n), rnd(B, L, cols, n), rnd(B, L, cols, n)
    res_a, res_b, tmp = torch.empty_like(d0), torch.empty_like(d0), torch.empty_like(d0)
    # the tensor key: synthetic digits prepared on the device, dnum = the tensor's limbs
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

    def measure(a, b):
        ta1, tb1 = timed(a, 2), timed(b, 2)
        sa, sb = max(3, math.ceil(args.window / ta1)), max(3, math.ceil(args.window / tb1))
        ta, ta2, tb = [], [], []
        for _ in range(args.rounds):
            ta.append(timed(a, sa))
            tb.append(timed(b, sb))
            ta2.append(timed(a, sa))
        return statistics.median(ta), statistics.median(ta2), statistics.median(tb), [sa, sb], ta, ta2, tb

    def verdict(ma, ma2, mb):
        return {"a_over_b": round(ma / mb, 4), "a_over_a2": round(ma / ma2, 4), "a_beats_b_beyond_spread": bool(ma / mb < 1 - abs(1 - ma / ma2))}

    def common(ma, ma2, mb, steps, ta, ta2, tb, same):
        return {"n": n, "limbs": L, "rank": rank, "base2k": K, "batch": B, "a_ms_per_call": round(ma * 1e3, 4), "a2_ms_per_call": round(ma2 * 1e3, 4),
                "b_ms_per_call": round(mb * 1e3, 4), "products_per_s": round(B / ma, 1), **verdict(ma, ma2, mb), "same_bytes_a_b": same, "steps": steps,
                "a_rounds_ms": [round(x * 1e3, 4) for x in ta], "a2_rounds_ms": [round(x * 1e3, 4) for x in ta2],
                "b_rounds_ms": [round(x * 1e3, 4) for x in tb], "dispatch": hip.dispatch_notes()}

    lines, ok_all = [], True
    ct_bytes = L * cols * n * 8

    # ---- (a) mul_add_ct: one call against product-into-scratch + combine ----
    a_ct, b_ct = Ct(K, L, delta, full, cols, P(a_t)), Ct(K, L, delta, full, cols, P(b_t))
    dst_meta = Ct(K, L, delta, full - delta - 5, cols)              # 5 bits below the product's budget: the product is shifted into the join
    plan = ckks.plan_mul_add_ct(dst_meta, a_ct, b_ct)
    tp, rp = plan.params(dst_meta, tsk)
    join_terms = [dict(a=None, a_size=L, kind=LSH if plan.join == ckks.LSH_ACC else RAW, k=plan.k if plan.join == ckks.LSH_ACC else 0),
                  dict(a=P(tmp), a_size=L, kind=LSH if plan.join == ckks.LSH_TERM else RAW, k=plan.k if plan.join == ckks.LSH_TERM else 0, sign=plan.sign)]

    def leg_a():
        plan.launch(hip, Ct(K, L, dst_meta.log_delta, dst_meta.log_budget, cols, P(res_a)), B, a_ct, b_ct, P(pmat), tsk)

    def leg_b():
        hip.glwe_tensor_mul_relinearize_batched(P(tmp), P(a_t), P(b_t), P(pmat), tp, rp, "apply", B)
        join_terms[0]["a"] = P(res_b)
        hip.glwe_combine_batched(P(res_b), cols, L, K, join_terms, True, B)

    res_a.copy_(d0)
    res_b.copy_(d0)
    hip.dispatch_notes(reset=True)
    leg_a()
    leg_b()
    hip.sync()
    same = bool(torch.equal(res_a, res_b))
    ok_all &= same
    m = measure(leg_a, leg_b)
    ws = hip.glwe_tensor_mul_relinearize_acc_workspace_bytes(tp, rp, True, "apply", B)
    line = {"op": "mul_add_ct", "join": plan.join, "k": plan.k, **common(*m, same), "a_scratch_bytes": 0, "b_scratch_bytes": B * ct_bytes,
            "a_workspace_bytes": int(ws), "module_workspace_bytes": int(hip.lib.pz_module_workspace_bytes(hip.handle))}
    print(json.dumps(line), flush=True)
    lines.append(line)

    # ---- (b) a product of rescaled operands: strides against copy-compaction ----
    used_k = U * K                      # after a rescale: the top U limbs in use
    ra, rb = Ct(K, L, delta, used_k - delta, cols, P(a_t)), Ct(K, L, delta, used_k - delta, cols, P(b_t))
    out_meta = Ct(K, L, 0, 0, cols)
    sp = ckks.plan_mul_into(out_meta, ra, rb)
    assert (sp.a_size, sp.a_stride) == (U, L)
    ac, bc = torch.empty((B, U, cols, n), dtype=torch.int64, device=dev), torch.empty((B, U, cols, n), dtype=torch.int64, device=dev)
    ctp, crp = sp.params(out_meta, tsk)     # the same tensor layout in both legs: only the operands' stride differs
    cpa = ckks.plan_compact_limbs_copy(Ct(K, U, 0, 0, cols), ra)

    def leg_sa():
        sp.launch(hip, Ct(K, L, 0, 0, cols, P(res_a)), B, ra, rb, P(pmat), tsk)

    def leg_sb():
        cpa.launch(hip, Ct(K, U, 0, 0, cols, P(ac)), B, ra)
        cpa.launch(hip, Ct(K, U, 0, 0, cols, P(bc)), B, rb)
        hip.glwe_tensor_mul_relinearize_batched(P(res_b), P(ac), P(bc), P(pmat), ctp, crp, "apply", B)

    hip.dispatch_notes(reset=True)
    leg_sa()
    leg_sb()
    hip.sync()
    same = bool(torch.equal(res_a, res_b))
    ok_all &= same
    m = measure(leg_sa, leg_sb)
    line = {"op": "mul_into, rescaled operands", "used_limbs": U, **common(*m, same), "b_copy_bytes": 2 * B * U * cols * n * 8}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del ac, bc

    # ---- (c) mul_many ----
    for nt in [int(x) for x in args.many.split(",") if x]:
        srcs = [a_t, b_t, d0, tmp]
        ins = [Ct(K, L, delta, full, cols, P(srcs[i % 4])) for i in range(nt)]
        mp = ckks.plan_mul_many(Ct(K, L, 0, 0, cols), ins)
        nbytes = mp.scratch_bytes(B, n)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)

        def leg_m():
            mp.launch(hip, Ct(K, L, 0, 0, cols, P(res_a)), B, ins, P(pmat), tsk, tmp=P(scratch))
        hip.dispatch_notes(reset=True)
        leg_m()
        hip.sync()
        t1 = timed(leg_m, 2)
        steps = max(3, math.ceil(args.window / t1))
        ts = [timed(leg_m, steps) for _ in range(args.rounds)]
        med = statistics.median(ts)
        muls = sum(nd.op == "mul" for nd in mp.nodes)
        line = {"op": "mul_many", "inputs": nt, "nodes": [nd.op for nd in mp.nodes], "slot_limbs": mp.slot_limbs, "scratch_bytes": nbytes, "n": n,
                "limbs": L, "rank": rank, "base2k": K, "batch": B, "ms_per_call": round(med * 1e3, 4), "ms_per_multiplication": round(med * 1e3 / muls, 4),
                "multiplications_per_s": round(B * muls / med, 1), "rounds_ms": [round(x * 1e3, 4) for x in ts], "steps": steps,
                "dispatch": hip.dispatch_notes()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del scratch
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
