#!/usr/bin/env python3
"""Secondary measurement: the CKKS linear operations (poulpy-ckks src/leveled/default/{add,sub,neg,rescale,pt_znx}.rs) per second on one
MI355X, each as ONE pz_glwe_combine_batched call (poulpy_amd/ckks.py) on device-resident ciphertexts.  Where the operation can be built from
the older batched entry points, that composition is timed in the same process, interleaved, and the ratio reported:
  add / sub (equal budgets): per column pz_vec_znx_add_into_batched (sub_batched) + pz_vec_znx_normalize_batched
  rescale:                   per column pz_vec_znx_lsh_batched
A few timed outputs are compared bit for bit with the oracle composition of tests/shift_oracle.py.

    python tools/bench_ckks_linear.py --op add|add_unequal|sub|neg|rescale|add_pt [--n 65536] [--limbs 16] [--rank 1] [--base2k 12]
                                      [--batch 256] [--steps 20] [--warmup 3] [--rounds 5]

Shapes: configs[4] of tools/bench_tensor.py (N = 2^16, 16 limbs, rank 1, base2k 12, 256 ciphertexts).  Bytes are algorithmic: every
operand read once (a shared plaintext once per call), res written once, plus res read when it is an operand.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PEAK, COPY = 8.0e12, 6.29e12   # HBM3E spec and measured float4 copy rate (B/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=("add", "add_unequal", "sub", "neg", "rescale", "add_pt"), default="add")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--rank", type=int, default=1)
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from oracle.ref import RefModule
    from poulpy_amd import ckks
    from poulpy_amd.ckks import Ct, Pt
    from poulpy_amd.hal import Module
    from poulpy_amd.layouts import VecZnx
    from tests import shift_oracle as so

    n, L, B, K, cols = args.n, args.limbs, args.batch, args.base2k, args.rank + 1
    hip = Module(n)
    dev = torch.device("cuda")
    h = 1 << (K - 1)

    def ct_batch(size, c=cols, m=B):
        return torch.randint(-h, h, (m, size, c, n), dtype=torch.int64, device=dev)

    dst = Ct(K, L, 0, 0, cols)
    ops, shared = {}, ()
    if args.op in ("add", "sub"):
        ops = {"a": Ct(K, L, 40, L * K - 40, cols), "b": Ct(K, L, 40, L * K - 40, cols)}
        plan = ckks.plan_add_into(dst, ops["a"], ops["b"], sub=args.op == "sub")
    elif args.op == "add_unequal":
        ops = {"a": Ct(K, L, 40, L * K - 40, cols), "b": Ct(K, L, 40, L * K - 40 - 2 * K - 5, cols)}
        plan = ckks.plan_add_into(dst, ops["a"], ops["b"])
    elif args.op == "neg":
        ops = {"a": Ct(K, L, 40, L * K - 40, cols)}
        plan = ckks.plan_neg_into(dst, ops["a"])
    elif args.op == "rescale":
        ops = {"a": Ct(K, L, 40, L * K - 40, cols)}
        plan = ckks.plan_rescale_into(dst, ops["a"], 40)
    else:
        ops = {"a": Ct(K, L, 40, L * K - 40, cols), "pt": Pt(K, 3, 40)}
        shared = ("pt",)
        plan = ckks.plan_add_pt_into(dst, ops["a"], ops["pt"])
    bufs = {k: ct_batch(o.size, 1 if isinstance(o, Pt) else cols, 1 if k in shared else B) for k, o in ops.items()}
    res = torch.zeros((B, L, cols, n), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())
    dargs = {k: (Pt if isinstance(o, Pt) else Ct)(**{**o.__dict__, "data": P(bufs[k])}) for k, o in ops.items()}

    def fused():
        d = Ct(**{**dst.__dict__, "data": P(res)})
        plan.launch(hip, d, B, dargs.get("a"), dargs.get("b"), dargs.get("pt"), shared=shared)

    comp, tmp = None, None
    L_ = hip.lib
    sz = lambda *xs: [C.c_size_t(int(x)) for x in xs]
    if args.op in ("add", "sub") and plan.terms[0].kind == ckks.RAW:
        tmp = torch.empty_like(res)
        f = L_.pz_vec_znx_sub_batched if args.op == "sub" else L_.pz_vec_znx_add_into_batched

        def comp():
            for c in range(cols):
                hip._ck(f(hip.handle, C.c_size_t(B), P(tmp), *sz(cols, L, c), P(bufs["a"]), *sz(cols, L, c), P(bufs["b"]), *sz(cols, L, c)))
                hip._ck(L_.pz_vec_znx_normalize_batched(hip.handle, C.c_size_t(B), P(res), *sz(cols, L, K), C.c_int64(0), C.c_size_t(c), P(tmp),
                                                        *sz(cols, L, K, c)))
    elif args.op == "rescale":
        def comp():
            for c in range(cols):
                hip._ck(L_.pz_vec_znx_lsh_batched(hip.handle, C.c_size_t(B), *sz(K, 40), P(res), *sz(cols, L, c), P(bufs["a"]), *sz(cols, L, c)))

    def timed(fn, steps):
        hip.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        hip.sync()
        return (time.perf_counter() - t0) / steps

    def parity(out):
        ref = RefModule(n)
        ok = True
        for t in sorted({0, B - 1}):
            host = {k: bufs[k][0 if k in shared else t].cpu().numpy().copy() for k in ops}
            kw = {}
            for k, o in ops.items():
                v = VecZnx(n, host[k].shape[1], o.size, host[k])
                kw[k] = Pt(o.base2k, o.size, o.log_delta, v) if isinstance(o, Pt) else Ct(o.base2k, o.size, o.log_delta, o.log_budget, cols, v)
            d = Ct(K, L, 0, 0, cols, VecZnx(n, cols, L))
            so.run(ref, plan, d, kw.get("a"), kw.get("b"), kw.get("pt"))
            ok &= bool(np.array_equal(out[t].cpu().numpy(), d.data.data))
        return ok

    timed(fused, args.warmup)
    if comp:
        timed(comp, args.warmup)
    tf, tc = [], []
    for _ in range(args.rounds):
        tf.append(timed(fused, args.steps))
        if comp:
            tc.append(timed(comp, args.steps))
            comp_out = res.clone() if comp else None
    fused()
    hip.sync()
    ok = parity(res)
    comp_same = None
    if comp:
        comp()
        hip.sync()
        comp_same = bool(torch.equal(res, comp_out)) and ok
        fused()
        hip.sync()
        comp_same = comp_same and bool(torch.equal(res, comp_out))
    ct_bytes = L * cols * n * 8
    nbytes = B * ct_bytes                                   # res written
    for t in plan.terms:
        o = ops.get(t.src)
        if t.src == "dst":
            nbytes += B * ct_bytes
        elif t.src in shared:
            nbytes += o.size * n * 8
        else:
            nbytes += B * o.size * (1 if isinstance(o, Pt) else cols) * n * 8
    mf = statistics.median(tf)
    line = {"op": args.op, "n": n, "limbs": L, "rank": args.rank, "base2k": K, "batch": B, "terms": len(plan.terms), "normalize": plan.normalize,
            "ms_per_call": round(mf * 1e3, 4), "ops_per_s": round(B / mf, 1), "alg_bytes": nbytes, "gbps": round(nbytes / mf / 1e9, 1),
            "frac_peak_8tbs": round(nbytes / mf / PEAK, 3), "frac_copy_6_3tbs": round(nbytes / mf / COPY, 3), "parity": ok,
            "rounds_ms": [round(x * 1e3, 4) for x in tf]}
    if comp:
        mc = statistics.median(tc)
        line.update({"composition_ms_per_call": round(mc * 1e3, 4), "composition_ops_per_s": round(B / mc, 1), "speedup_vs_composition": round(mc / mf, 3),
                     "composition_same_digits": comp_same, "composition_rounds_ms": [round(x * 1e3, 4) for x in tc]})
    print(json.dumps(line))
    return 0 if ok and comp_same is not False else 1


if __name__ == "__main__":
    sys.exit(main())
