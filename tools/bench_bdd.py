#!/usr/bin/env python3
"""Secondary measurement: encrypted 32-bit additions per second on one MI355X through the BDD circuit evaluator
(pz_bdd_circuit_execute_batched on poulpy_amd.bdd.adder(32): 1584 CMUX gates in 64 levels), legs in one process on one device.

    A   the call as it is                                   gathered route: one launch per level, every ciphertext with its own key
    A'  A again                                             the run-to-run spread of the identical leg
    B   the same compiled schedule, POULPY_DBG_BDD_GATHER=0  one CMUX per (gate, input) on the existing kernels, copies renamed, one HIP graph
    C   (--walk, one line) the literal node-by-node walk through the public pz_glwe_cmux_batched (one call per gate and input: every input
        has its own GGSWs) and pz_vec_znx_copy_batched (one call per Copy node and column, over the batch), two banks per output

Every (input, input bit) has its OWN GGSW buffer, pinned (the contents repeat a pool of --distinct prepared keys: what is measured is traffic,
and a key per (input, selector) is fetched from its own address).  The legs alternate A B A' `--rounds` times, every leg warmed (the third
identical call is the first graph replay), every window at least `--window` seconds of device work ending in a synchronise.  Reported per
(shape, batch): additions / s and CMUX gates / s of each leg, A / B, the spread |A - A'| / A, and A's gates / s over the rate of
pz_glwe_cmux_batched on 4096 ciphertexts sharing ONE pinned key, measured in the same process (tools/bench_cmux.py's leg A): the price of one key
per (input, selector).  A and B must agree bit for bit (and C, where it runs); input 0 of the first batch of a shape is checked against the oracle.

    python tools/bench_bdd.py [--shapes 1024:3,2048:3,4096:4] [--batches 1,16,64] [--rounds 3] [--window 0.5] [--walk 1024:16]
                              [--per-gate-max-batch 16] [--gpus 1]

Prints one JSON line per (shape, batch)."""
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
W = 32


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


class Shape:
    """One ring degree: the module, max_batch x 64 pinned key buffers filled from a pool of `distinct` prepared GGSWs, which pool key each is"""

    def __init__(self, n, size, k, max_batch, distinct, seed=0x626464):
        import torch
        from poulpy_amd.hal import GlweOpParams, Module
        from poulpy_amd.layouts import MatZnx
        self.n, self.size, self.k, self.cols = n, size, k, 2
        self.mod = mod = Module(n, device=0)
        rng = np.random.default_rng(seed)
        self.mats, self.pool = [], []
        for _ in range(distinct):
            mat = MatZnx(n, size, 2, 2, size).fill_uniform(k, rng)
            pm = mod.vmp_pmat_alloc(size, 2, 2, size)
            mod.vmp_prepare(pm, mat)
            self.mats.append(mat)
            self.pool.append(torch.from_numpy(pm.data.view(np.float64).reshape(-1)).to("cuda:0"))
        self.which = rng.integers(0, distinct, (max_batch, 2 * W))
        self.keys = []                                   # [b][i]: a torch buffer of its own
        for b in range(max_batch):
            row = []
            for i in range(2 * W):
                buf = self.pool[self.which[b, i]].clone()
                row.append(buf)
            self.keys.append(row)
        torch.cuda.synchronize()
        for row in self.keys:
            for buf in row:
                mod.pin_key(VP(buf.data_ptr()), size, 2, 2, size)
        self.p = GlweOpParams(rank=1, dnum=size, dsize=1, key_size=size, key_base2k=k, a_size=size, a_base2k=k, res_size=size, res_base2k=k, rank_out=1)

    def bits(self, batch):
        return [[VP(buf.data_ptr()) for buf in self.keys[b]] for b in range(batch)]

    def shared_key_rate(self, window, batch=4096):
        """pz_glwe_cmux_batched on `batch` ciphertexts under ONE pinned key: gates / s"""
        import torch
        half = 1 << (self.k - 1)
        t = torch.randint(-half, half, (batch, self.size, 2, self.n), dtype=torch.int64, device="cuda:0")
        f = torch.randint(-half, half, (batch, self.size, 2, self.n), dtype=torch.int64, device="cuda:0")
        res = torch.zeros_like(t)
        torch.cuda.synchronize()
        key = VP(self.keys[0][0].data_ptr())

        def gate():
            self.mod.glwe_cmux_batched(VP(res.data_ptr()), VP(t.data_ptr()), VP(f.data_ptr()), key, self.p, batch, t_size=self.size, f_size=self.size)
        gate()
        return timed(self.mod, gate, window) * batch


def walk(sh, circuit, banks, out, bits, batch):
    """leg C: eval_level node by node through the public entry points; banks: torch (outputs, 2 S, batch, size, cols, n), zero but slot 1"""
    mod, p, size, cols = sh.mod, sh.p, sh.size, sh.cols
    ct = size * cols * sh.n * 8
    for o, (nodes, s) in enumerate(circuit.outputs):
        base = banks[o].data_ptr()

        def slot(bank, j, b=0):
            return VP(base + ((bank * s + j) * batch + b) * ct)
        prev, nxt = 0, 1
        for c in range(0, len(nodes), s):
            last = c + s == len(nodes)
            for j, (kind, sel, hi, lo) in enumerate(nodes[c:c + s]):
                if kind == 2:
                    for b in range(batch):
                        dst = VP(out.data_ptr() + (o * batch + b) * ct) if last else slot(nxt, j, b)
                        mod.glwe_cmux_batched(dst, slot(prev, hi, b), slot(prev, lo, b), bits[b][sel], p, 1, t_size=size, f_size=size)
                elif kind == 1:
                    for col in range(cols):
                        mod.lib.pz_vec_znx_copy_batched(mod.handle, batch, slot(nxt, j), cols, size, col, slot(prev, j), cols, size, col)
            prev, nxt = nxt, prev


def oracle_input0(sh, circuit, n_out):
    from oracle.ref import RefModule
    from tests import bdd_oracle as bo
    ref = RefModule(sh.n)
    prepared = []
    for mat in sh.mats:
        pr = ref.vmp_pmat_alloc(mat.rows, 2, 2, sh.size)
        ref.vmp_prepare(pr, mat)
        prepared.append(pr)
    outs = bo.execute_bdd_circuit(ref, circuit, lambda i: prepared[sh.which[0, i]], n_out, 2, sh.size, sh.k)
    return np.stack([ct.data for ct in outs])


def bench(sh, circuit, handle, batch, args, shared, do_walk, check_oracle):
    import torch
    mod, p = sh.mod, sh.p
    n_out, gates = circuit.output_size, circuit.count(2)
    bits = sh.bits(batch)
    out_a = torch.zeros((n_out, batch, sh.size, 2, sh.n), dtype=torch.int64, device="cuda:0")
    out_b = torch.zeros_like(out_a)
    tmp = mod.device_alloc(max(mod.bdd_circuit_execute_tmp_bytes(handle, p, batch), 8))
    torch.cuda.synchronize()

    def call(out):
        mod.bdd_circuit_execute_batched(handle, VP(out.data_ptr()), n_out, bits, p, tmp.ptr, tmp.nbytes, batch)

    def leg_a():
        call(out_a)

    def leg_b():
        os.environ["POULPY_DBG_BDD_GATHER"] = "0"
        try:
            call(out_b)
        finally:
            os.environ.pop("POULPY_DBG_BDD_GATHER")
    notes = {}
    with_b = batch <= args.per_gate_max_batch   # (one kernel node per gate and input in its graph: 100 000 of them at batch 64)
    for name, leg in (("default", leg_a), ("POULPY_DBG_BDD_GATHER=0", leg_b))[:2 if with_b else 1]:
        mod.dispatch_notes(reset=True)
        for _ in range(max(args.warmup, 3)):
            leg()
        mod.sync()
        notes[name] = mod.dispatch_notes()
    a, b, a2 = [], [], []
    for _ in range(args.rounds):
        a.append(timed(mod, leg_a, args.window) * batch)
        if with_b:
            b.append(timed(mod, leg_b, args.window) * batch)
        a2.append(timed(mod, leg_a, args.window) * batch)
    same = not with_b or bool(torch.equal(out_a, out_b))
    c_rate = None
    if do_walk:
        s_max = circuit.max_state_size
        banks = torch.zeros((n_out, 2 * s_max, batch, sh.size, 2, sh.n), dtype=torch.int64, device="cuda:0")
        out_c = torch.zeros_like(out_a)

        def leg_c():
            mod.sync()
            banks.zero_()
            for o, (_, s) in enumerate(circuit.outputs):   # slot 1 of the 2 s slots of every output: the constant one
                banks[o].view(-1, batch, sh.size, 2, sh.n)[1, :, 0, 0, 0] = 1 << (sh.k - 2)
            torch.cuda.synchronize()
            walk(sh, circuit, [banks[o] for o in range(n_out)], out_c, bits, batch)
        leg_c()
        mod.sync()
        same = same and bool(torch.equal(out_a, out_c))
        c_rate = timed(mod, leg_c, args.window) * batch
    ok = None
    if check_oracle:
        ok = bool(np.array_equal(out_a[:, 0].cpu().numpy(), oracle_input0(sh, circuit, n_out)))
    ma, ma2 = statistics.median(a), statistics.median(a2)
    mb = statistics.median(b) if b else None
    print(json.dumps({
        "metric": "encrypted 32-bit additions / s (pz_bdd_circuit_execute_batched, adder(32): 1584 CMUX gates, 64 levels)", "unit": "additions/s",
        "value": ma, "additions_per_s": a, "per_gate_route_additions_per_s": b or None, "again_additions_per_s": a2, "node_walk_additions_per_s": c_rate,
        "gates_per_s": ma * gates, "per_gate_route_gates_per_s": mb * gates if mb else None, "default_over_per_gate": ma / mb if mb else None,
        "default_over_node_walk": ma / c_rate if c_rate else None, "spread_same_leg": abs(ma - ma2) / ma,
        "shared_key_cmux_gates_per_s": shared, "gates_per_s_over_shared_key": ma * gates / shared,
        "routes_bit_identical": same, "parity_ok_input0": ok, "graph_launches": mod.graph_launches(),
        "config": {"n": sh.n, "rank": 1, "limbs": sh.size, "base2k": sh.k, "batch": batch, "keys": batch * 2 * W, "rounds": args.rounds,
                   "window_s": args.window, "levels": circuit.max_depth, "gates": gates},
        "dispatch_notes": notes}), flush=True)
    tmp.free()
    if ok is False or not same:
        raise SystemExit(3)   # a fast wrong answer is not a result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024:3,2048:3,4096:4", help="N:limbs, comma separated (rank 1)")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--base2k", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8, help="prepared GGSWs the key buffers are filled from")
    ap.add_argument("--walk", default="1024:16", help="N:batch of the one line that also times the node-by-node walk ('' for none)")
    ap.add_argument("--per-gate-max-batch", type=int, default=16, help="leg B is timed up to this batch (above it: not measured)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_bdd.py measures one device (--gpus 1)")
    from poulpy_amd import bdd
    circuit = bdd.adder(W)
    batches = [int(x) for x in args.batches.split(",")]
    for spec in args.shapes.split(","):
        n, size = (int(x) for x in spec.split(":"))
        sh = Shape(n, size, args.base2k, max(batches), args.distinct)
        handle = sh.mod.bdd_circuit_new(circuit)
        shared = sh.shared_key_rate(args.window)
        for i, batch in enumerate(batches):
            bench(sh, circuit, handle, batch, args, shared, args.walk == f"{n}:{batch}", i == 0 and not args.no_parity)
        sh.mod.bdd_circuit_free(handle)
        sh.mod.close()


if __name__ == "__main__":
    main()
