#!/usr/bin/env python3
"""Secondary measurement: FheUint words prepared per second on one MI355X (pz_fhe_uint_prepare_batched), legs in one process
on one device.

    A   the call as it is: u32 words in, 32 prepared GGSWs per word out
    A'  A again                                  the run-to-run spread of the identical leg
    B   the same work through the entry points that existed before it: one pz_lwe_from_glwe_batched + pz_lwe_mod_switch_2n_batched per
        bit, ONE pz_circuit_bootstrapping_execute_to_constant_batched over all bits, one pz_vmp_prepare per GGSW
    C   the circuit bootstrapping of B alone: its share of A bounds what the rest of the call can gain

and one more figure per line: encrypted 32-bit additions per second from words to word (prepare both operands, adder(32) on the evaluator,
glwe_pack).  Key material is uniform digits - what is measured is time, not noise; A and B must agree bit for bit.  Rank 1, one base2k for
every object, no rank-reducing key switch; `--n-lwe` defaults to the 77 of the reference's own test of this path.

    python tools/bench_fhe_uint.py [--shapes 1024,2048] [--batches 1,16,64] [--rounds 3] [--window 0.3] [--n-lwe 77] [--gpus 1]

Prints one JSON line per (shape, batch)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
VP = C.c_void_p
W = 32
K, WORD_SIZE, GGSW_SIZE, GGSW_DNUM, KEY_SIZE, KEY_DNUM, BLOCK = 13, 2, 3, 2, 4, 4, 7


def timed(mod, run, window):
    """calls of `run` per second over a window of at least `window` seconds (sized from a first timed call), ending in a synchronise"""
    mod.sync()
    t0 = time.perf_counter()
    run()
    mod.sync()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(2, int(window / one) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    mod.sync()
    return reps / (time.perf_counter() - t0)


class Shape:
    """One ring degree: the module and a BDD key of uniform digits, prepared on the device"""

    def __init__(self, n, n_lwe, seed=0x66687569):
        import torch
        from poulpy_amd.hal import BlindRotationParams, CircuitBootstrappingParams, FheUintPrepareParams, GlweOpParams, Module
        self.n, self.n_lwe = n, n_lwe
        self.mod = mod = Module(n, device=0)
        self.gen = torch.Generator(device="cuda:0").manual_seed(seed)
        self.keep = []

        def prepared(count, rows, cols_in, cols_out, size):
            mats = self.digits((count, rows, cols_in, size, cols_out, n))
            pm = torch.empty(mats.shape, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            if cols_in == cols_out:
                mod.ggsw_prepare_batched(VP(pm.data_ptr()), VP(mats.data_ptr()), count, rows, cols_in - 1, size)
            else:
                for i in range(count):
                    mod.lib.pz_vmp_prepare(mod.handle, VP(pm[i].data_ptr()), VP(mats[i].data_ptr()), rows, cols_in, cols_out, size)
            mod.sync()
            self.keep.append(pm)
            return pm
        self.brk = prepared(n_lwe, KEY_DNUM, 2, 2, KEY_SIZE)
        log_n = n.bit_length() - 1
        self.gals = [-1] + [pow(5, 1 << i, 2 * n) for i in range(log_n - 1)]
        self.atk = [prepared(1, KEY_DNUM, 1, 2, KEY_SIZE) for _ in self.gals]
        self.tsk = [prepared(1, KEY_DNUM, 1, 2, KEY_SIZE)]
        self.ks_lwe = prepared(1, WORD_SIZE, 1, 2, WORD_SIZE + 1)
        self.lut = self.digits((GGSW_DNUM, 1, n))
        cbt = CircuitBootstrappingParams(
            br=BlindRotationParams(rank=1, n_lwe=n_lwe, block_size=BLOCK, dnum=KEY_DNUM, brk_size=KEY_SIZE, base2k=K, res_size=KEY_SIZE, lut_size=GGSW_DNUM),
            atk_dnum=KEY_DNUM, atk_size=KEY_SIZE, tsk_dnum=KEY_DNUM, tsk_size=KEY_SIZE, res_dnum=GGSW_DNUM, res_size=GGSW_SIZE, gap=n // 8,
            atk_base2k=K, tsk_base2k=K, res_base2k=K, atk_glwe_size=KEY_SIZE, trace_size=KEY_SIZE)
        self.ks = GlweOpParams(rank=1, dnum=WORD_SIZE, dsize=1, key_size=WORD_SIZE + 1, key_base2k=K, a_size=WORD_SIZE, a_base2k=K, res_size=WORD_SIZE,
                               res_base2k=K, rank_out=1)
        self.p = FheUintPrepareParams(cbt=cbt, ks_glwe=GlweOpParams(), ks_lwe=self.ks, n_lwe=n_lwe, lwe_size=WORD_SIZE, lwe_base2k=K, word_bits=W,
                                      bit_start=0, bit_count=W)
        self.gate = GlweOpParams(rank=1, dnum=GGSW_DNUM, dsize=1, key_size=GGSW_SIZE, key_base2k=K, a_size=GGSW_SIZE, a_base2k=K, res_size=GGSW_SIZE,
                                 res_base2k=K, rank_out=1)
        self.pack = GlweOpParams(rank=1, dnum=KEY_DNUM, dsize=1, key_size=KEY_SIZE, key_base2k=K, a_size=GGSW_SIZE, a_base2k=K, res_size=GGSW_SIZE,
                                 res_base2k=K, rank_out=1)
        self.ggsw_doubles = GGSW_DNUM * 4 * GGSW_SIZE * n

    def digits(self, shape):
        import torch
        return torch.randint(-(1 << (K - 1)), 1 << (K - 1), shape, dtype=torch.int64, device="cuda:0", generator=self.gen)

    def key_view(self):
        from types import SimpleNamespace
        return SimpleNamespace(ks_glwe=None, ks_lwe=VP(self.ks_lwe.data_ptr()), lut=VP(self.lut.data_ptr()), brk=VP(self.brk.data_ptr()), gals=self.gals,
                               atk=[VP(k.data_ptr()) for k in self.atk], tsk=[VP(k.data_ptr()) for k in self.tsk])


def bench(sh, batch, args):
    import torch
    from poulpy_amd import bdd
    mod, p, n, n_lwe = sh.mod, sh.p, sh.n, sh.n_lwe
    key = sh.key_view()
    nb = batch * W
    words = sh.digits((2 * batch, WORD_SIZE, 2, n))          # both operands of the additions; the legs prepare the first `batch`
    pm_a = torch.zeros((2 * batch, W, sh.ggsw_doubles), dtype=torch.float64, device="cuda:0")
    pm_b = torch.zeros((W, batch, sh.ggsw_doubles), dtype=torch.float64, device="cuda:0")           # leg B works bit-major
    lwe = torch.zeros((W, batch, WORD_SIZE, n_lwe + 1), dtype=torch.int64, device="cuda:0")
    lwe_2n = torch.zeros((W, batch, n_lwe + 1), dtype=torch.int64, device="cuda:0")
    ggsw = torch.zeros((W, batch, sh.ggsw_doubles), dtype=torch.int64, device="cuda:0")
    tmp = mod.device_alloc(mod.fhe_uint_prepare_tmp_bytes(p, 2 * batch))
    cbt_tmp = mod.device_alloc(mod.circuit_bootstrapping_tmp_bytes(p.cbt, nb))
    coef = [bdd.bit_index(i, W) * (n // W) for i in range(W)]
    torch.cuda.synchronize()

    def leg_a(count=batch):
        mod.fhe_uint_prepare_batched(VP(pm_a.data_ptr()), VP(words.data_ptr()), None, key.ks_lwe, key.lut, key.brk, key.gals, key.atk, key.tsk, p, tmp.ptr,
                                     tmp.nbytes, count)

    def leg_c():
        mod.circuit_bootstrapping_execute_to_constant_batched(VP(ggsw.data_ptr()), VP(lwe_2n.data_ptr()), key.lut, key.brk, key.gals, key.atk, key.tsk,
                                                              p.cbt, cbt_tmp.ptr, cbt_tmp.nbytes, nb)

    def leg_b():
        for i in range(W):
            mod.lwe_from_glwe_batched(VP(lwe[i].data_ptr()), n_lwe, VP(words.data_ptr()), coef[i], key.ks_lwe, sh.ks, batch)
            mod.lwe_mod_switch_2n_batched(VP(lwe_2n[i].data_ptr()), VP(lwe[i].data_ptr()), n_lwe, WORD_SIZE, K, 2 * n, True, batch)
        leg_c()
        g, q = ggsw.data_ptr(), pm_b.data_ptr()
        for j in range(nb):
            mod.lib.pz_vmp_prepare(mod.handle, VP(q + j * sh.ggsw_doubles * 8), VP(g + j * sh.ggsw_doubles * 8), GGSW_DNUM, 2, 2, GGSW_SIZE)
    for leg in (leg_a, leg_b):
        for _ in range(args.warmup):
            leg()
    mod.sync()
    same = bool(torch.equal(pm_a[:batch].view(torch.int64), pm_b.permute(1, 0, 2).contiguous().view(torch.int64)))
    a, b, a2, c = [], [], [], []
    for _ in range(args.rounds):
        a.append(timed(mod, leg_a, args.window) * batch)
        b.append(timed(mod, leg_b, args.window) * batch)
        a2.append(timed(mod, leg_a, args.window) * batch)
        c.append(timed(mod, leg_c, args.window) * batch)
    # words to word: prepare both operands, the adder, pack
    circuit = mod.bdd_circuit_new(bdd.adder(W))
    out = torch.zeros((W, batch, GGSW_SIZE, 2, n), dtype=torch.int64, device="cuda:0")
    res = torch.zeros((batch, GGSW_SIZE, 2, n), dtype=torch.int64, device="cuda:0")
    ev_tmp = mod.device_alloc(max(mod.bdd_circuit_execute_tmp_bytes(circuit, sh.gate, batch), 8))
    pk_tmp = mod.device_alloc(max(mod.glwe_pack_tmp_bytes(sh.pack, batch), 8))
    base, gb = pm_a.data_ptr(), sh.ggsw_doubles * 8
    bits = [[VP(base + ((w * batch + e) * W + i) * gb) for w in (0, 1) for i in range(W)] for e in range(batch)]
    torch.cuda.synchronize()

    def addition():
        leg_a(2 * batch)
        mod.bdd_circuit_execute_batched(circuit, VP(out.data_ptr()), W, bits, sh.gate, ev_tmp.ptr, ev_tmp.nbytes, batch)
        bdd.fhe_uint_pack(mod, VP(res.data_ptr()), VP(out.data_ptr()), W, sh.gals, key.atk, sh.pack, batch, tmp=pk_tmp)
    for _ in range(args.warmup):
        addition()
    adds = [timed(mod, addition, args.window) * batch for _ in range(args.rounds)]
    ma, mb, ma2, mc = (statistics.median(x) for x in (a, b, a2, c))
    spread_a, spread_b = abs(ma - ma2) / ma, (max(b) - min(b)) / mb
    print(json.dumps({
        "metric": "u32 FheUint words prepared / s (pz_fhe_uint_prepare_batched: 32 circuit bootstrappings + ggsw_prepare per word)", "unit": "words/s",
        "value": ma, "words_per_s": a, "existing_entry_points_words_per_s": b, "again_words_per_s": a2, "new_over_existing": ma / mb,
        "spread_same_leg": spread_a, "spread_existing_leg": spread_b, "not_slower_beyond_spread": bool(ma >= mb * (1.0 - max(spread_a, spread_b))),
        "circuit_bootstrapping_alone_words_per_s": c, "circuit_bootstrapping_share_of_call": ma / mc,
        "encrypted_32bit_additions_per_s_words_to_word": statistics.median(adds), "additions_per_s": adds,
        "legs_bit_identical": same, "graph_launches": mod.graph_launches(),
        "config": {"n": n, "rank": 1, "base2k": K, "n_lwe": n_lwe, "block_size": BLOCK, "batch": batch, "word_bits": W, "rounds": args.rounds,
                   "window_s": args.window, "ggsw": [GGSW_DNUM, GGSW_SIZE], "keys": [KEY_DNUM, KEY_SIZE]},
        "dispatch_notes": mod.dispatch_notes()}), flush=True)
    mod.bdd_circuit_free(circuit)
    for t in (tmp, cbt_tmp, ev_tmp, pk_tmp):
        t.free()
    if not same:
        raise SystemExit(3)   # a fast wrong answer is not a result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024,2048", help="ring degrees, comma separated")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-lwe", type=int, default=77)
    ap.add_argument("--gpus", type=int, default=1)
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_fhe_uint.py measures one device (--gpus 1)")
    for n in (int(x) for x in args.shapes.split(",")):
        sh = Shape(n, args.n_lwe)
        for batch in (int(x) for x in args.batches.split(",")):
            bench(sh, batch, args)
        sh.mod.close()


if __name__ == "__main__":
    main()
