#!/usr/bin/env python3
"""Secondary measurement: FheUint words to word on one MI355X (pz_fhe_uint_pack_batched, pz_fhe_uint_execute_batched), legs
in one process on one device, alternated A B A' `--rounds` times.

  pack      A   pz_fhe_uint_pack_batched on the evaluator's [32][batch] bits (by levels)
            B   the same bits through pz_glwe_pack_batched with the word's indices: what poulpy_amd.bdd.fhe_uint_pack does
            A'  A again                               the run-to-run spread of the identical leg
            Both calls clobber their input: every repetition of every leg first restores it by one device copy on the module's stream; the
            copy is timed alone and the rates are given with it and with it subtracted.
  addition  A   pz_fhe_uint_execute_batched(adder(32)) on prepared GGSWs (uniform digits)
            B   pz_bdd_circuit_execute_batched, then leg B of the pack
  round trip    words to word as tools/bench_fhe_uint.py measures it (pz_fhe_uint_prepare_batched on both operands, then the addition), with
            the new call and with the old pair; the pack's share of it from the rates above.  Skipped with --no-round-trip.

Key material is uniform digits - what is measured is time, not noise; A and B must agree bit for bit.  u32 words, rank 1, one base2k.

    python tools/bench_fhe_uint_op.py [--shapes 1024,2048] [--batches 1,16,64] [--rounds 3] [--window 0.3] [--no-round-trip] [--gpus 1]

Prints one JSON line per (shape, batch)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_fhe_uint import GGSW_SIZE, K, W, WORD_SIZE, Shape, timed  # noqa: E402

VP = C.c_void_p


def without(rate, copy_rate):
    """calls / s of a leg with the restoring copy's time taken out"""
    t = 1.0 / rate - 1.0 / copy_rate
    return 1.0 / t if t > 0 else float("inf")


def bench(sh, batch, args):
    import torch
    from poulpy_amd import bdd
    mod, n = sh.mod, sh.n
    key = sh.key_view()
    src = sh.digits((W, batch, GGSW_SIZE, 2, n))
    bits = torch.zeros_like(src)
    res_a, res_b = (torch.zeros((batch, GGSW_SIZE, 2, n), dtype=torch.int64, device="cuda:0") for _ in range(2))
    pk_new = mod.device_alloc(mod.fhe_uint_pack_tmp_bytes(sh.pack, W, batch))
    pk_old = mod.device_alloc(max(mod.glwe_pack_tmp_bytes(sh.pack, batch), 8))
    polys = W * batch * GGSW_SIZE * 2
    torch.cuda.synchronize()

    def restore():   # one launch on the module's stream: the buffer as `polys` one-limb, one-column objects
        mod._ck(mod.lib.pz_vec_znx_copy_batched(mod.handle, polys, VP(bits.data_ptr()), 1, 1, 0, VP(src.data_ptr()), 1, 1, 0))

    def pack_a():
        restore()
        mod.fhe_uint_pack_batched(VP(res_a.data_ptr()), VP(bits.data_ptr()), W, sh.gals, key.atk, sh.pack, pk_new.ptr, pk_new.nbytes, batch)

    def pack_b(out=bits):
        if out is bits:
            restore()
        bdd.fhe_uint_pack(mod, VP(res_b.data_ptr()), VP(out.data_ptr()), W, sh.gals, key.atk, sh.pack, batch, tmp=pk_old)
    mod.dispatch_notes(reset=True)
    for leg in (pack_a, pack_b):
        for _ in range(args.warmup):
            leg()
    mod.sync()
    notes = mod.dispatch_notes()     # (from the warm-up: a replayed graph leaves none)
    same = bool(torch.equal(res_a, res_b))
    a, b, a2, cp = [], [], [], []
    for _ in range(args.rounds):
        a.append(timed(mod, pack_a, args.window))
        b.append(timed(mod, pack_b, args.window))
        a2.append(timed(mod, pack_a, args.window))
        cp.append(timed(mod, restore, args.window))
    ma, mb, ma2, mcp = (statistics.median(x) for x in (a, b, a2, cp))
    spread = abs(ma - ma2) / ma
    line = {
        "metric": "u32 FheUint words packed / s (pz_fhe_uint_pack_batched, restoring copy included)", "unit": "words/s", "value": ma * batch,
        "packs_per_s": [x * batch for x in a], "general_pack_per_s": [x * batch for x in b], "again_packs_per_s": [x * batch for x in a2],
        "restore_copies_per_s": cp, "new_over_general": ma / mb, "new_over_general_copy_subtracted": without(ma, mcp) / without(mb, mcp),
        "packs_per_s_copy_subtracted": without(ma, mcp) * batch, "general_pack_per_s_copy_subtracted": without(mb, mcp) * batch,
        "spread_same_leg": spread, "not_slower_beyond_spread": bool(ma >= mb * (1.0 - spread)), "pack_legs_bit_identical": same,
    }
    # ---- the addition: evaluator + pack in one call against the two calls ----
    circuit = mod.bdd_circuit_new(bdd.adder(W))
    ggsw = sh.digits((batch * 2 * W, 2, 2, GGSW_SIZE, 2, n))
    pm = torch.empty(ggsw.shape, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    mod.ggsw_prepare_batched(VP(pm.data_ptr()), VP(ggsw.data_ptr()), batch * 2 * W, 2, 1, GGSW_SIZE)
    mod.sync()
    del ggsw
    gb = sh.ggsw_doubles * 8
    rows = [[VP(pm.data_ptr() + ((e * 2 + w) * W + i) * gb) for w in (0, 1) for i in range(W)] for e in range(batch)]
    out = torch.zeros((W, batch, GGSW_SIZE, 2, n), dtype=torch.int64, device="cuda:0")
    ev_tmp = mod.device_alloc(max(mod.bdd_circuit_execute_tmp_bytes(circuit, sh.gate, batch), 8))
    op_tmp = mod.device_alloc(mod.fhe_uint_execute_tmp_bytes(circuit, sh.gate, sh.pack, W, batch))
    torch.cuda.synchronize()

    def add_a(bits_rows=rows):
        mod.fhe_uint_execute_batched(circuit, VP(res_a.data_ptr()), W, bits_rows, sh.gate, sh.gals, key.atk, sh.pack, op_tmp.ptr, op_tmp.nbytes, batch)

    def add_b(bits_rows=rows):
        mod.bdd_circuit_execute_batched(circuit, VP(out.data_ptr()), W, bits_rows, sh.gate, ev_tmp.ptr, ev_tmp.nbytes, batch)
        pack_b(out)
    for leg in (add_a, add_b):
        for _ in range(args.warmup):
            leg()
    mod.sync()
    same_add = bool(torch.equal(res_a, res_b))
    ea, eb, ea2 = [], [], []
    for _ in range(args.rounds):
        ea.append(timed(mod, add_a, args.window))
        eb.append(timed(mod, add_b, args.window))
        ea2.append(timed(mod, add_a, args.window))
    mea, meb, mea2 = (statistics.median(x) for x in (ea, eb, ea2))
    spread_add = abs(mea - mea2) / mea
    line.update({
        "additions_per_s_prepared_inputs": [x * batch for x in ea], "additions_per_s_two_calls": [x * batch for x in eb],
        "again_additions_per_s": [x * batch for x in ea2], "addition_new_over_two_calls": mea / meb, "addition_spread_same_leg": spread_add,
        "addition_not_slower_beyond_spread": bool(mea >= meb * (1.0 - spread_add)), "addition_legs_bit_identical": same_add,
        "pack_share_of_addition": mea / without(ma, mcp), "general_pack_share_of_two_calls": meb / without(mb, mcp),
    })
    # ---- words to word: prepare both operands, then the addition ----
    if args.round_trip:
        words = sh.digits((2 * batch, WORD_SIZE, 2, n))
        pm_w = torch.zeros((2 * batch, W, sh.ggsw_doubles), dtype=torch.float64, device="cuda:0")
        pr_tmp = mod.device_alloc(mod.fhe_uint_prepare_tmp_bytes(sh.p, 2 * batch))
        base = pm_w.data_ptr()
        wrows = [[VP(base + ((w * batch + e) * W + i) * gb) for w in (0, 1) for i in range(W)] for e in range(batch)]
        torch.cuda.synchronize()

        def prepare():
            mod.fhe_uint_prepare_batched(VP(pm_w.data_ptr()), VP(words.data_ptr()), None, key.ks_lwe, key.lut, key.brk, key.gals, key.atk, key.tsk, sh.p,
                                         pr_tmp.ptr, pr_tmp.nbytes, 2 * batch)

        def trip_a():
            prepare()
            add_a(wrows)

        def trip_b():
            prepare()
            add_b(wrows)
        for leg in (trip_a, trip_b):
            for _ in range(args.warmup):
                leg()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(mod, trip_a, args.window))
            tb.append(timed(mod, trip_b, args.window))
        mta, mtb = statistics.median(ta), statistics.median(tb)
        line.update({
            "encrypted_32bit_additions_per_s_words_to_word": mta * batch, "words_to_word_two_calls_per_s": mtb * batch,
            "words_to_word_per_s": [x * batch for x in ta], "pack_share_of_round_trip": mta / without(ma, mcp),
            "general_pack_share_of_old_round_trip": mtb / without(mb, mcp),
        })
        pr_tmp.free()
    else:
        line.update({"encrypted_32bit_additions_per_s_words_to_word": "not measured", "pack_share_of_round_trip": "not measured"})
    line.update({"graph_launches": mod.graph_launches(),
                 "config": {"n": n, "rank": 1, "base2k": K, "batch": batch, "word_bits": W, "limbs": GGSW_SIZE, "rounds": args.rounds, "window_s": args.window,
                            "n_lwe": sh.n_lwe},
                 "dispatch_notes": notes})
    print(json.dumps(line), flush=True)
    mod.bdd_circuit_free(circuit)
    for t in (pk_new, pk_old, ev_tmp, op_tmp):
        t.free()
    if not (same and same_add):
        raise SystemExit(3)   # a fast wrong answer is not a result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024,2048", help="ring degrees, comma separated")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-lwe", type=int, default=77)
    ap.add_argument("--no-round-trip", dest="round_trip", action="store_false")
    ap.add_argument("--gpus", type=int, default=1)
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_fhe_uint_op.py measures one device (--gpus 1)")
    for n in (int(x) for x in args.shapes.split(",")):
        sh = Shape(n, args.n_lwe)
        for batch in (int(x) for x in args.batches.split(",")):
            bench(sh, batch, args)
        sh.mod.close()


if __name__ == "__main__":
    main()
