#!/usr/bin/env python3
"""Secondary measurement: the FheUint byte operations on one MI355X (pz_fhe_uint_get_batched, pz_fhe_uint_splice_batched,
pz_fhe_uint_sext_batched), legs in one process on one device, alternated A B A' `--rounds` times.

    A   the new call (by stages)
    B   the same operation through the entry points that existed before it, in the reference's order: pz_vec_znx_rotate_batched (one launch
        per glwe_rotate: the batch's polynomials as one-limb objects), pz_glwe_trace_batched (one per trace), pz_vec_znx_copy_batched /
        _add_assign_batched / _sub_assign_batched (one launch each)
    A'  A again                               the run-to-run spread of the identical leg

Operations: get of all 32 bits, splice_u8(1, 2), splice_u16(1, 0), sext(0) on u32 words.  sext works in place: both of its legs first restore
the word by one device copy, which is timed alone; its rates are given with the copy and with it subtracted.  Key material and words are
uniform digits - what is measured is time, not noise; A and B must agree bit for bit.  Rank 1, one base2k.

    python tools/bench_fhe_uint_bytes.py [--shapes 1024,2048] [--batches 1,16,64] [--rounds 3] [--window 0.3] [--gpus 1]

Prints one JSON line per (shape, batch, operation)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_fhe_uint import GGSW_SIZE, K, KEY_DNUM, KEY_SIZE, W, timed  # noqa: E402

VP = C.c_void_p
TS = 3


class Shape:
    """One ring degree: the module and the log2(n) automorphism keys, uniform digits, prepared on the device"""

    def __init__(self, n, seed=0x62797465):
        import torch
        from poulpy_amd.hal import GlweOpParams, Module
        self.n = n
        self.mod = mod = Module(n, device=0)
        self.gen = torch.Generator(device="cuda:0").manual_seed(seed)
        self.gals = [-1] + [pow(5, 1 << i, 2 * n) for i in range(n.bit_length() - 2)]
        self.keep = []
        for _ in self.gals:
            mat = self.digits((KEY_DNUM, 1, KEY_SIZE, 2, n))
            pm = torch.empty(mat.shape, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            mod.lib.pz_vmp_prepare(mod.handle, VP(pm.data_ptr()), VP(mat.data_ptr()), KEY_DNUM, 1, 2, KEY_SIZE)
            mod.sync()
            self.keep.append(pm)
        self.atk = [VP(k.data_ptr()) for k in self.keep]
        self.p = GlweOpParams(rank=1, dnum=KEY_DNUM, dsize=1, key_size=KEY_SIZE, key_base2k=K, a_size=GGSW_SIZE, a_base2k=K, res_size=GGSW_SIZE,
                              res_base2k=K, rank_out=1)

    def digits(self, shape):
        import torch
        return torch.randint(-(1 << (K - 1)), 1 << (K - 1), shape, dtype=torch.int64, device="cuda:0", generator=self.gen)


def without(rate, copy_rate):
    """calls / s of a leg with the restoring copy's time taken out"""
    t = 1.0 / rate - 1.0 / copy_rate
    return 1.0 / t if t > 0 else float("inf")


def bench(sh, batch, args):
    import torch
    from poulpy_amd import abi
    from poulpy_amd.hal import fhe_uint_bit_coefficient
    mod, n, p = sh.mod, sh.n, sh.p
    shape = (batch, GGSW_SIZE, 2, n)
    polys = batch * GGSW_SIZE * 2
    a, b, word0 = sh.digits(shape), sh.digits(shape), sh.digits(shape)
    new = lambda *lead: torch.zeros(lead + shape, dtype=torch.int64, device="cuda:0")   # noqa: E731
    res_a, res_b, bits_a, bits_b, word = new(), new(), new(W), new(W), new()
    t = [new() for _ in range(6)]
    tmp = mod.device_alloc(mod.fhe_uint_word_op_tmp_bytes(p, W, batch, W))
    torch.cuda.synchronize()
    ptr = lambda x: VP(x.data_ptr())   # noqa: E731
    c = lambda bit: fhe_uint_bit_coefficient(n, W, bit)   # noqa: E731

    # ---- leg B: the parent commit's entry points, the reference's calls in its order (fhe_uint.rs:259-524) ----
    def rot(k, dst, src):
        mod._ck(mod.lib.pz_vec_znx_rotate_batched(mod.handle, polys, k, ptr(dst), 1, 1, 0, ptr(src), 1, 1, 0))

    def ew(name, dst, src):
        mod._ck(getattr(mod.lib, name)(mod.handle, polys, ptr(dst), 1, 1, 0, ptr(src), 1, 1, 0))

    def trace(x, skip):
        mod.glwe_trace_batched(ptr(x), sh.gals[skip:], sh.atk[skip:], p, batch)

    def zero_byte_b(res, src, r):
        rot(-r, t[0], src)
        ew("pz_vec_znx_copy_batched", t[1], t[0])
        trace(t[1], TS)
        ew("pz_vec_znx_sub_assign_batched", t[0], t[1])
        rot(r, res, t[0])

    def splice8_b(res, x, y, dst, src):
        zero_byte_b(res, x, c(8 * dst))
        rot(-c(8 * src), t[2], y)
        trace(t[2], TS)
        rot(c(8 * dst), t[3], t[2])
        ew("pz_vec_znx_add_assign_batched", res, t[3])

    def restore():
        ew("pz_vec_znx_copy_batched", word, word0)

    def get_a():
        mod.fhe_uint_get_batched(ptr(bits_a), ptr(a), W, abi.PZ_WORD_BIT, list(range(W)), sh.gals, sh.atk, p, tmp.ptr, tmp.nbytes, batch)

    def get_b():
        for i in range(W):
            rot(-c(i), bits_b[i], a)
            trace(bits_b[i], 0)

    def s8_a():
        mod.fhe_uint_splice_batched(ptr(res_a), ptr(a), ptr(b), W, 8, 1, 2, sh.gals, sh.atk, p, tmp.ptr, tmp.nbytes, batch)

    def s8_b():
        splice8_b(res_b, a, b, 1, 2)

    def s16_a():
        mod.fhe_uint_splice_batched(ptr(res_a), ptr(a), ptr(b), W, 16, 1, 0, sh.gals, sh.atk, p, tmp.ptr, tmp.nbytes, batch)

    def s16_b():
        splice8_b(t[4], a, b, 2, 0)
        splice8_b(res_b, t[4], b, 3, 1)

    def sext_a():
        restore()
        mod.fhe_uint_sext_batched(ptr(word), W, 0, sh.gals, sh.atk, p, tmp.ptr, tmp.nbytes, batch)
        ew("pz_vec_znx_copy_batched", res_a, word)

    def sext_b():
        restore()
        rot(-c(7), t[4], word)
        trace(t[4], 0)
        for i in range(3):
            rot((n // 8) << i, t[5], t[4])
            ew("pz_vec_znx_add_assign_batched", t[4], t[5])
        for i in range(1, W // 8):
            splice8_b(res_b, word, t[4], i, 0)
            ew("pz_vec_znx_copy_batched", word, res_b)

    cp = None
    for name, leg_a, leg_b, out_a, out_b, traces in (("get_bits", get_a, get_b, bits_a, bits_b, "32 -> 1"), ("splice_u8", s8_a, s8_b, res_a, res_b, "2 -> 1"),
                                                     ("splice_u16", s16_a, s16_b, res_a, res_b, "4 -> 2"), ("sext0", sext_a, sext_b, res_a, res_b, "7 -> 4")):
        mod.dispatch_notes(reset=True)
        for leg in (leg_a, leg_b):
            for _ in range(args.warmup):
                leg()
        mod.sync()
        notes = mod.dispatch_notes()     # (from the warm-up: a replayed graph leaves none)
        same = bool(torch.equal(out_a, out_b))
        ra, rb, ra2 = [], [], []
        for _ in range(args.rounds):
            ra.append(timed(mod, leg_a, args.window))
            rb.append(timed(mod, leg_b, args.window))
            ra2.append(timed(mod, leg_a, args.window))
        ma, mb, ma2 = (statistics.median(x) for x in (ra, rb, ra2))
        spread = abs(ma - ma2) / ma
        line = {"metric": "u32 FheUint words / s through %s (the new call)" % name, "unit": "words/s", "value": ma * batch, "operation": name,
                "new_per_s": [x * batch for x in ra], "old_entry_points_per_s": [x * batch for x in rb], "again_new_per_s": [x * batch for x in ra2],
                "new_over_old": ma / mb, "spread_same_leg": spread, "not_slower_beyond_spread": bool(ma >= mb * (1.0 - spread)),
                "legs_bit_identical": same, "traces_old_to_new": traces}
        if name == "sext0":   # both legs carry copies the operation does not have: the restoring one (A also one into res_a)
            cp = statistics.median([timed(mod, restore, args.window) for _ in range(args.rounds)])
            line.update({"restore_copies_per_s": cp, "new_over_old_one_copy_subtracted": without(ma, cp) / without(mb, cp),
                         "new_per_s_two_copies_subtracted": without(without(ma, cp), cp) * batch})
        line.update({"graph_launches": mod.graph_launches(),
                     "config": {"n": n, "rank": 1, "base2k": K, "batch": batch, "word_bits": W, "limbs": GGSW_SIZE, "rounds": args.rounds, "window_s": args.window},
                     "dispatch_notes": notes})
        print(json.dumps(line), flush=True)
        if not same:
            raise SystemExit(3)   # a fast wrong answer is not a result
    tmp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024,2048", help="ring degrees, comma separated")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gpus", type=int, default=1)
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_fhe_uint_bytes.py measures one device (--gpus 1)")
    for n in (int(x) for x in args.shapes.split(",")):
        sh = Shape(n)
        for batch in (int(x) for x in args.batches.split(",")):
            bench(sh, batch, args)
        sh.mod.close()


if __name__ == "__main__":
    main()
