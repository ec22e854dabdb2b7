"""Helpers on top of the gate entry points (pz_glwe_cmux_batched, pz_glwe_cswap_batched) for poulpy-bin-fhe's bdd_arithmetic, and the BDD
circuits of its evaluator (ExecuteBDDCircuit, eval.rs:104-305): construction (from_truth_table, adder, ...), evaluation on clear bits
(eval_plain) and on the device (execute_bdd_circuit -> pz_bdd_circuit_execute_batched)."""
from __future__ import annotations

from ctypes import c_void_p
from functools import lru_cache


def _addr(p) -> int:
    return p.value if isinstance(p, c_void_p) else int(p)


def glwe_blind_selection(mod, buf, bit_ptrs, params, batch: int) -> c_void_p:
    """GLWEBlindSelection::glwe_blind_selection (bdd_arithmetic/blind_selection.rs:41-104) on `batch` independent maps.

    buf: device pointer to a dense slot-major buffer [2^bit_mask slots][batch] of GLWE ciphertexts (one layout: params.a_size ==
    params.res_size limbs), slot s holding entry s of every map; an absent entry is a zero ciphertext (:75-76, :82-83).  bit_ptrs[i]: the
    prepared GGSW of bit bit_rsh + i (device pointers), bit_mask = len(bit_ptrs).  The buffer is CLOBBERED, as the reference's entries are.

    Level i (bit bit_rsh + bit_mask - 1 - i, :62) pairs entry j with entry j + t, t = 2^(bit_mask - 1 - i), by cmux_assign(lo = a[j + t],
    hi = a[j]) (:70): with the live entries kept in the LAST 2t slots that is ONE call - f = the first t of them, res = t = the last t, on
    t * batch ciphertexts - and the survivors are the last t slots.  Returns the device pointer of the result: the last slot."""
    assert params.a_size == params.res_size
    bit_mask = len(bit_ptrs)
    slots = 1 << bit_mask
    size = int(params.res_size)
    slot_bytes = batch * mod.n() * (int(params.rank) + 1) * size * 8
    base = _addr(buf)
    for i in range(bit_mask):
        t = 1 << (bit_mask - 1 - i)
        lo = c_void_p(base + (slots - t) * slot_bytes)
        hi = c_void_p(base + (slots - 2 * t) * slot_bytes)
        mod.glwe_cmux_batched(lo, lo, hi, bit_ptrs[bit_mask - 1 - i], params, t * batch, t_size=size, f_size=size)
    return c_void_p(base + (slots - 1) * slot_bytes)


def glwe_blind_retrieval(mod, buf, nslots: int, bit_ptrs, params, batch: int, reverse: bool = False) -> c_void_p:
    """GLWEBlindRetrieval::glwe_blind_retrieval_statefull / _rev (bdd_arithmetic/blind_retrieval.rs:195-266) on `batch` independent vectors.

    buf: device pointer to a dense slot-major buffer [nslots][batch] of GLWE ciphertexts (one layout: params.a_size == params.res_size limbs),
    slot s holding element s of every vector.  bit_ptrs[i]: the prepared GGSW of bit bit_rsh + i (device pointers), bit_mask = len(bit_ptrs).
    The buffer is permuted IN PLACE, as the reference's Vec is: afterwards slot 0 holds the element at the encrypted index; reverse=True applies
    the same network backwards and restores the order.

    Level i (bit bit_rsh + bit_mask - 1 - i, :222-223) pairs element j with element j + t, t = 2^(bit_mask - 1 - i), for every j < t with
    j + t < nslots (:224-230): one conditional swap on min(t, nslots - t) * batch contiguous pairs.  All levels are ONE call of
    pz_glwe_blind_retrieval_batched.  Returns the device pointer of slot 0."""
    assert params.a_size == params.res_size
    mod.glwe_blind_retrieval_batched(buf, nslots, bit_ptrs, reverse, params, batch)
    return c_void_p(_addr(buf))


# ------------------------------------------------------------------------------------------------------------------------------------------
# BDD circuits in the evaluator's node format (eval.rs:241-332).  One node list per output bit, in chunks of state_size nodes, one chunk per
# level, evaluated from the terminals up: the state starts as slot 0 = zero, slot 1 = one; Cmux(sel, hi, lo) at position j of a chunk writes
# next[j] = bit[sel] ? prev[hi] : prev[lo], Copy carries prev[j] over, NONE leaves next[j] as it was; the last chunk is [Cmux, NONE, ...] and
# its gate is the output.  A node is the tuple (kind, sel, hi, lo).
# ------------------------------------------------------------------------------------------------------------------------------------------
NONE, COPY, CMUX = 0, 1, 2
_NONE_NODE, _COPY_NODE = (NONE, 0, 0, 0), (COPY, 0, 0, 0)


class Circuit:
    """GetBitCircuitInfo: input_size, and per output bit (nodes, state_size) - `outputs[o]`; state_size 0 (no nodes): a zero output."""

    def __init__(self, input_size: int, outputs):
        self.input_size = int(input_size)
        self.outputs = [([tuple(int(x) for x in nd) for nd in nodes], int(s)) for nodes, s in outputs]

    @property
    def output_size(self) -> int:
        return len(self.outputs)

    @property
    def max_state_size(self) -> int:
        return max((s for _, s in self.outputs), default=0)

    def depth(self, o: int) -> int:
        nodes, s = self.outputs[o]
        return len(nodes) // s if s else 0

    @property
    def max_depth(self) -> int:
        return max((self.depth(o) for o in range(self.output_size)), default=0)

    def count(self, kind: int) -> int:
        return sum(1 for nodes, _ in self.outputs for nd in nodes if nd[0] == kind)


def eval_plain(circuit: Circuit, input_bits) -> list:
    """The walk of eval_level on clear bits: two banks of state_size values, a NONE slot keeps what its bank held; -> one bit per output."""
    out = []
    for nodes, s in circuit.outputs:
        if s == 0:
            out.append(0)
            continue
        assert len(nodes) % s == 0 and len(nodes) >= s
        level = [0] * (2 * s)
        level[1] = 1
        prev, nxt = 0, s
        for c in range(0, len(nodes) - s, s):
            for j in range(s):
                kind, sel, hi, lo = nodes[c + j]
                if kind == CMUX:
                    level[nxt + j] = level[prev + hi] if input_bits[sel] else level[prev + lo]
                elif kind == COPY:
                    level[nxt + j] = level[prev + j]
            prev, nxt = nxt, prev
        kind, sel, hi, lo = nodes[len(nodes) - s]
        assert kind == CMUX, "invalid last node, should be CMUX"
        out.append(level[prev + hi] if input_bits[sel] else level[prev + lo])
    return out


class _Bdd:
    """A reduced ordered BDD under construction: ids 0 / 1 are the terminals, node id -> (position in the order, lo, hi)."""

    def __init__(self):
        self.nodes, self.unique = {}, {}

    def mk(self, pos: int, lo: int, hi: int) -> int:
        if lo == hi:
            return lo
        key = (pos, lo, hi)
        if key not in self.unique:
            self.unique[key] = len(self.nodes) + 2
            self.nodes[self.unique[key]] = key
        return self.unique[key]


def _layout(bdd: _Bdd, root: int, sel_of_pos, const_sel: int = 0):
    """One output bit's BDD -> (nodes, state_size).  The levels are the order positions that carry a node of this output, the deepest first;
    a value keeps ONE position from the level that makes it to the last level that reads it (Copy in between - it cannot move), positions
    0 and 1 start as the terminals and are handed out again once those are no longer read."""
    if root == 0:
        return [], 0
    if root == 1:   # the constant one: a gate choosing between one and one
        return [(CMUX, const_sel, 1, 1), _NONE_NODE], 2
    reach, stack = set(), [root]
    while stack:
        v = stack.pop()
        if v < 2 or v in reach:
            continue
        reach.add(v)
        stack += [bdd.nodes[v][1], bdd.nodes[v][2]]
    positions = sorted({bdd.nodes[v][0] for v in reach}, reverse=True)
    level_of = {p: i for i, p in enumerate(positions)}
    nlev = len(positions)
    made = {0: -1, 1: -1}
    last = {}
    for v in reach:
        lv = level_of[bdd.nodes[v][0]]
        made[v] = lv
        for src in bdd.nodes[v][1:]:
            last[src] = max(last.get(src, -1), lv)
    by_level = [[] for _ in range(nlev)]
    for v in sorted(reach):
        by_level[made[v]].append(v)
    pos = {0: 0, 1: 1}
    free_from = [last.get(0, -1) + 1, last.get(1, -1) + 1]   # the first level whose `prev` no longer needs the position
    for lv in range(nlev - 1):
        for v in by_level[lv]:
            p = next((i for i, f in enumerate(free_from) if f <= lv + 1), len(free_from))
            if p == len(free_from):
                free_from.append(0)
            free_from[p] = last[v] + 1
            pos[v] = p
    s = len(free_from)
    nodes = []
    for lv in range(nlev - 1):
        chunk = [_NONE_NODE] * s
        for v, p in pos.items():
            if v != root and made[v] < lv and last.get(v, -1) > lv:
                chunk[p] = _COPY_NODE
        for v in by_level[lv]:
            vp, lo, hi = bdd.nodes[v]
            assert chunk[pos[v]] == _NONE_NODE
            chunk[pos[v]] = (CMUX, sel_of_pos(vp), pos[hi], pos[lo])
        nodes += chunk
    assert by_level[nlev - 1] == [root]
    vp, lo, hi = bdd.nodes[root]
    nodes += [(CMUX, sel_of_pos(vp), pos[hi], pos[lo])] + [_NONE_NODE] * (s - 1)
    return nodes, s


def from_truth_table(fn, n_in: int, n_out: int, order=None) -> Circuit:
    """fn: the n_in-bit input as an integer (input bit i = bit i) -> the n_out-bit output.  One reduced ordered BDD per output bit by Shannon
    expansion over `order` (order[0] is tested at the root, i.e. evaluated LAST; default 0, 1, ...).  Exponential in n_in: small widths."""
    order = list(range(n_in)) if order is None else [int(x) for x in order]
    assert sorted(order) == list(range(n_in))
    values = []
    for idx in range(1 << n_in):   # idx: the assignment with order[0] as its most significant bit
        x = 0
        for k, var in enumerate(order):
            x |= ((idx >> (n_in - 1 - k)) & 1) << var
        values.append(int(fn(x)))
    outputs = []
    for o in range(n_out):
        table = tuple((v >> o) & 1 for v in values)
        bdd, memo = _Bdd(), {}

        def build(k, sub):
            if not any(sub):
                return 0
            if all(sub):
                return 1
            if (k, sub) not in memo:
                half = len(sub) // 2
                memo[(k, sub)] = bdd.mk(k, build(k + 1, sub[:half]), build(k + 1, sub[half:]))
            return memo[(k, sub)]
        outputs.append(_layout(bdd, build(0, table), lambda p: order[p], order[0] if order else 0))
    return Circuit(n_in, outputs)


def _ripple(w: int, n_out: int, carry, out_bit, last_is_carry: bool) -> Circuit:
    """Bit-serial circuits on two w-bit words a (input bits 0 .. w-1) and b (w .. 2w-1), built from the root over the order a_0, b_0, a_1, b_1,
    ...: the BDD of output bit i walks the bits j = 0 .. i with the carry as its only state - at a_j one node per carry, at b_j one per
    (carry, a_j) - and ends in out_bit(c, a_i, b_i); carry(c, a, b) is the next carry.  last_is_carry: output n_out - 1 is the carry out
    of bit w - 1 instead.  The unique table merges what the carry does not tell apart, so the state is 3 wide at most."""
    outputs = []
    for i in range(n_out):
        as_carry = last_is_carry and i == n_out - 1
        top = w - 1 if as_carry else i
        bdd = _Bdd()

        @lru_cache(maxsize=None)
        def at_a(j, c):
            return bdd.mk(2 * j, at_b(j, c, 0), at_b(j, c, 1))

        @lru_cache(maxsize=None)
        def at_b(j, c, a):
            return bdd.mk(2 * j + 1, after(j, c, a, 0), after(j, c, a, 1))

        def after(j, c, a, b):
            if j == top:
                return int(carry(c, a, b) if as_carry else out_bit(c, a, b))
            return at_a(j + 1, int(carry(c, a, b)))
        outputs.append(_layout(bdd, at_a(0, 0), lambda p: (p >> 1) + (w if p & 1 else 0)))
    return Circuit(2 * w, outputs)


def adder(w: int, carry_out: bool = False) -> Circuit:
    """a + b mod 2^w (with carry_out: w + 1 output bits)."""
    return _ripple(w, w + (1 if carry_out else 0), lambda c, a, b: (a + b + c) >> 1, lambda c, a, b: a ^ b ^ c, carry_out)


def sub(w: int) -> Circuit:
    """a - b mod 2^w; the state is the borrow."""
    return _ripple(w, w, lambda c, a, b: int(a - b - c < 0), lambda c, a, b: a ^ b ^ c, False)


def xor(w: int) -> Circuit:
    return _ripple(w, w, lambda c, a, b: 0, lambda c, a, b: a ^ b, False)


def ltu(w: int) -> Circuit:
    """One output bit: a < b (unsigned) - the borrow out of a - b."""
    return _ripple(w, 1, lambda c, a, b: int(a - b - c < 0), lambda c, a, b: 0, True)


def word_bits(a: int, b: int, w: int) -> list:
    """The input bits of the two-word circuits above: a in bits 0 .. w-1, b in bits w .. 2w-1."""
    return [(a >> i) & 1 for i in range(w)] + [(b >> i) & 1 for i in range(w)]


def execute_bdd_circuit(mod, circuit, out, bits, params, batch: int, tmp=None):
    """ExecuteBDDCircuit::execute_bdd_circuit (eval.rs:123-239) on `batch` independent inputs: pz_bdd_circuit_execute_batched.

    circuit: a compiled handle of mod.bdd_circuit_new (a Circuit is compiled, and freed, around the call).  out: (device pointer, n_out) - a dense
    slot-major buffer [n_out][batch] of GLWEs of params.res_size limbs, n_out >= output_size; slots beyond output_size are zeroed.  bits[b][i]: the
    prepared GGSW of input bit i of input b (device pointer, pinned or not; None where the circuit never selects it).  tmp: a DeviceBuffer of at
    least mod.bdd_circuit_execute_tmp_bytes(...) bytes; allocated and freed here when absent (the call is synchronized then)."""
    handle = circuit
    own = isinstance(circuit, Circuit)
    if own:
        handle = mod.bdd_circuit_new(circuit)
    try:
        out_ptr, n_out = out
        need = mod.bdd_circuit_execute_tmp_bytes(handle, params, batch)
        buf = tmp if tmp is not None else (mod.device_alloc(max(need, 8)))
        try:
            mod.bdd_circuit_execute_batched(handle, out_ptr, n_out, bits, params, buf.ptr, buf.nbytes, batch)
            if tmp is None:
                mod.sync()
        finally:
            if tmp is None:
                buf.free()
    finally:
        if own:
            mod.bdd_circuit_free(handle)


# ------------------------------------------------------------------------------------------------------------------------------------------
# FheUint words (bdd_arithmetic/ciphertexts/fhe_uint.rs): one GLWE per integer, bit i at coefficient bit_index(i) << log_gap.  A word becomes
# the evaluator's selectors through fhe_uint_prepare (pz_fhe_uint_prepare_batched), the evaluator's output a word again through fhe_uint_pack.
# ------------------------------------------------------------------------------------------------------------------------------------------
def bit_index(i: int, word_bits: int) -> int:
    """bdd_arithmetic/mod.rs:97-99: the bytes of a word are interleaved - bit i of the integer lies at ((i & 7) << LOG_BYTES) | (i >> 3)."""
    assert word_bits in (8, 16, 32, 64, 128) and 0 <= i < word_bits
    log_bytes = (word_bits // 8).bit_length() - 1
    return ((i & 7) << log_bytes) | (i >> 3)


def fhe_uint_prepare(mod, res_pmat, words, key, params, batch: int, tmp=None, ggsw_out=None, lwe_out=None) -> list:
    """FheUintPrepared::prepare (fhe_uint_prepared.rs:399-460) on `batch` words: pz_fhe_uint_prepare_batched.

    res_pmat: device pointer to batch * word_bits prepared GGSWs (word-major).  words: device pointer to the batch GLWEs.  key: an object with
    the device pointers ks_glwe (or None), ks_lwe, lut, brk, the list gals and the pointer lists atk, tsk.  params: FheUintPrepareParams.
    tmp: a DeviceBuffer of at least mod.fhe_uint_prepare_tmp_bytes(params, batch, chunk) bytes for some chunk >= 1; allocated for the whole
    batch, and freed, here when absent (the call is synchronized then).
    Returns bits[b][i], the device address of the prepared GGSW of bit i of word b: the table execute_bdd_circuit takes; the rows of two
    words concatenate to the 2 w inputs of adder / sub / ltu."""
    need = mod.fhe_uint_prepare_tmp_bytes(params, batch)
    buf = tmp if tmp is not None else mod.device_alloc(max(need, 8))
    try:
        mod.fhe_uint_prepare_batched(res_pmat, words, key.ks_glwe, key.ks_lwe, key.lut, key.brk, key.gals, key.atk, key.tsk, params, buf.ptr,
                                     buf.nbytes, batch, ggsw_out=ggsw_out, lwe_out=lwe_out)
        if tmp is None:
            mod.sync()
    finally:
        if tmp is None:
            buf.free()
    cols = int(params.cbt.br.rank) + 1
    ggsw_bytes = int(params.cbt.res_dnum) * cols * cols * int(params.cbt.res_size) * mod.n() * 8
    w = int(params.word_bits)
    base = _addr(res_pmat)
    return [[base + (b * w + i) * ggsw_bytes for i in range(w)] for b in range(batch)]


def fhe_uint_pack(mod, res, out, word_bits: int, gals, key_ptrs, params, batch: int, tmp=None, index=bit_index):
    """FheUint::pack (fhe_uint.rs:239-255) on `batch` words through pz_glwe_pack_batched: out = the evaluator's dense slot-major buffer
    [word_bits][batch] (slot s = bit s of every word; CLOBBERED), res = device pointer to the batch packed words.  gals / key_ptrs: the
    log2(n) trace steps (-1, then 5^(2^(i-1))) and their prepared automorphism keys; params: a_size = res_size = the limbs of the GLWEs.
    index (tests: a negative control) maps a bit to its slot of the word."""
    n = mod.n()
    assert n % word_bits == 0 and params.a_size == params.res_size
    log_gap = (n // word_bits).bit_length() - 1
    ct_bytes = batch * n * (int(params.rank) + 1) * int(params.res_size) * 8
    base = _addr(out)
    cts = [c_void_p(base + s * ct_bytes) for s in range(word_bits)]
    indices = [index(s, word_bits) << log_gap for s in range(word_bits)]
    need = mod.glwe_pack_tmp_bytes(params, batch)
    buf = tmp if tmp is not None else mod.device_alloc(max(need, 8))
    try:
        mod.glwe_pack_batched(res, indices, cts, log_gap, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch)
        if tmp is None:
            mod.sync()
    finally:
        if tmp is None:
            buf.free()


def fhe_uint_pack_words(mod, res, out, word_bits: int, gals, key_ptrs, params, batch: int, tmp=None, trace_size: int = 0):
    """FheUint::pack (fhe_uint.rs:239-255) on `batch` words through pz_fhe_uint_pack_batched, level by level: the arguments of fhe_uint_pack
    (out = the evaluator's dense slot-major buffer [word_bits][batch], CLOBBERED; res = the batch packed words), bit-identical to it.
    trace_size >= 1: the automorphism keys have their own base2k (as for glwe_pack_bases_batched)."""
    need = mod.fhe_uint_pack_tmp_bytes(params, word_bits, batch, trace_size)
    buf = tmp if tmp is not None else mod.device_alloc(max(need, 8))
    try:
        mod.fhe_uint_pack_batched(res, out, word_bits, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch, trace_size)
        if tmp is None:
            mod.sync()
    finally:
        if tmp is None:
            buf.free()


def fhe_uint_execute(mod, circuit, res, word_bits: int, bits, gate, gals, key_ptrs, pack, batch: int, tmp=None, trace_size: int = 0):
    """execute_bdd_circuit_2w_to_1w / _1w_to_1w (bdd_2w_to_1w.rs:103-136, bdd_1w_to_1w.rs:46-70) on `batch` inputs: pz_fhe_uint_execute_batched.

    circuit: a compiled handle of mod.bdd_circuit_new (a Circuit is compiled, and freed, around the call), output_size <= word_bits.  res: device
    pointer to the batch packed words.  bits[b][i]: the prepared GGSW of input bit i of input b - the rows of the one or two prepared words of
    fhe_uint_prepare, concatenated.  gate: the evaluator's params; gals / key_ptrs / pack: the arguments of fhe_uint_pack_words.  tmp: a
    DeviceBuffer of at least mod.fhe_uint_execute_tmp_bytes(...) bytes; allocated and freed here when absent (the call is synchronized then)."""
    handle = circuit
    own = isinstance(circuit, Circuit)
    if own:
        handle = mod.bdd_circuit_new(circuit)
    try:
        need = mod.fhe_uint_execute_tmp_bytes(handle, gate, pack, word_bits, batch, trace_size)
        buf = tmp if tmp is not None else mod.device_alloc(max(need, 8))
        try:
            mod.fhe_uint_execute_batched(handle, res, word_bits, bits, gate, gals, key_ptrs, pack, buf.ptr, buf.nbytes, batch, trace_size)
            if tmp is None:
                mod.sync()
        finally:
            if tmp is None:
                buf.free()
    finally:
        if own:
            mod.bdd_circuit_free(handle)


def _with_word_tmp(mod, params, word_bits, batch, max_items, tmp, call):
    need = mod.fhe_uint_word_op_tmp_bytes(params, word_bits, batch, max_items)
    buf = tmp if tmp is not None else mod.device_alloc(max(need, 8))
    try:
        call(buf)
        if tmp is None:
            mod.sync()
    finally:
        if tmp is None:
            buf.free()


def fhe_uint_get_bits(mod, res, words, word_bits: int, bits, gals, key_ptrs, params, batch: int, tmp=None):
    """FheUint::get_bit_glwe (fhe_uint.rs:401-414) of `batch` words at every bit of `bits`: res = device pointer to [len(bits)][batch] GLWEs,
    bit-major - with bits = range(word_bits) the inverse of fhe_uint_pack_words.  gals / key_ptrs: all log2(n) trace steps; tmp: a
    DeviceBuffer of at least mod.fhe_uint_word_op_tmp_bytes(...) bytes, allocated and freed here when absent (the call is synchronized then)."""
    from .abi import PZ_WORD_BIT
    _with_word_tmp(mod, params, word_bits, batch, len(bits), tmp,
                   lambda buf: mod.fhe_uint_get_batched(res, words, word_bits, PZ_WORD_BIT, bits, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch))


def fhe_uint_get_bytes(mod, res, words, word_bits: int, byte_indices, gals, key_ptrs, params, batch: int, tmp=None):
    """FheUint::get_byte (fhe_uint.rs:416-430): as fhe_uint_get_bits, the byte at coefficient 0 .. of every result and nothing else."""
    from .abi import PZ_WORD_BYTE
    _with_word_tmp(mod, params, word_bits, batch, len(byte_indices), tmp,
                   lambda buf: mod.fhe_uint_get_batched(res, words, word_bits, PZ_WORD_BYTE, byte_indices, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch))


def fhe_uint_zero_byte(mod, res, a, word_bits: int, byte: int, gals, key_ptrs, params, batch: int, tmp=None):
    """FheUint::zero_byte (fhe_uint.rs:466-489) on `batch` words: res = a with byte `byte` zeroed (res may be a)."""
    _with_word_tmp(mod, params, word_bits, batch, 1, tmp,
                   lambda buf: mod.fhe_uint_zero_byte_batched(res, a, word_bits, byte, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch))


def fhe_uint_splice(mod, res, a, b, word_bits: int, width: int, dst: int, src: int, gals, key_ptrs, params, batch: int, tmp=None):
    """FheUint::splice_u8 / splice_u16 (fhe_uint.rs:259-329; width 8 / 16) on `batch` words: res = a with byte (half-word) dst replaced by
    byte (half-word) src of b; res may be a or b."""
    _with_word_tmp(mod, params, word_bits, batch, 3, tmp,
                   lambda buf: mod.fhe_uint_splice_batched(res, a, b, word_bits, width, dst, src, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch))


def fhe_uint_sext(mod, word, word_bits: int, byte: int, gals, key_ptrs, params, batch: int, tmp=None):
    """FheUint::sext (fhe_uint.rs:491-524) on `batch` words, in place: the bytes above `byte` become copies of its sign bit."""
    _with_word_tmp(mod, params, word_bits, batch, 2, tmp,
                   lambda buf: mod.fhe_uint_sext_batched(word, word_bits, byte, gals, key_ptrs, params, buf.ptr, buf.nbytes, batch))
