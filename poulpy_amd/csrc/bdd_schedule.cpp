// bdd_schedule.cpp — see bdd_schedule.hpp.  The compiler walks every output's node list the way eval_level does (two banks of state_size positions,
// all zero but position 1, swapped after every level, a None position keeping what its bank held), but on VALUE NAMES instead of ciphertexts: the two
// constants, and one fresh name per Cmux.  A Copy hands the name of prev[j] to next[j] and nothing else - a copy is exact, so whoever reads next[j]
// later may as well read the value where it already is.  What is left is a list of gates (level, t, f, selector) over names; a name gets a physical
// slot from the level that makes it to the last level that reads it.
#include "bdd_schedule.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

namespace pz {
namespace {

bool bad(std::string* err, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return false;
}

struct NamedGate { uint32_t level, t, f, sel; };   // t, f: value names; the gate's own name is 2 + its index

}  // namespace

bool bdd_compile(const BddNode* const* nodes, const size_t* node_count, const size_t* state_size, size_t output_size, size_t input_size,
                 BddSchedule* out, std::string* err) {
    if (!out) return bad(err, "bdd_circuit_new: null result");
    if (output_size && (!nodes || !node_count || !state_size)) return bad(err, "bdd_circuit_new: null argument");
    if (output_size >= kBddOut || input_size >= kBddOut) return bad(err, "bdd_circuit_new: more than 2^31 outputs or inputs");
    BddSchedule s;
    s.input_size = input_size; s.output_size = output_size;
    s.selected.assign(input_size, 0);
    s.slot_first.assign(output_size, 0); s.slot_count.assign(output_size, 0); s.state_size.assign(output_size, 0);
    std::vector<std::vector<BddGate>> by_level;
    for (size_t o = 0; o < output_size; ++o) {
        const size_t S = state_size[o], cnt = node_count[o];
        s.slot_first[o] = (uint32_t)s.slots;
        if (S == 0) {
            if (cnt != 0) return bad(err, "bdd_circuit_new: output %zu has state_size 0 and %zu nodes (node 0): a zero output has none", o, cnt);
            s.zero_outputs.push_back((uint32_t)o);
            continue;
        }
        if (S >= (1u << 30)) return bad(err, "bdd_circuit_new: output %zu: state_size %zu", o, S);
        s.state_size[o] = (uint32_t)S;
        s.max_state_size = std::max(s.max_state_size, S);
        if (cnt == 0 || cnt % S != 0)
            return bad(err, "bdd_circuit_new: output %zu: %zu nodes are not whole chunks of state_size %zu (node %zu starts a ragged chunk)", o, cnt, S, cnt - cnt % S);
        const BddNode* nd = nodes[o];
        if (!nd) return bad(err, "bdd_circuit_new: output %zu: null node list", o);
        const size_t depth = cnt / S;
        if (depth >= (1u << 30)) return bad(err, "bdd_circuit_new: output %zu: %zu levels", o, depth);
        for (size_t i = 0; i < cnt; ++i) {
            const BddNode& x = nd[i];
            if (x.kind > kBddCmux) return bad(err, "bdd_circuit_new: output %zu node %zu: unknown kind %u", o, i, x.kind);
            if (x.kind != kBddCmux) continue;
            if (x.hi >= S) return bad(err, "bdd_circuit_new: output %zu node %zu: hi index %u >= state_size %zu", o, i, x.hi, S);
            if (x.lo >= S) return bad(err, "bdd_circuit_new: output %zu node %zu: lo index %u >= state_size %zu", o, i, x.lo, S);
            if (x.sel >= input_size) return bad(err, "bdd_circuit_new: output %zu node %zu: selector %u >= input_size %zu", o, i, x.sel, input_size);
        }
        if (nd[cnt - S].kind != kBddCmux) return bad(err, "bdd_circuit_new: output %zu node %zu: the last chunk must start with a cmux", o, cnt - S);
        for (size_t i = cnt - S + 1; i < cnt; ++i)
            if (nd[i].kind != kBddNone) return bad(err, "bdd_circuit_new: output %zu node %zu: the last chunk is [cmux, none, ...]", o, i);
        // ---- the walk on names (eval.rs:257-299) ----
        std::vector<uint32_t> bank(2 * S, 0u);
        bank[1] = 1u;   // slot 1 of the 2 S (S = 1: that is the SECOND bank's only position)
        std::vector<NamedGate> g;
        size_t prev = 0, next = S;
        for (size_t lv = 0; lv + 1 < depth; ++lv) {
            for (size_t j = 0; j < S; ++j) {
                const BddNode& x = nd[lv * S + j];
                if (x.kind == kBddCmux) {
                    g.push_back({(uint32_t)lv, bank[prev + x.hi], bank[prev + x.lo], x.sel});
                    bank[next + j] = (uint32_t)(g.size() + 1);   // = 2 + index
                } else if (x.kind == kBddCopy) {
                    bank[next + j] = bank[prev + j];
                    s.copies++;
                }
            }
            std::swap(prev, next);
        }
        const BddNode& root = nd[cnt - S];
        g.push_back({(uint32_t)(depth - 1), bank[prev + root.hi], bank[prev + root.lo], root.sel});
        if (g.size() + 2 >= kBddOut) return bad(err, "bdd_circuit_new: output %zu: too many gates", o);
        // ---- slots: a name holds one from its own level to the last level that reads it; a slot given back after level l is handed out from
        //      level l + 1 on, so no gate of a level writes what a gate of that level reads (or writes) ----
        const size_t nv = g.size() + 2;
        std::vector<int64_t> last(nv, -1);
        for (const NamedGate& x : g) { last[x.t] = std::max<int64_t>(last[x.t], x.level); last[x.f] = std::max<int64_t>(last[x.f], x.level); }
        std::vector<uint32_t> slot(nv, 0u);
        slot[1] = kBddSlotOne;
        std::vector<std::vector<uint32_t>> dies(depth);   // names whose slot is given back after that level
        std::vector<uint32_t> free_slots, pending;
        uint32_t used = 0;
        size_t k = 0;
        for (size_t lv = 0; lv < depth; ++lv) {
            free_slots.insert(free_slots.end(), pending.begin(), pending.end());
            pending.clear();
            for (; k + 1 < g.size() && g[k].level == lv; ++k) {   // (the root, g.back(), writes the output)
                const uint32_t name = (uint32_t)(k + 2);
                uint32_t sl;
                if (!free_slots.empty()) { sl = free_slots.back(); free_slots.pop_back(); }
                else sl = used++;
                slot[name] = (uint32_t)s.slots + sl;
                dies[(size_t)std::max<int64_t>(last[name], (int64_t)lv)].push_back(name);
            }
            for (uint32_t name : dies[lv]) pending.push_back(slot[name] - (uint32_t)s.slots);
        }
        if (used > 2 * S) return bad(err, "bdd_circuit_new: output %zu: %u live values in a state of 2 x %zu (internal error)", o, used, S);
        if (s.slots + used >= kBddOut) return bad(err, "bdd_circuit_new: more than 2^31 slots");
        s.slot_count[o] = used;
        s.slots += used;
        if (by_level.size() < depth) by_level.resize(depth);
        for (size_t i = 0; i < g.size(); ++i) {
            const bool is_root = i + 1 == g.size();
            by_level[g[i].level].push_back({slot[g[i].t], slot[g[i].f], is_root ? (kBddOut | (uint32_t)o) : slot[i + 2], g[i].sel});
            s.selected[g[i].sel] = 1;
        }
    }
    s.level_start.push_back(0);
    for (auto& lv : by_level) {
        std::stable_sort(lv.begin(), lv.end(), [](const BddGate& a, const BddGate& b) { return a.sel < b.sel; });
        s.gates.insert(s.gates.end(), lv.begin(), lv.end());
        if (s.gates.size() >= 0xFFFFFFFFull) return bad(err, "bdd_circuit_new: more than 2^32 gates");
        s.level_start.push_back((uint32_t)s.gates.size());
    }
    if (!bdd_check(s, err)) return false;
    *out = std::move(s);
    return true;
}

bool bdd_check(const BddSchedule& s, std::string* err) {
    const size_t nl = s.levels();
    if (s.level_start.empty() || s.level_start[0] != 0 || s.level_start[nl] != s.gates.size()) return bad(err, "bdd schedule: level offsets do not cover the gates");
    if (s.slot_first.size() != s.output_size || s.slot_count.size() != s.output_size || s.state_size.size() != s.output_size || s.selected.size() != s.input_size)
        return bad(err, "bdd schedule: per-output / per-input tables of the wrong length");
    size_t at = 2;
    for (size_t o = 0; o < s.output_size; ++o) {
        if (s.slot_first[o] != at) return bad(err, "bdd schedule: output %zu: slot range out of order", o);
        if (s.slot_count[o] > 2 * (size_t)s.state_size[o]) return bad(err, "bdd schedule: output %zu: %u slots for a state of %u", o, s.slot_count[o], s.state_size[o]);
        at += s.slot_count[o];
    }
    if (at != s.slots) return bad(err, "bdd schedule: the slot ranges do not add up");
    // the output a slot belongs to (slots 0 / 1: everybody's)
    auto owner = [&](uint32_t sl) -> size_t {
        size_t lo = 0, hi = s.output_size;   // last o with slot_first[o] <= sl
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; (s.slot_first[mid] <= sl ? lo : hi) = mid; }
        return lo;
    };
    std::vector<uint8_t> defined(s.slots, 0), written_now(s.slots, 0), written_out(s.output_size, 0);
    defined[kBddSlotZero] = defined[kBddSlotOne] = 1;
    for (uint32_t o : s.zero_outputs) {
        if (o >= s.output_size || written_out[o]) return bad(err, "bdd schedule: zero output %u out of range or listed twice", o);
        written_out[o] = 2;
    }
    for (size_t lv = 0; lv < nl; ++lv) {
        const size_t a = s.level_start[lv], b = s.level_start[lv + 1];
        if (a > b || b > s.gates.size()) return bad(err, "bdd schedule: level %zu: offsets out of order", lv);
        for (size_t i = a; i < b; ++i) {
            const BddGate& g = s.gates[i];
            if (g.sel >= s.input_size || !s.selected[g.sel]) return bad(err, "bdd schedule: level %zu gate %zu: selector %u out of range or not marked", lv, i - a, g.sel);
            if (i > a && s.gates[i - 1].sel > g.sel) return bad(err, "bdd schedule: level %zu gate %zu: not sorted by selector", lv, i - a);
            if (g.t >= s.slots || g.f >= s.slots) return bad(err, "bdd schedule: level %zu gate %zu: source slot out of range", lv, i - a);
            if (!defined[g.t] || !defined[g.f]) return bad(err, "bdd schedule: level %zu gate %zu: reads a slot nothing has written", lv, i - a);
            size_t o;
            if (g.res & kBddOut) {
                o = g.res & ~kBddOut;
                if (o >= s.output_size || written_out[o]) return bad(err, "bdd schedule: level %zu gate %zu: output %zu out of range or written twice", lv, i - a, o);
                written_out[o] = 1;
            } else {
                if (g.res < 2 || g.res >= s.slots) return bad(err, "bdd schedule: level %zu gate %zu: result slot %u out of range", lv, i - a, g.res);
                if (written_now[g.res]) return bad(err, "bdd schedule: level %zu gate %zu: slot %u written twice in one level", lv, i - a, g.res);
                written_now[g.res] = 1;
                o = owner(g.res);
            }
            for (uint32_t src : {g.t, g.f})
                if (src >= 2 && (src < s.slot_first[o] || src >= s.slot_first[o] + s.slot_count[o]))
                    return bad(err, "bdd schedule: level %zu gate %zu: reads slot %u of another output", lv, i - a, src);
        }
        for (size_t i = a; i < b; ++i)   // the aliasing invariant: all gates of a level run concurrently
            if (written_now[s.gates[i].t] || written_now[s.gates[i].f])
                return bad(err, "bdd schedule: level %zu gate %zu: reads a slot a gate of the same level writes", lv, i - a);
        for (size_t i = a; i < b; ++i)
            if (!(s.gates[i].res & kBddOut)) { written_now[s.gates[i].res] = 0; defined[s.gates[i].res] = 1; }
    }
    for (size_t o = 0; o < s.output_size; ++o)
        if (!written_out[o]) return bad(err, "bdd schedule: output %zu is never written", o);
    return true;
}

}  // namespace pz
