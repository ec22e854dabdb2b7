// bdd_schedule.hpp — the host-side compiler of BDD circuits (pz_bdd_circuit_new): poulpy-bin-fhe's node lists
// (bdd_arithmetic/eval.rs:241-332) -> level tables of gates over physical slots.  Plain C++, no HIP: bdd_schedule.cpp links into host-only
// programs (tests/cpp/test_bdd_schedule.cpp), and every index a device table will ever hold is checked here, on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pz {

enum : uint32_t { kBddNone = 0, kBddCopy = 1, kBddCmux = 2 };   // pz_bdd_node::kind
struct BddNode { uint32_t kind, sel, hi, lo; };                  // the layout of pz_bdd_node

// res of a root gate: the output bit it writes, tagged
constexpr uint32_t kBddOut = 0x80000000u;
// the two slots every output shares; nothing ever writes them
constexpr uint32_t kBddSlotZero = 0, kBddSlotOne = 1;

// res = cmux(t = the value `hi` named, f = the value `lo` named, GGSW(sel)); t, f: slots; res: a slot, or kBddOut | output bit
struct BddGate { uint32_t t, f, res, sel; };

struct BddSchedule {
    size_t input_size = 0, output_size = 0, max_state_size = 0;
    std::vector<BddGate> gates;              // level-major; inside a level sorted by selector
    std::vector<uint32_t> level_start;       // levels() + 1 offsets into gates
    std::vector<uint32_t> slot_first, slot_count;   // per output: its range of slots, slot_count <= 2 * state_size
    std::vector<uint32_t> state_size;        // per output, as given
    std::vector<uint32_t> zero_outputs;      // outputs with state_size 0
    std::vector<uint8_t> selected;           // per input bit: some gate selects it
    size_t slots = 2;                        // all of them: the two shared ones and every output's range
    size_t moved_copies = 0;                 // Copy nodes that move data: none - a Copy renames (the value keeps its slot)
    size_t copies = 0;                       // Copy nodes of the circuit
    size_t levels() const { return level_start.empty() ? 0 : level_start.size() - 1; }
};

// Validates and compiles; on a violation returns false and *err names the output bit and the node.
bool bdd_compile(const BddNode* const* nodes, const size_t* node_count, const size_t* state_size, size_t output_size, size_t input_size,
                 BddSchedule* out, std::string* err);
// Re-checks what the device relies on, from the tables alone: every index in range, every output written exactly once by a gate of its own, no gate
// of a level writing a slot that a gate of the same level reads or writes, every slot written before it is read (the two shared ones never written),
// the gates of a level sorted by selector.  false + *err on a violation.
bool bdd_check(const BddSchedule& s, std::string* err);

}  // namespace pz
