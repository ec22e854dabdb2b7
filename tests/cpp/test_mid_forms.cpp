// Host-only check of the middle-kernel dispatch (poulpy_amd/csrc/mid_forms.hpp) and of the block step's (br_forms.hpp, its plain C++ part):
// built with -fsanitize=address,undefined and run as a child process by tests/test_mid_forms_host.py.
//   closure      over every shape launch_mid128 can be handed, the form mid128_form returns has an entry in its list and keeps the kernels'
//                preconditions; the same for br_block_form, whose one form without an entry is (9, 4) without LDS
//   equivalence  argv[1] = tests/golden/mid128_forms.txt, one line per shape: the fields of Mid128Shape, then the dispatch note the selection
//                code BEFORE mid_forms.hpp (five nested macros in launch_mid.hip) produced for it; every note is re-derived and compared as a
//                string, and the file meets every form the sweep meets
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>

#include "../../poulpy_amd/csrc/br_forms.hpp"
#include "../../poulpy_amd/csrc/mid_forms.hpp"

using namespace pz;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 50) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

constexpr int kKR = 6;   // PZ_MIDR_KR of a default build (device_mid.hpp): the golden notes were recorded from one

static std::string note_of(const Mid128Form& f) {
    char buf[160];
    mid128_note(f, kKR, buf, sizeof buf);
    return buf;
}
static int form_key(const Mid128Form& f) {   // every field, packed
    int k = f.ring;
    k = k * 64 + f.ct; k = k * 64 + f.np; k = k * 2 + f.perm; k = k * 2 + f.ds; k = k * 2 + f.br; k = k * 2 + f.skipw;
    k = k * 4 + f.brnest; k = k * 4 + f.nco; k = k * 64 + f.nr; k = k * 2 + f.halfin; k = k * 2 + f.c2;
    return k;
}
static void check_form(const Mid128Shape& s, const Mid128Form& f) {
    CHECK(mid128_form_exists(f), "no entry for %s (npi %d npo %d row_max %d ncols %d)", note_of(f).c_str(), s.npi, s.npo, s.row_max, s.ncols);
    CHECK((f.ct == 8 && f.np == 8) || (f.ct == 4 && f.np == 16) || (f.ct == 2 && f.np == 32), "tile %d x %d", f.ct, f.np);
    CHECK(s.npi <= f.np && (s.npo <= f.np || f.c2), "tile of %d slots for %d in, %d out", f.np, s.npi, s.npo);
    if (f.ring) {
        CHECK(s.mid_r, "k_mid128r with the switch off");
        CHECK(f.nr == f.np || f.nr == f.np / 2, "NR=%d of NP=%d", f.nr, f.np);
        CHECK(!f.halfin || f.np >= 16, "HALFIN with NP=%d", f.np);
        CHECK(!f.halfin || (s.npi <= f.np / 2 && f.nr == f.np / 2), "HALFIN with %d inputs, NR=%d", s.npi, f.nr);
        CHECK(!f.c2 || (s.npi == 16 && s.npo == 32 && f.ct == 4 && f.np == 16 && f.nr == 16), "C2 for %d in, %d out", s.npi, s.npo);
        CHECK((f.ds ? s.ds_n : s.row_max) == f.nr, "NR=%d for %d product terms", f.nr, f.ds ? s.ds_n : s.row_max);
        CHECK(!f.br && !f.skipw && !f.brnest && !f.nco, "k_mid128 fields set on a k_mid128r form");
    } else {
        CHECK(f.nco == 0 || (f.nco == 3 && f.np == 8 && f.brnest == 2), "NCO=%d with NP=%d", f.nco, f.np);
        CHECK(f.brnest == 0 || (f.br && (s.br_rm & 1) == 0), "BRNEST with %d key rows", s.br_rm);
        CHECK(!f.skipw || (f.np > 8 && !f.br && !f.ds), "SKIPW on NP=%d BR=%d DS=%d", f.np, (int)f.br, (int)f.ds);
        CHECK(!f.nr && !f.halfin && !f.c2, "k_mid128r fields set on a k_mid128 form");
    }
    CHECK(f.ds == s.ds && f.br == s.br, "product form DS=%d BR=%d for ds %d br %d", (int)f.ds, (int)f.br, (int)s.ds, (int)s.br);
    CHECK(!f.perm || (s.perm && !s.ds && !s.br), "PERM on ds %d br %d", (int)s.ds, (int)s.br);
}

int main(int argc, char** argv) {
    // ---- closure: npi, npo 1..32; key rows 1..32, of which the choice sees row_max = min(rows, npi), so the loop runs over 1..npi; key columns
    //      1..64; plain | ds_n 1..16 | br_rm 1..12 (the block step's row_max is rows x block size: not read); perm and the switch both ways ----
    unsigned long long shapes = 0;
    std::set<int> swept;
    int last_key = -1;
    auto one = [&](const Mid128Shape& s) {
        const Mid128Form f = mid128_form(s);
        ++shapes;
        check_form(s, f);
        const int k = form_key(f);
        if (k != last_key) { swept.insert(k); last_key = k; }
    };
    for (int npi = 1; npi <= 32; ++npi)
    for (int npo = 1; npo <= 32; ++npo)
    for (int ncols = 1; ncols <= 64; ++ncols)
    for (int sw = 0; sw < 4; ++sw) {
        Mid128Shape s;
        s.npi = npi; s.npo = npo; s.ncols = ncols; s.ncomp = std::min(npo, ncols);
        s.perm = sw & 1; s.mid_r = sw >> 1;
        for (s.row_max = 1; s.row_max <= npi; ++s.row_max) {
            s.ds = false; s.ds_n = 0;
            one(s);
            s.ds = true;
            for (s.ds_n = 1; s.ds_n <= 16; ++s.ds_n) one(s);
        }
        s.ds = false; s.ds_n = 0; s.br = true;
        for (s.br_rm = 1; s.br_rm <= 12; ++s.br_rm) { s.row_max = s.br_rm; one(s); }
    }
    std::printf("closure: %llu shapes, %zu distinct forms\n", shapes, swept.size());
    CHECK(swept.size() <= 19 + 18, "%zu forms from lists of 19 + 18", swept.size());

    // ---- equivalence with the recorded selection ----
    CHECK(argc > 1, "usage: test_mid_forms tests/golden/mid128_forms.txt");
    std::set<int> recorded;
    size_t lines = 0;
    if (argc > 1) {
        std::ifstream in(argv[1]);
        CHECK(in.good(), "cannot read %s", argv[1]);
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            const size_t bar = line.find(" | ");
            CHECK(bar != std::string::npos, "line without a note: %s", line.c_str());
            if (bar == std::string::npos) continue;
            std::istringstream is(line.substr(0, bar));
            Mid128Shape s;
            int perm, ds, br, mid_r;
            const bool ok = (bool)(is >> s.npi >> s.npo >> s.row_max >> s.ncols >> s.ncomp >> s.ds_n >> s.br_rm >> perm >> ds >> br >> mid_r);
            CHECK(ok, "bad shape: %s", line.c_str());
            if (!ok) continue;
            s.perm = perm; s.ds = ds; s.br = br; s.mid_r = mid_r;
            const Mid128Form f = mid128_form(s);
            const std::string want = line.substr(bar + 3), got = note_of(f);
            CHECK(got == want, "%s\n    recorded %s\n    derived  %s", line.substr(0, bar).c_str(), want.c_str(), got.c_str());
            CHECK(mid128_form_exists(f), "no entry for %s", got.c_str());
            recorded.insert(form_key(f));
            ++lines;
        }
        CHECK(lines >= 300, "%zu recorded shapes", lines);
        for (int k : swept) CHECK(recorded.count(k), "a form the sweep reaches is in no recorded shape (key %d)", k);
    }
    std::printf("equivalence: %zu recorded shapes, %zu distinct forms\n", lines, recorded.size());

    // ---- the block step: every (mr, cg) has an entry in the list of its kernel, or is reported as "no form" ----
    int none = 0;
    for (int lds = 0; lds < 2; ++lds)
    for (int row_max = 1; row_max <= 12; ++row_max)
    for (int ncols = 1; ncols <= 24; ++ncols) {
        const BrBlockForm f = br_block_form(row_max, ncols, lds != 0);
        if (f.mr == 0) {
            ++none;
            CHECK(f.cg == 0 && !lds && row_max == 9 && ncols % 12 == 0, "no form for %d rows, %d columns, lds %d", row_max, ncols, lds);
            CHECK(br_block_form(row_max, ncols, true).mr == 9 && br_block_form(row_max, ncols, true).cg == 4, "the LDS kernel has (9, 4)");
            continue;
        }
        CHECK(br_block_form_exists(f, lds != 0), "(%d, %d) has no entry, lds %d", f.mr, f.cg, lds);
        CHECK(f.mr >= row_max && f.cg >= 2 && f.cg <= 4, "(%d, %d) for %d rows", f.mr, f.cg, row_max);
    }
    CHECK(none == 2, "%d shapes without a form (9 rows with 12 and with 24 columns, no LDS)", none);
    CHECK(!br_block_form_exists(BrBlockForm{9, 4}, false) && br_block_form_exists(BrBlockForm{9, 4}, true), "(9, 4)");

    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("all middle-kernel form checks passed\n");
    return 0;
}
