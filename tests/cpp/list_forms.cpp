// Host-only list of every kernel instantiation the hot path chooses among, expanded from the X-macro lists themselves (mid_forms.hpp,
// tail_plan.hpp, br_forms.hpp) and spelled as the dispatch notes spell them: tests/test_form_census_host.py holds the list against the
// census table (tests/form_census_cases.py), entry for entry.  No HIP, its own main.
//   list_forms                       one line per form: the note up to its closing '>' (the fused tail: the whole note)
//   list_forms mid <npi> <npo> <nrows> <ncols> <ds_n> <br_rm> <perm> <ds> <br>
//                                    the note mid128_form chooses for the shape launch_mid (launch_mid.hip) derives from these
//   list_forms brblock <row_max> <ncols> <use_lds>
//                                    the note of the block step br_block_form chooses, or "none"
//   list_forms tail-gate             per plan of the fused tail: does tail_supported() (tail_plan_whole_waves), which every caller asks first, admit it
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../poulpy_amd/csrc/br_forms.hpp"
#include "../../poulpy_amd/csrc/mid_forms.hpp"
#include "../../poulpy_amd/csrc/tail_plan.hpp"

using namespace pz;

constexpr int kKR = 6;   // PZ_MIDR_KR of a default build (device_mid.hpp)

// a note up to and with its closing '>'
static std::string upto_gt(const char* note) {
    const char* gt = std::strchr(note, '>');
    return gt ? std::string(note, gt + 1) : std::string(note);
}
static std::string mid_key(const Mid128Form& f) {
    char buf[160];
    mid128_note(f, kKR, buf, sizeof buf);
    return upto_gt(buf);
}
static std::string tail_key(TailForm::Kind kind, bool rowmajor, bool has_small, int a, int b, int c) {
    TailForm f;
    f.kind = kind; f.rowmajor = rowmajor; f.has_small = has_small;
    char buf[64];
    tail_note(f, a, b, c, buf, sizeof buf);
    return buf;
}

static void list_all() {
#define X(CT_, NP_, PERM_, DS_, BR_, SKIPW_, BRNEST_, NCO_)                                                                  \
    { Mid128Form f; f.ct = CT_; f.np = NP_; f.perm = PERM_; f.ds = DS_; f.br = BR_; f.skipw = SKIPW_; f.brnest = BRNEST_; f.nco = NCO_; \
      std::printf("%s\n", mid_key(f).c_str()); }
    PZ_MID128_FORMS(X)
#undef X
#define X(CT_, NP_, PERM_, NR_, HALFIN_, DS_, C2_)                                                                           \
    { Mid128Form f; f.ring = true; f.ct = CT_; f.np = NP_; f.perm = PERM_; f.nr = NR_; f.halfin = HALFIN_; f.ds = DS_; f.c2 = C2_; \
      std::printf("%s\n", mid_key(f).c_str()); }
    PZ_MID128R_FORMS(X)
#undef X
#define X(A, B, C) for (int v = 0; v < 4; ++v) std::printf("%s\n", tail_key(TailForm::PLAIN, v >> 1, v & 1, A, B, C).c_str());
    PZ_P1F_CASES(X)
#undef X
    static const TailForm::Kind rsh_kinds[] = {TailForm::RSH, TailForm::SGN, TailForm::SGN16, TailForm::SGN16R, TailForm::NZ2, TailForm::NZ1,
                                               TailForm::NZ1W, TailForm::NZ2R, TailForm::NZ1O, TailForm::NZ2O};   // (tail_forms.hpp walks these ten)
#define X(A, B, C) for (TailForm::Kind k : rsh_kinds) std::printf("%s\n", tail_key(k, true, false, A, B, C).c_str());
    PZ_RSH_CASES(X)
#undef X
#define X(A, B, C) std::printf("%s\n", tail_key(TailForm::ACC32, true, true, A, B, C).c_str());
    PZ_ACC32_CASES(X)
#undef X
    // the blind-rotation kernels write their notes where they launch (br_forms.hpp, launch_br.hip): the same spelling, up to the '>'
#define X(R0_, CT_, PJ_, MR_, CG_, A32_) std::printf("k_br_fused<R0=%d,CT=%d,NT=512,PJ=%d,MR=%d,CG=%d,A32=%d>\n", R0_, CT_, PJ_, MR_, CG_, (int)(A32_));
    PZ_BR_FORMS(X)
#undef X
#define X(R0_, PJ_, MR_, CG_, A32_) std::printf("k_br_fused<R0=%d,CT=1,NT=256,PJ=%d,MR=%d,CG=%d,A32=%d>\n", R0_, PJ_, MR_, CG_, (int)(A32_));
    PZ_BR_HALF_FORMS(X)
#undef X
#define X(R0_, PJ_, MR_, CG_) std::printf("k_br_fused<R0=%d,CT=1,NT=512,PJ=%d,MR=%d,CG=%d,A32=0,STD=1>\n", R0_, PJ_, MR_, CG_);
    PZ_BR_STD_FORMS(X)
#undef X
#define X(MR_, CG_) std::printf("k_br_block_lds<2,MR=%d,CG=%d>\n", MR_, CG_);
    PZ_BR_BLOCK_LDS_FORMS(X)
#undef X
#define X(MR_, CG_) std::printf("k_br_block<2,MR=%d,CG=%d>\n", MR_, CG_);
    PZ_BR_BLOCK_FORMS(X)
#undef X
}

int main(int argc, char** argv) {
    if (argc == 1 || (argc == 2 && !std::strcmp(argv[1], "--list"))) { list_all(); return 0; }
    if (argc == 11 && !std::strcmp(argv[1], "mid")) {
        int v[9];
        for (int i = 0; i < 9; ++i) v[i] = std::atoi(argv[2 + i]);
        Mid128Shape s;
        const int nrows = v[2];
        s.npi = v[0]; s.npo = v[1]; s.ncols = v[3]; s.ds_n = v[4]; s.br_rm = v[5]; s.perm = v[6]; s.ds = v[7]; s.br = v[8];
        s.row_max = s.br ? nrows : std::min(nrows, s.npi);   // launch_mid: the block step hands over the rows of all its GGSWs
        s.ncomp = std::min(s.npo, s.ncols);
        const Mid128Form f = mid128_form(s);
        if (!mid128_form_exists(f)) { std::printf("none\n"); return 1; }
        std::printf("%s\n", mid_key(f).c_str());
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "brblock")) {
        const bool lds = std::atoi(argv[4]) != 0;
        const BrBlockForm f = br_block_form(std::atoi(argv[2]), std::atoi(argv[3]), lds);
        if (f.mr == 0) { std::printf("none\n"); return 0; }
        std::printf(lds ? "k_br_block_lds<2,MR=%d,CG=%d>\n" : "k_br_block<2,MR=%d,CG=%d>\n", f.mr, f.cg);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "tail-gate")) {
#define X(A, B, C) std::printf("k_inv_tail<%d,%d,%d> | %d\n", A, B, C, (int)tail_plan_whole_waves(B, C));
        PZ_P1F_CASES(X)
#undef X
        return 0;
    }
    std::fprintf(stderr, "usage: list_forms [--list | mid <9 ints> | brblock <row_max> <ncols> <use_lds> | tail-gate]\n");
    return 2;
}
