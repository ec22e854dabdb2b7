// mid_forms.hpp — the instantiations of the 128-point-row middle kernels (k_mid128 / k_mid128r, device_mid.hpp) and the choice among them.
// Plain C++ with no HIP header: launch_mid.hip walks the two lists to launch, tests/cpp/test_mid_forms.cpp compiles the choice with the host
// compiler and sweeps it (every form chosen has an entry; the notes are the ones tests/golden/mid128_forms.txt records).
#pragma once
#include <cstddef>
#include <cstdio>

namespace pz {

// what the choice depends on (the batch, m1 and the CU count only size the grid)
struct Mid128Shape {
    int npi = 0, npo = 0;        // polynomials in / out per ciphertext
    int row_max = 0;             // product rows: min(key rows, npi)
    int ncols = 0, ncomp = 0;    // key columns; output columns computed: min(npo, ncols)
    int ds_n = 0;                // digit-selected product: its terms
    int br_rm = 0;               // CGGI block step: key rows of one GGSW
    bool perm = false, ds = false, br = false;
    bool mid_r = true;           // POULPY_DBG_MID_R; false: k_mid128 where k_mid128r would run (A/B)
};

// one instantiation: tile of ct ciphertexts x np polynomial slots, then the template arguments of the kernel named by `ring`
struct Mid128Form {
    bool ring = false;           // k_mid128r (key rows through a ring of LDS slots) instead of k_mid128
    int ct = 4, np = 16;
    bool perm = false, ds = false;
    // k_mid128
    bool br = false, skipw = false;
    int brnest = 0, nco = 0;
    // k_mid128r (KR is the kernel's default)
    int nr = 0;
    bool halfin = false, c2 = false;
};

// k_mid128: (CT, NP, PERM, DS, BR, SKIPW, BRNEST, NCO)
#define PZ_MID128_FORMS(X)                                                                                                   \
    X(8, 8, false, false, false, false, 0, 0) X(8, 8, true, false, false, false, 0, 0)                                       \
    X(4, 16, false, false, false, false, 0, 0) X(4, 16, true, false, false, false, 0, 0)                                     \
    X(4, 16, false, false, false, true, 0, 0) X(4, 16, true, false, false, true, 0, 0)                                       \
    X(2, 32, false, false, false, false, 0, 0) X(2, 32, true, false, false, false, 0, 0)                                     \
    X(2, 32, false, false, false, true, 0, 0) X(2, 32, true, false, false, true, 0, 0)                                       \
    X(8, 8, false, true, false, false, 0, 0) X(4, 16, false, true, false, false, 0, 0) X(2, 32, false, true, false, false, 0, 0) \
    X(8, 8, false, false, true, false, 0, 0) X(4, 16, false, false, true, false, 0, 0) X(2, 32, false, false, true, false, 0, 0) \
    X(8, 8, false, false, true, false, 2, 0) X(4, 16, false, false, true, false, 2, 0) X(8, 8, false, false, true, false, 2, 3)
// k_mid128r: (CT, NP, PERM, NR, HALFIN, DS, C2)
#define PZ_MID128R_FORMS(X)                                                                                                  \
    X(8, 8, false, 8, false, false, false) X(8, 8, true, 8, false, false, false)                                             \
    X(4, 16, false, 16, false, false, false) X(4, 16, false, 8, true, false, false) X(4, 16, false, 8, false, false, false)   \
    X(4, 16, true, 16, false, false, false) X(4, 16, true, 8, true, false, false) X(4, 16, true, 8, false, false, false)      \
    X(2, 32, false, 32, false, false, false) X(2, 32, false, 16, true, false, false) X(2, 32, false, 16, false, false, false) \
    X(2, 32, true, 32, false, false, false) X(2, 32, true, 16, true, false, false) X(2, 32, true, 16, false, false, false)    \
    X(4, 16, false, 16, false, true, false) X(4, 16, false, 8, true, true, false)                                            \
    X(4, 16, false, 16, false, false, true) X(4, 16, true, 16, false, false, true)

inline bool mid128_form_exists(const Mid128Form& f) {
    if (f.ring) {
#define X(CT_, NP_, PERM_, NR_, HALFIN_, DS_, C2_)                                                                           \
    if (f.ct == CT_ && f.np == NP_ && f.perm == PERM_ && f.nr == NR_ && f.halfin == HALFIN_ && f.ds == DS_ && f.c2 == C2_) return true;
        PZ_MID128R_FORMS(X)
#undef X
        return false;
    }
#define X(CT_, NP_, PERM_, DS_, BR_, SKIPW_, BRNEST_, NCO_)                                                                  \
    if (f.ct == CT_ && f.np == NP_ && f.perm == PERM_ && f.ds == DS_ && f.br == BR_ && f.skipw == SKIPW_ && f.brnest == BRNEST_ && f.nco == NCO_) return true;
    PZ_MID128_FORMS(X)
#undef X
    return false;
}

// which instantiation for this shape: tile geometry by the polynomials in and out, then the product form (CGGI block step / digit-selected /
// plain or permuted)
inline Mid128Form mid128_form(const Mid128Shape& s) {
    Mid128Form f;
    // 16 polynomials in, 32 = 16 limbs x 2 columns out, 16 key rows of 32 columns (rank-1 key switch / automorphism / relinearization at 16 limbs:
    // BASELINE configs[4]): 4 ciphertexts per tile and the two output columns as two passes over the same inputs - every key value serves 4
    // ciphertexts instead of the 32-slot tile's 2 (k_mid128r<.., C2>; profiles/r06_ab_mid_c2.txt)
    if (s.mid_r && !s.br && !s.ds && s.npi == 16 && s.npo == 32 && s.row_max == 16 && s.ncols == 32 && s.ncomp == 32) {
        f.ring = true; f.ct = 4; f.np = 16; f.perm = s.perm; f.nr = 16; f.c2 = true;
        return f;
    }
    if (s.npi <= 8 && s.npo <= 8) {
        // <= 8 polynomials in and out (e.g. rank 1 with 4 limbs, BASELINE configs[1]): 8 ciphertexts x 8 slots per tile
        f.ct = 8; f.np = 8;
    } else if (s.npi > 16 || s.npo > 16) {
        // 17..32 polynomials in or out (rank 2-3 with 8 limbs, rank 1 with 16 limbs): 2 ciphertexts x 32 slots per tile
        f.ct = 2; f.np = 32;
    } else {
        f.ct = 4; f.np = 16;
    }
    const int np = f.np;
    if (s.br) {   // ct ciphertexts per key value
        f.br = true;
        if ((s.br_rm & 1) == 0 && np < 32) {   // an even number of key rows per coefficient: the nested form of the product loop
            f.brnest = 2;
            if (np == 8 && s.ncomp == 6 && s.npi <= 6) f.nco = 3;   // six output columns in an 8-slot tile: 2 x 3 per thread
        }
        return f;
    }
    if (s.ds) {
        f.ds = true;
        // 16-slot tile with 16 terms on 16 inputs (external product) or 8 terms on <= 8 inputs (key switch): k_mid128r
        if (s.mid_r && np == 16 && s.ds_n == 16 && s.npi == 16) { f.ring = true; f.nr = 16; }
        else if (s.mid_r && np == 16 && s.ds_n == 8 && s.npi <= 8 && s.npo > 8) { f.ring = true; f.nr = 8; f.halfin = true; }
        return f;
    }
    // plain product: the interleaved kernel k_mid128r where it applies - 8 or 16 product rows, no idle waves or exactly the upper half of a
    // 16-slot tile without input (key switch) - k_mid128 otherwise
    f.perm = s.perm;
    const bool skipw = np > 8 && (s.npi <= np - 8 || s.npo <= np - 8);   // shapes with idle waves
    const bool ring = s.mid_r && (s.row_max == np || (np >= 16 && s.row_max == np / 2));   // product rows k_mid128r is built for
    const bool half_in = np >= 16 && s.npi <= np / 2;   // the upper half of the slots without input
    if (ring && (!skipw || (half_in && s.npo > np / 2))) {
        // k_mid128r: product rows = NP (no idle waves) or NP / 2, then with or without input in the upper half of the slots
        f.ring = true;
        if (s.row_max == np) f.nr = np;
        else { f.nr = np / 2; f.halfin = half_in; }
    } else {
        f.skipw = skipw;
    }
    return f;
}

// the dispatch note of a form (tests, profiles/ and the bench tools match on these); midr_kr: PZ_MIDR_KR of the build (device_mid.hpp)
inline void mid128_note(const Mid128Form& f, int midr_kr, char* buf, size_t n) {
    const int kr = f.np == 32 ? 3 : midr_kr;
    if (f.ring && f.c2)
        snprintf(buf, n, "k_mid128r<CT=%d,NP=%d,PERM=%d,NR=%d,HALFIN=%d,KR=%d,C2=1> (two output-column passes per tile of %d ciphertexts)", f.ct,
                 f.np, (int)f.perm, f.nr, (int)f.halfin, kr, f.ct);
    else if (f.ring && f.ds) snprintf(buf, n, "k_mid128r<CT=%d,NP=%d,NR=%d,HALFIN=%d,KR=%d,DS=1>", f.ct, f.np, f.nr, (int)f.halfin, kr);
    else if (f.ring) snprintf(buf, n, "k_mid128r<CT=%d,NP=%d,PERM=%d,NR=%d,HALFIN=%d,KR=%d>", f.ct, f.np, (int)f.perm, f.nr, (int)f.halfin, kr);
    else if (f.br && f.nco) snprintf(buf, n, "k_mid128<CT=%d,NP=%d,BR=1,BRNEST=%d,NCO=%d> (%d ciphertexts per key value)", f.ct, f.np, f.brnest, f.nco, f.ct);
    else if (f.br && f.brnest) snprintf(buf, n, "k_mid128<CT=%d,NP=%d,BR=1,BRNEST=%d> (%d ciphertexts per key value)", f.ct, f.np, f.brnest, f.ct);
    else if (f.br) snprintf(buf, n, "k_mid128<CT=%d,NP=%d,BR=1> (%d ciphertexts per key value)", f.ct, f.np, f.ct);
    else if (f.ds) snprintf(buf, n, "k_mid128<CT=%d,NP=%d,DS=1>", f.ct, f.np);
    else snprintf(buf, n, "k_mid128<CT=%d,NP=%d,PERM=%d,DS=0,BR=0,SKIPW=%d>", f.ct, f.np, (int)f.perm, (int)f.skipw);
}

}  // namespace pz
