// kin_math.h — the integer arithmetic of impop_kinship_scan (plain C++, no HIP types: tests/fuzz/kin_math.cc compiles it on the
// host under the sanitizers; kinship.hip runs the same code on the device).
//
// Individual i has two bit planes over the sites: H_i = h1 ^ h2 (heterozygous) and A_i = h1 & h2 (homozygous for the allele).  With
// the popcount-AND counts HH = |H_i & H_j|, HA = |H_i & A_j|, AH = |A_i & H_j|, AA = |A_i & A_j|, the diagonals het = |H|, alt = |A|
// and the window's W, the 3 x 3 joint genotype table t[a][b] (a = genotype of i, b = of j; 0 hom-ref, 1 het, 2 hom-alt) follows.
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

namespace impop {

struct KinTable {
    int64_t t[9];  // t[3 a + b]
};

// the table from the Gram entries; false when a cell comes out negative (the entries cannot be popcounts of one window)
DIP_HD inline bool kin_table(int64_t W, int64_t het_i, int64_t alt_i, int64_t het_j, int64_t alt_j, int64_t HH, int64_t HA, int64_t AH,
                             int64_t AA, KinTable &k) {
    int64_t *t = k.t;
    t[4] = HH; t[5] = HA; t[7] = AH; t[8] = AA;
    t[3] = het_i - HH - HA;  // t10
    t[1] = het_j - HH - AH;  // t01
    t[6] = alt_i - AH - AA;  // t20
    t[2] = alt_j - HA - AA;  // t02
    int64_t rest = 0;
    for (int c = 1; c < 9; ++c) rest += t[c];
    t[0] = W - rest;
    bool ok = true;
    for (int c = 0; c < 9; ++c) ok = ok && t[c] >= 0;
    return ok;
}
DIP_HD inline int64_t kin_het_het(const KinTable &k) { return k.t[4]; }
DIP_HD inline int64_t kin_ibs0(const KinTable &k) { return k.t[2] + k.t[6]; }
DIP_HD inline int64_t kin_ibs2(const KinTable &k) { return k.t[0] + k.t[4] + k.t[8]; }

// KING-robust kinship >= num / den, exactly:  (2 (hh - 2 ibs0) + 2 m - a - b) / (4 m) >= num / den  with m = min(a, b) > 0.
// m == 0: undefined, never related.  |hh - 2 ibs0| < 2^33, den <= 2^20, m < 2^31: both sides stay below 2^56.
DIP_HD inline bool kin_related(int64_t het_i, int64_t het_j, int64_t het_het, int64_t ibs0, int64_t num, int64_t den) {
    const int64_t m = het_i < het_j ? het_i : het_j;
    if (m <= 0) return false;
    return den * (2 * (het_het - 2 * ibs0) + 2 * m - het_i - het_j) >= 4 * m * num;
}

// index of the pair i < j among N, in impop_scan_multi's order (0,1),(0,2),..,(1,2),..
DIP_HD inline uint64_t kin_pair_index(uint64_t N, uint64_t i, uint64_t j) { return i * (2 * N - i - 1) / 2 + (j - i - 1); }

}  // namespace impop
