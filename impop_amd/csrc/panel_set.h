// panel_set.h — K disjoint panels of haplotypes as the all-pairs calls over panels lay them out (impop_pairdist_scan,
// impop_permtest_scan, impop_pairwise_scan_panel): who is in which panel, the panels' members as POSITIONS 0 .. M - 1, and per pair of
// panels both panels' positions merged into one ascending list.  Membership is win_chunks.h member_set.  Plain C++, no HIP:
// tests/fuzz/panel_set.cc compiles it on the host under the sanitizers and checks it against a brute-force model.
#pragma once
#include <stdint.h>

#include <vector>

#include "win_chunks.h"

namespace impop {

constexpr uint32_t PANEL_MAX_K = 8;
// why a set of masks is no panel set: population k shares a member with the earlier population `other`, or has none
struct PanelRefusal {
    enum Kind { NONE, OVERLAP, EMPTY } kind = NONE;
    uint32_t k = 0, other = 0;
};
struct PanelSet {
    std::vector<uint8_t> cls;       // n_hap: the panel of haplotype i, 0xFF: in none
    std::vector<uint32_t> hap_of;   // M: the panels' members back to back, each ascending: position -> haplotype
    std::vector<uint32_t> sizes;    // K: members per panel
    uint32_t off[PANEL_MAX_K + 1];  // panel k is the positions off[k] .. off[k + 1); the entries from K on equal M
    uint32_t K = 0, M = 0;
    uint32_t size(uint32_t k) const { return off[k + 1] - off[k]; }
};

// masks: K <= PANEL_MAX_K bitsets of ceil(n_hap / 64) words each, back to back (member_set's convention: null means everyone,
// bits at or above n_hap are ignored).  The populations in turn; the first one that overlaps an earlier one or is empty is the refusal.
inline PanelRefusal panel_set(const uint64_t *masks, uint32_t K, uint32_t n_hap, PanelSet &out) {
    const uint32_t mwords = (n_hap + 63) / 64;
    out.cls.assign(n_hap, 0xFF);
    out.hap_of.clear();
    out.sizes.assign(K, 0);
    out.K = K;
    for (uint32_t k = 0; k < K; ++k) {
        out.off[k] = (uint32_t)out.hap_of.size();
        for (uint32_t i : member_set(masks ? masks + (size_t)k * mwords : nullptr, n_hap, (n_hap + 31) / 32).idx) {
            if (out.cls[i] != 0xFF) return PanelRefusal{PanelRefusal::OVERLAP, k, out.cls[i]};
            out.cls[i] = (uint8_t)k;
            out.hap_of.push_back(i);
        }
        out.sizes[k] = (uint32_t)out.hap_of.size() - out.off[k];
        if (!out.sizes[k]) return PanelRefusal{PanelRefusal::EMPTY, k, 0};
    }
    out.M = (uint32_t)out.hap_of.size();
    for (uint32_t k = K; k <= PANEL_MAX_K; ++k) out.off[k] = out.M;
    return PanelRefusal{};
}

// Per pair of panels p = (a, b), a < b, in the order (0,1),(0,2),..,(1,2),.. of impop_scan_multi: the positions of both panels in
// ascending haplotype index at merged[moff[p] .. moff[p + 1]) (the order of the S_nn sum), and, when asked for, the observed
// labelling z0: bit `at` of the pair's mw_max words at z0[p * mw_max] is set when entry `at` of its list comes from panel a.
struct MergedPairs {
    std::vector<uint32_t> merged, moff = {0u};  // moff: K (K - 1) / 2 + 1
    std::vector<uint64_t> z0;            // K (K - 1) / 2 x mw_max, or empty
    uint32_t m_max = 0, mw_max = 0;      // the longest list and its 64-bit words
};
inline MergedPairs merged_pairs(const PanelSet &P, bool want_z0) {
    MergedPairs R;
    for (uint32_t a = 0; a < P.K; ++a)
        for (uint32_t b = a + 1; b < P.K; ++b) R.m_max = std::max(R.m_max, P.size(a) + P.size(b));
    R.mw_max = (R.m_max + 63) / 64;
    for (uint32_t a = 0, p = 0; a < P.K; ++a)
        for (uint32_t b = a + 1; b < P.K; ++b, ++p) {
            uint32_t i = P.off[a], j = P.off[b];
            if (want_z0) R.z0.resize((size_t)(p + 1) * R.mw_max, 0ull);
            for (uint32_t at = 0; i < P.off[a + 1] || j < P.off[b + 1]; ++at) {
                const bool from_a = j >= P.off[b + 1] || (i < P.off[a + 1] && P.hap_of[i] < P.hap_of[j]);
                if (from_a && want_z0) R.z0[(size_t)p * R.mw_max + (at >> 6)] |= 1ull << (at & 63u);
                R.merged.push_back(from_a ? i++ : j++);
            }
            R.moff.push_back((uint32_t)R.merged.size());
        }
    return R;
}

}  // namespace impop
