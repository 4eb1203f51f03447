// ndtgpu_split.h -- how the registrar splits the chip between the grid builds and a matcher instance: every decision of a
// calibration sub-batch (ndtgpu_registrar.hip, calibrate) and the rule that asks for the next one, as plain host arithmetic.
// C++17 and the standard library only -- no HIP, no ndtgpu.h: tests/native/split_checks.cpp compiles it alone with g++.
// The thresholds compare doubles: operand order and casts are part of the rule.  Internal, not installed.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

// The kernels' own clocks of a calibration sub-batch: CU-time of the builds B and of the registrations M_raw.
struct SplitClocks {
    double B = 0, M_raw = 0, cells = 0;   // (B, M_raw: after finish())
    size_t n_results = 0, n_bad = 0;      // registrations seen / left out
    void add_map(const uint32_t cyc[4], uint32_t n_cells)
    {
        B += (double)cyc[0] + (double)cyc[1] + (double)cyc[2] + (double)cyc[3];
        cells += (double)n_cells;
    }
    // (a clock sum outside any plausible range -- seen once in six runs on the cluttered scene: 2^63 in one result -- is
    //  left out: the split is a heuristic, one registration does not move it; NDTGPU_REG_VERBOSE reports it)
    bool add_result(long long cycles_eval, long long cycles_solver)
    {
        const bool sane = cycles_eval >= 0 && cycles_eval < (1ll << 44) && cycles_solver >= 0 && cycles_solver < (1ll << 44);
        if (sane) M_raw += (double)cycles_eval + (double)cycles_solver / 8.0;
        else n_bad++;
        n_results++;
        return sane;
    }
    void finish()
    {
        B /= 4.0;                                         // a build workgroup shares its CU with three others
        if (n_bad < n_results) M_raw *= (double)n_results / (double)(n_results - n_bad);
    }
};

// what the model charges the matcher side: the raw CU-clocks of the sub-batch's registrations and a margin
// (measured optimum on the bench scene: 144 of 256 CUs where the raw clocks say 138)
inline double split_matcher_clocks(double M_raw) { return M_raw * 1.125; }

// The model: a matcher instance gets n_cu M / (M + B) CUs, rounded to eight, ...
inline unsigned split_proportional(double B, double M_raw, int n_cu)
{
    const double M = split_matcher_clocks(M_raw);
    double share = (M + B) > 0 ? M / (M + B) : 0.5;
    share = std::min(0.9, std::max(0.25, share));
    return std::max(8u, ((unsigned)(share * n_cu + 4.0) / 8u) * 8u);
}

// ... refined by what the build side really does with the CUs it is left: a build launch is one workgroup per
// map, four to a CU, so on F CUs it takes ceil(maps / 4F) ROUNDS of the mean workgroup time -- 2048 maps take
// four rounds on 128 CUs and five on 120, 112 or 104.  Of the splits around the proportional one, take the one
// whose slower side is fastest (the bench halls after the round's matcher savings: 136 by proportion, 573 k
// registrations/s; 128 by this rule, 624 k; 120: 585 k, 144: 544 k).
inline unsigned split_model(double B, double M_raw, size_t pairs, int n_cu)
{
    const double M = split_matcher_clocks(M_raw);
    const unsigned groups = split_proportional(B, M_raw, n_cu);
    if (!(B > 0 && M > 0)) return groups;
    const double wg = 4.0 * B / (2.0 * (double)pairs);            // mean clocks of a build workgroup
    double best_t = 0;
    unsigned best_g = groups;
    for (int g8 = (int)groups - 32; g8 <= (int)groups + 32; g8 += 8) {
        if (g8 < 16 || g8 > n_cu - 16) continue;
        const double slots = 4.0 * (n_cu - g8);
        const double t = std::max(M / g8, std::ceil(2.0 * (double)pairs / slots) * wg);
        const bool closer = std::abs(g8 - (int)groups) < std::abs((int)best_g - (int)groups);
        if (best_t == 0 || t < 0.99 * best_t || (t <= 1.01 * best_t && closer && t <= best_t)) { best_t = t; best_g = (unsigned)g8; }
    }
    return best_g;
}

// the most matcher CUs that leave the builds of `maps` maps k rounds (a multiple of 8 CUs, one per XCD; 0: none worth having)
inline unsigned split_groups_of(size_t maps, unsigned k, int n_cu)
{
    const unsigned F = (unsigned)((maps + 4u * k - 1u) / (4u * k));
    const unsigned F8 = (F + 7u) / 8u * 8u;
    return ((unsigned)n_cu > F8 + 15u) ? (unsigned)n_cu - F8 : 0u;
}

// (the clock under these kernels: 1.93-2.1 of 2.4 GHz)
inline double split_clk_per_ms(int khz) { return 0.85 * (double)(khz > 0 ? khz : 2400000); }

// The split, MEASURED on the build side.  The model's clocks are those of workgroups that had the whole chip: beside a matcher
// instance the builds of the bench halls run 20 % faster than that (half as many workgroups pull on the HBM), those of a
// cluttered scene 30 % slower (four workgroups to a CU where the lone launch had three), and a quarter more or less decides
// between two splits (halls 120 instead of 128 CUs on one box in three: -5 %; clutter 184 instead of 160: 103 against 127 k
// registrations/s).  A build launch takes whole rounds, so the only splits worth having are those that leave the builds just
// enough CUs for k rounds, k = 1, 2, ...: probe(g, &build_ms) -> bool times the sub-batch's builds beside g matcher CUs, and the
// split whose slower side -- that time, or the registrations' CU-clocks over the matcher's CUs -- is fastest wins.
struct SplitCand { unsigned g; double build_ms, match_ms, t_ms; };   // matcher CUs; the two sides; the slower one
struct SplitSearch {
    bool ok = true;                // false: a probe failed -- the search ended there and the model's split stands
    unsigned groups = 0;           // the split to use
    std::vector<SplitCand> cand;   // what was probed, in order
    bool have(unsigned g) const { for (const SplitCand &c : cand) if (c.g == g) return true; return false; }
    size_t best() const { size_t b = 0; for (size_t i = 1; i < cand.size(); i++) if (cand[i].t_ms < cand[b].t_ms) b = i; return b; }
};

template <class Probe>
SplitSearch split_probe_search(unsigned model_groups, size_t maps, int n_cu, double M_raw, double clk_per_ms, Probe &&probe)
{
    SplitSearch s;
    s.groups = model_groups;
    auto add = [&](unsigned k) {
        const unsigned g = k >= 1 && k <= 16 ? split_groups_of(maps, k, n_cu) : 0u;
        if (!s.ok || g < 16u || s.have(g)) return;
        SplitCand c{g, 0.0, 0.0, 0.0};
        if (!probe(g, &c.build_ms)) { s.ok = false; return; }
        c.match_ms = M_raw / (double)g / clk_per_ms;
        c.t_ms = std::max(c.build_ms, c.match_ms);
        s.cand.push_back(c);
    };
    // the round count the model's split stands for, and its neighbours; further out while the edge keeps winning
    unsigned k0 = 1;
    for (unsigned k = 1; k <= 16; k++) { k0 = k; if (split_groups_of(maps, k, n_cu) >= model_groups) break; }
    add(k0); add(k0 > 1 ? k0 - 1 : k0 + 2); add(k0 + 1);
    for (int more = 0; s.ok && more < 3 && !s.cand.empty(); more++) {
        const unsigned gb = s.cand[s.best()].g;
        unsigned kb = 0;
        for (unsigned k = 1; k <= 16; k++) if (split_groups_of(maps, k, n_cu) == gb) { kb = k; break; }
        const size_t n_before = s.cand.size();
        if (kb > 1 && !s.have(split_groups_of(maps, kb - 1, n_cu))) add(kb - 1);
        if (kb && kb < 16 && !s.have(split_groups_of(maps, kb + 1, n_cu))) add(kb + 1);
        if (s.cand.size() == n_before) break;
    }
    if (s.ok && !s.cand.empty()) s.groups = s.cand[s.best()].g;
    return s;
}

inline double split_cells_per_map(double cells, size_t pairs) { return cells / (double)(2 * pairs); }

// three registrations per workgroup (hit lists of 640 entries per share) where the maps are small -- up to 448 cells: the
// one-lane solver steps are a third of a registration there --, two with lists of 1024 entries otherwise (measured
// on the cluttered scene: three are slower)
inline int split_slots(double cells_per_map) { return cells_per_map <= 448.0 ? 3 : 2; }

// When is the split measured again?  The mean Gaussian cells per map of the last sub-batches seen (at most `depth`) against
// the figure the split stands for.
struct RecalWindow {
    std::vector<double> recent;    // mean cells per map of the last sub-batches seen
    double calib_cells = 0.0;      // mean Gaussian cells per map the split stands for: of the sub-batch it was first measured
                                   // on; after a re-measurement, of the recent sub-batches that asked for it (a registrar
                                   // that is fed two kinds of scenes in turn settles on their mean instead of measuring
                                   // again at every change)
    double recal_ref = 0.0;        // the mean that asked for the measurement under way (0: none)
    size_t calib_at = 0;           // the sub-batch the split was measured on
    // a map-counter sample arrived
    void sample(double cells_per_map, int depth)
    {
        if (recent.size() >= (size_t)depth) recent.erase(recent.begin());
        recent.push_back(cells_per_map);
    }
    // should sub-batch j measure again?  (`mean`: what the caller then stores in recal_ref, once the pipeline is drained)
    bool should_remeasure(size_t j, int depth, int pct, double *mean_out) const
    {
        if (!(recent.size() >= (size_t)std::min(depth, 4) && calib_cells > 0 && j >= calib_at + 2 * (size_t)depth)) return false;
        double mean = 0;
        for (double v : recent) mean += v;
        mean /= (double)recent.size();
        *mean_out = mean;
        return std::fabs(mean / calib_cells - 1.0) * 100.0 > (double)pct;
    }
    // sub-batch j measured the split on maps of `cells_per_map`
    void measured(double cells_per_map, size_t j)
    {
        calib_cells = recal_ref > 0 ? recal_ref : cells_per_map;
        recal_ref = 0.0;
        calib_at = j;
        recent.clear();
    }
};
