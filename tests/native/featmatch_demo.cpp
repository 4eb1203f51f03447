// featmatch_demo.cpp -- the host mirror's feature maps and matcher (host/ndt_feature_map_gpu.h) called the way computeLink and
// computeAllPossibleLinks call them (ndt_feature_graph.cpp:162-177, :395-405): 6 maps of one scene seen from 6 poses -> 15 links in
// one device call, against the ndtgpu_featbank_* calls it wraps given the same sets by hand -- poses, scores and correspondences
// must be those of the C-ABI bit for bit -- and matchFeatureMap's max() for an empty map.  Exit code 0 = every check passed;
// without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_map_gpu.h"

#include <cstdio>
#include <limits>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

int main()
{
    const size_t n_maps = 6, n_world = 40, desc_len = 48;
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> nd(0.0, 1.0);
    // a world of 40 interest points with normalised random histograms
    std::vector<InterestPointGPU> world(n_world);
    for (InterestPointGPU &p : world) {
        p.x = 20.0 * U(rng) - 10.0;
        p.y = 20.0 * U(rng) - 10.0;
        p.descriptor.resize(desc_len);
        double sum = 0;
        for (double &d : p.descriptor) sum += d = U(rng);
        for (double &d : p.descriptor) d /= sum;
    }
    // map k sees 30 of them from its own pose, with 1 cm of noise; update's every-4th-call rule decides what it keeps
    std::vector<NDTFeatureMapGPU> maps(n_maps);
    std::vector<std::array<double, 3>> pose(n_maps);
    for (size_t k = 0; k < n_maps; k++) {
        pose[k] = {0.3 * (double)k, -0.2 * (double)k, 0.1 * (double)k};
        const double c = std::cos(pose[k][2]), s = std::sin(pose[k][2]);
        InterestPointGPUVec seen, later;
        for (size_t i = 0; i < n_world; i++) {
            if ((i + k) % 4 == 0) continue;
            InterestPointGPU p = world[i];
            const double dx = world[i].x - pose[k][0], dy = world[i].y - pose[k][1];
            p.x = c * dx + s * dy + 0.01 * nd(rng);
            p.y = -s * dx + c * dy + 0.01 * nd(rng);
            p.theta = -pose[k][2];
            seen.push_back(p);
        }
        later.push_back(world[0]);
        maps[k].update(seen);                 // call 0: appended
        maps[k].update(later);                // calls 1-3: dropped
        maps[k].update(later);
        maps[k].update(later);
        CHECK(maps[k].getMap().size() == 30, "map %zu holds %zu points", k, maps[k].getMap().size());
    }
    maps[0].update(InterestPointGPUVec());    // call 4: appended (nothing)

    std::vector<NDTFeatureMatchLink> links;
    try {
        links = computeAllPossibleFeatureLinks(maps);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("featmatch_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    CHECK(links.size() == 15, "%zu links", links.size());

    // the same by hand: a bank of another shape, the maps in its last slots
    ndtgpu_featbank *h = nullptr;
    ndtgpu_host::check(ndtgpu_featbank_create(n_maps + 2, 50, desc_len, &h), "ndtgpu_featbank_create");
    for (size_t k = 0; k < n_maps; k++) {
        std::vector<double> pos, desc;
        for (const InterestPointGPU &p : maps[k].map) {
            pos.push_back(p.x); pos.push_back(p.y); pos.push_back(p.theta);
            desc.insert(desc.end(), p.descriptor.begin(), p.descriptor.end());
        }
        ndtgpu_host::check(ndtgpu_featbank_set(h, k + 2, maps[k].map.size(), pos.data(), desc.data()), "ndtgpu_featbank_set");
    }
    std::vector<uint32_t> ref, mov;
    for (size_t i = 0; i < n_maps; i++)
        for (size_t j = i + 1; j < n_maps; j++) { ref.push_back((uint32_t)i + 2); mov.push_back((uint32_t)j + 2); }
    ndtgpu_host::check(ndtgpu_featbank_match(h, ref.data(), mov.data(), ref.size(), nullptr, nullptr), "ndtgpu_featbank_match");
    std::vector<ndtgpu_featmatch_result> res(ref.size());
    std::vector<double> T16(16 * ref.size());
    std::vector<uint32_t> corr(ref.size() * 50 * 2);
    ndtgpu_host::check(ndtgpu_featbank_results(h, 0, ref.size(), res.data(), T16.data(), corr.data()), "ndtgpu_featbank_results");
    ndtgpu_featbank_destroy(h);

    int equal = 0;
    double worst = 0;
    for (size_t p = 0; p < links.size() && p < ref.size(); p++) {
        const NDTFeatureMatchLink &l = links[p];
        bool same = l.ref_idx + 2 == ref[p] && l.mov_idx + 2 == mov[p] && l.score == res[p].score && res[p].status == NDTGPU_FEATMATCH_OK &&
                    l.matches.size() == (size_t)res[p].n_inliers;
        for (int e = 0; e < 16; e++) same = same && l.T.data()[e] == T16[16 * p + e];
        for (size_t k = 0; same && k < l.matches.size(); k++)
            same = l.matches[k].first == corr[(p * 50 + k) * 2] && l.matches[k].second == corr[(p * 50 + k) * 2 + 1];
        CHECK(same, "link %zu (%zu, %zu): the mirror differs from the C-ABI", p, l.ref_idx, l.mov_idx);
        equal += same ? 1 : 0;
        // link.T maps mov into ref: pose_ref^-1 * pose_mov
        const double *a = pose[l.ref_idx].data(), *b = pose[l.mov_idx].data();
        const double c = std::cos(a[2]), s = std::sin(a[2]), dx = b[0] - a[0], dy = b[1] - a[1];
        worst = std::max(worst, std::hypot(l.T.translation()(0) - (c * dx + s * dy), l.T.translation()(1) - (-s * dx + c * dy)));
        CHECK(l.matches.size() >= 15, "link %zu: %zu correspondences", p, l.matches.size());
    }
    CHECK(worst < 0.05, "a link ends %.3f m from the truth", worst);

    // one pair through matchFeatureMap: the link's values; an empty map: max(), T and matches untouched
    CorrespondencesGPU m;
    Eigen::Affine3d T;
    const double score = matchFeatureMap(maps[1], maps[4], m, T);
    const NDTFeatureMatchLink &l14 = links[7];                       // (0,1) .. (0,5), (1,2), (1,3), (1,4)
    bool same = l14.ref_idx == 1 && l14.mov_idx == 4 && score == l14.score && m == l14.matches;
    for (int e = 0; e < 16; e++) same = same && T.data()[e] == l14.T.data()[e];
    CHECK(same, "matchFeatureMap differs from the batch's link (1, 4)");
    NDTFeatureMapGPU none;
    Eigen::Affine3d Tu = ndtgpu_host::affine_from_pose(1, 2, 0, 0, 0, 0.5), Tu0 = Tu;
    CorrespondencesGPU mu(3);
    const double big = std::numeric_limits<double>::max();
    CHECK(matchFeatureMap(none, maps[0], mu, Tu) == big && matchFeatureMap(maps[0], none, mu, Tu) == big, "an empty map must return max()");
    bool untouched = mu.size() == 3;
    for (int e = 0; e < 16; e++) untouched = untouched && Tu.data()[e] == Tu0.data()[e];
    CHECK(untouched, "an empty map must leave T and matches alone");
    std::vector<NDTFeatureMapGPU> with_empty = {maps[0], none, maps[1]};
    const std::vector<NDTFeatureMatchLink> le = computeAllPossibleFeatureLinks(with_empty);
    CHECK(le.size() == 3 && le[0].score == big && le[2].score == big && le[0].matches.empty(), "links with an empty map");
    CHECK(le.size() == 3 && le[1].score == links[0].score && le[1].matches == links[0].matches, "the link (0, 2) beside an empty map");

    std::printf("featmatch_demo: %zu maps, %zu links, %d equal to the C-ABI bit for bit, worst |dt| %.4f m, %d failures\n", n_maps,
                links.size(), equal, worst, g_fails);
    return g_fails ? 1 : 0;
}
