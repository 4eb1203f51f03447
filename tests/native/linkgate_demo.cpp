// linkgate_demo.cpp -- the host mirror's link gate (host/ndt_link_gate_gpu.h: computeCandidateLinks, getValidLinksGPU,
// optimizeGraphGated over ndtgpu_linkgate_*) against the scalar code it stands beside: NDTFeatureGraph::getValidLinks and
// distanceBetweenAffine3d of host/ndt_feature_graph_gpu.h (Eigen's inverse, libm's acos), and the loop of
// ndt_feature_graph_opt.cpp:152-173 written out with them.  The two round differently, so a link the scalar code places within
// 1e-9 of a threshold (or whose cosine is within 1e-12 of 1 under upstream's NaN rule) is left out of the comparison, and the demo
// fails if that is more than 0.1 % of them.  Exit code 0 = every check passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_link_gate_gpu.h"

#include <cstdio>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

// a graph of poses alone: the nodes have no maps (the gate and the optimiser read poses and links only)
struct PoseGraph : NDTFeatureGraph {
    void addNode(const Eigen::Affine3d &T)
    {
        NDTFeatureNode n;
        n.T = T;
        nodes_.push_back(n);
    }
};

static bool in_band(const Eigen::Affine3d &own, const Eigen::Affine3d &pred, double maxDist, double maxAngle, bool clipped)
{
    double dist, ang;
    distanceBetweenAffine3d(own, pred, dist, ang);
    const double c = (own.inverse() * pred)(0, 0);
    return std::fabs(dist - maxDist) < 1e-9 || std::fabs(ang - maxAngle) < 1e-9 || (!clipped && std::fabs(c) > 1.0 - 1e-12);
}

int main()
{
    std::mt19937 rng(21);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 0.2);

    // ---- 1. getValidLinksGPU against NDTFeatureGraph::getValidLinks: 60 nodes on a walk, every pair a perturbed link ----------
    const size_t n = 60;
    PoseGraph graph;
    double x = 0, y = 0, t = 0;
    for (size_t i = 0; i < n; i++) {
        t += 0.25 * nd(rng);
        x += 2.0 * std::cos(t);
        y += 2.0 * std::sin(t);
        graph.addNode(ndtgpu_host::affine_from_pose(x, y, 0, 0, 0, t));
    }
    std::vector<NDTFeatureLink> links;
    for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
            NDTFeatureLink l(i, j);
            l.T = graph.getNode(i).T.inverse() * graph.getNode(j).T * ndtgpu_host::affine_from_pose(0.6 * nd(rng), 0.6 * nd(rng), 0, 0, 0, 0.15 * nd(rng));
            l.score = ud(rng);
            if ((i + j) % 7 == 0) {                      // some links the other way round: ref > mov
                std::swap(l.ref_idx, l.mov_idx);
                l.T = l.T.inverse();
            }
            links.push_back(l);
        }
    std::vector<uint32_t> kept;
    std::vector<NDTFeatureLink> gpu;
    try {
        gpu = getValidLinksGPU(graph, links, LinkGateParams(0.1, 1.0, 0.2, 2), &kept);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("linkgate_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    const std::vector<NDTFeatureLink> scalar = graph.getValidLinks(links, 0.1, 1.0, 0.2, 2);
    std::vector<char> on_gpu(links.size(), 0), on_host(links.size(), 0);
    for (uint32_t k : kept) on_gpu[k] = 1;
    {
        size_t s = 0;                                    // getValidLinks keeps the order: walk both lists
        for (size_t k = 0; k < links.size() && s < scalar.size(); k++)
            if (links[k].ref_idx == scalar[s].ref_idx && links[k].mov_idx == scalar[s].mov_idx && links[k].score == scalar[s].score) {
                on_host[k] = 1;
                s++;
            }
        CHECK(s == scalar.size(), "the scalar list is not a sub-sequence of the links");
    }
    size_t band = 0, differ = 0;
    for (size_t k = 0; k < links.size(); k++) {
        if (in_band(graph.getNode(links[k].mov_idx).T, graph.getNode(links[k].ref_idx).T * links[k].T, 1.0, 0.2, false)) {
            band++;
            continue;
        }
        differ += on_gpu[k] != on_host[k];
    }
    CHECK(differ == 0, "%zu links are kept by one of getValidLinksGPU / getValidLinks only", differ);
    CHECK(band * 1000 <= links.size(), "%zu of %zu links in the band", band, links.size());
    CHECK(gpu.size() == kept.size() && !kept.empty() && kept.size() < links.size(), "%zu kept", kept.size());
    for (size_t k = 0; k < kept.size(); k++)
        CHECK(gpu[k].ref_idx == links[kept[k]].ref_idx && gpu[k].mov_idx == links[kept[k]].mov_idx && (k == 0 || kept[k] > kept[k - 1]),
              "kept link %zu is not link %u", k, kept[k]);
    const size_t n_valid = kept.size();

    // ---- 2. computeCandidateLinks against the pair loop with distanceBetweenAffine3d -------------------------------------------
    LinkGateParams cp(0.1, 6.0, 0.6, 2, true);
    const std::vector<NDTFeatureLink> cand = computeCandidateLinks(graph, cp);
    size_t at = 0, cband = 0;
    double worst = 0;
    for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
            if ((int)j - (int)i < cp.min_idx_dist) continue;
            double dist, ang;
            distanceBetweenAffine3d(graph.getNode(i).T, graph.getNode(j).T, dist, ang);
            const bool hit = at < cand.size() && cand[at].ref_idx == i && cand[at].mov_idx == j;
            if (in_band(graph.getNode(i).T, graph.getNode(j).T, cp.max_dist, cp.max_angle, true)) {
                cband++;
                at += hit;
                continue;
            }
            const bool want = dist < cp.max_dist && ang < cp.max_angle;
            CHECK(hit == want, "pair (%zu, %zu): candidate %d, scalar %d", i, j, (int)hit, (int)want);
            if (hit) {
                const Eigen::Affine3d rel = graph.getNode(i).T.inverse() * graph.getNode(j).T;
                for (int e = 0; e < 16; e++) worst = std::max(worst, std::fabs(rel.data()[e] - cand[at].T.data()[e]));
                at++;
            }
        }
    CHECK(at == cand.size() && !cand.empty(), "%zu of %zu candidates are pairs of the loop, in its order", at, cand.size());
    CHECK(cband == 0, "%zu pairs in the band", cband);
    CHECK(worst < 1e-12 * 6.0, "T of a candidate is %.3g from T_i^-1 T_j", worst);

    // ---- 3. optimizeGraphGated against the loop of ndt_feature_graph_opt.cpp:152-173 written with the scalar getValidLinks -----
    const size_t m = 30;
    std::vector<Eigen::Affine3d> truth(m);
    PoseGraph a, b;
    for (size_t i = 0; i < m; i++) {
        const double ang = 2.0 * M_PI * (double)i / (double)m;
        truth[i] = ndtgpu_host::affine_from_pose(6.0 * std::cos(ang), 4.0 * std::sin(ang), 0, 0, 0, ang + 1.2);
        const Eigen::Affine3d start = i == 0 ? truth[0] : truth[i] * ndtgpu_host::affine_from_pose(0.01 * (double)i * nd(rng), 0.01 * (double)i * nd(rng), 0, 0, 0, 0.003 * (double)i * nd(rng));
        a.addNode(start);
        b.addNode(start);
    }
    std::vector<NDTFeatureLink> incremental, matched;
    for (size_t i = 0; i + 1 < m; i++) {
        NDTFeatureLink l(i, i + 1);
        l.T = truth[i].inverse() * truth[i + 1];
        l.score = -1.;                                   // getIncrementalLinks
        incremental.push_back(l);
    }
    for (size_t i = 0; i < m; i++)
        for (size_t j = i + 2; j < m; j++) {
            NDTFeatureLink l(i, j);
            const bool wrong = ud(rng) < 0.06;           // 30 % of the links are off by metres
            const double sxy = wrong ? 1.5 : 0.02, st = wrong ? 0.5 : 0.01;
            l.T = truth[i].inverse() * truth[j] * ndtgpu_host::affine_from_pose(sxy * nd(rng), sxy * nd(rng), 0, 0, 0, st * nd(rng));
            l.score = 0.6 * ud(rng);
            matched.push_back(l);
        }
    const std::vector<size_t> rounds = optimizeGraphGated(a, incremental, matched, LinkGateParams(), 8);
    std::vector<size_t> want_rounds;
    size_t prev = (size_t)-1;
    for (int round = 0; round < 8; round++) {
        b.clearAllLinks();
        b.appendLinks(incremental);
        const std::vector<NDTFeatureLink> v = b.getValidLinks(matched, 0.1, 1.0, 0.2, 2);
        want_rounds.push_back(v.size());
        if (v.empty()) break;
        b.appendLinks(v);
        optimizeGraphUsingISAM(b);
        if (prev == v.size()) break;
        prev = v.size();
    }
    CHECK(rounds == want_rounds && rounds.size() >= 2 && rounds.size() < 8, "%zu rounds against %zu", rounds.size(), want_rounds.size());
    CHECK(a.getNbLinks() == b.getNbLinks() && a.getNbLinks() == incremental.size() + rounds.back(), "%zu links against %zu", a.getNbLinks(), b.getNbLinks());
    int equal = 0;
    double off = 0;
    for (size_t i = 0; i < m; i++) {
        bool same = true;
        for (int e = 0; e < 16; e++) same = same && a.getNode(i).T.data()[e] == b.getNode(i).T.data()[e];
        CHECK(same, "node %zu: the gated loop differs from the scalar loop", i);
        equal += same ? 1 : 0;
        off = std::max(off, (a.getNode(i).T.translation() - truth[i].translation()).norm());
    }
    CHECK(off < 0.5, "a node ends %.3f m from the truth", off);
    std::printf("linkgate_demo: %zu of %zu links valid (%zu in the band), %zu candidates, %zu rounds of the gated loop ending with %zu links, "
                "%d of %zu nodes equal to the scalar loop bit for bit, %d failures\n",
                n_valid, links.size(), band, cand.size(), rounds.size(), rounds.back(), equal, m, g_fails);
    return g_fails ? 1 : 0;
}
