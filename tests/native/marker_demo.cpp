// marker_demo.cpp -- the host mirror's marker functions (host/ndt_rviz_gpu.h) called the way the reference's publish timers call
// ndt_rviz.h and ndt_feature_rviz.h (ndt_feature2d_fuser.cpp:425-433, 448-454, ndt_feature_mcl_node.cpp:274, 287): markerNDTCells of
// a map with and without a pose and markerNDTCells2 against the reference's own loop over getAllCells() / getEvals() / getEvecs()
// typed out on the host, markerParticlesNDTMCL3D against pf.pcloud, and markerNDTFeatureLinks of a small graph with and without
// skipOdom -- all bit for bit.  Exit code 0 = every check passed; without a GPU the library fails loudly (exit code 3).
//
//   marker_demo <cells.bin> <points.bin>: the cells of the file (doubles: n, has_pose, n x 3 means, n x 9 covariances, 16 of the
//   column-major pose) are installed in the map instead, and the points of markerNDTCells(map, pose, id, name) are written out as
//   doubles (tests/test_gpu_marker.py compares them with the library's).
#include "ndt_rviz_gpu.h"

#include <cstdio>
#include <cstring>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using ndt_visualisation::MarkerGPU;
using ndt_visualisation::PointGPU;

// ndt_rviz.h:1127-1153 typed out against the mirror's cells: the loop the device call replaces
static std::vector<PointGPU> reference_loop(lslgeneric::NDTMap &map, const Eigen::Affine3d *pose)
{
    std::vector<PointGPU> out;
    std::vector<lslgeneric::NDTCell *> cells = map.getAllCells();
    for (size_t i = 0; i < cells.size(); i++) {
        if (!cells[i]->hasGaussian_) continue;
        const Eigen::Vector3d mean = cells[i]->getMean();
        const Eigen::Matrix3d evecs = cells[i]->getEvecs();
        const Eigen::Vector3d evals = cells[i]->getEvals();
        for (int j = 0; j < 3; j++) {
            double scale = evals(j);
            if (scale < 0.0001) continue;
            scale = std::sqrt(scale);
            const Eigen::Vector3d offset(evecs(0, j) * scale, evecs(1, j) * scale, evecs(2, j) * scale);
            Eigen::Vector3d p1 = mean - offset, p2 = mean + offset;
            if (pose) {
                p1 = (*pose) * p1;
                p2 = (*pose) * p2;
            }
            out.push_back(PointGPU{p1(0), p1(1), p1(2)});
            out.push_back(PointGPU{p2(0), p2(1), p2(2)});
        }
    }
    for (lslgeneric::NDTCell *c : cells) delete c;
    return out;
}

static size_t differing(const std::vector<PointGPU> &a, const std::vector<PointGPU> &b)
{
    if (a.size() != b.size()) return a.size() > b.size() ? a.size() : b.size();
    size_t n = 0;
    for (size_t k = 0; k < a.size(); k++) n += std::memcmp(&a[k], &b[k], sizeof(PointGPU)) != 0;
    return n;
}

// a graph of poses and links over the interfaces markerNDTFeatureLinks reads
struct DemoNode : ndt_feature::NDTFeatureNodeInterface {
    Eigen::Affine3d T;
    Eigen::Matrix3d C;
    const Eigen::Affine3d &getPose() const override { return T; }
    const Eigen::Matrix3d &getCov() const override { return C; }
    void setPose(const Eigen::Affine3d &pose) override { T = pose; }
    void setCov(const Eigen::Matrix3d &cov) override { C = cov; }
};
struct DemoGraph : ndt_feature::NDTFeatureGraphInterface {
    std::vector<DemoNode> nodes;
    std::vector<ndt_feature::NDTFeatureLink> links;
    size_t getNbNodes() const override { return nodes.size(); }
    ndt_feature::NDTFeatureNodeInterface &getNodeInterface(size_t idx) override { return nodes[idx]; }
    const ndt_feature::NDTFeatureNodeInterface &getNodeInterface(size_t idx) const override { return nodes[idx]; }
    size_t getNbLinks() const override { return links.size(); }
    ndt_feature::NDTFeatureLinkInterface &getLinkInterface(size_t idx) override { return links[idx]; }
    const ndt_feature::NDTFeatureLinkInterface &getLinkInterface(size_t idx) const override { return links[idx]; }
};

static bool read_doubles(const char *path, std::vector<double> &v)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(double));
    const size_t got = std::fread(v.data(), sizeof(double), v.size(), f);
    std::fclose(f);
    return got == v.size();
}

int main(int argc, char **argv)
{
    const double res = 0.5;
    lslgeneric::NDTMap map(new lslgeneric::LazyGrid(res));
    try {
        map.guessSize(0, 0, 0, 12.5, 10.0, 1.0);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("marker_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    try {
        Eigen::Affine3d pose = ndtgpu_host::affine_from_pose(1.25, -0.75, 0.2, 0.4, 0.0, 0.3);
        std::vector<double> mean, cov;
        if (argc == 3) {
            std::vector<double> in;
            if (!read_doubles(argv[1], in) || in.size() < 2 || in.size() != 2 + 12 * (size_t)in[0] + 16) {
                std::printf("marker_demo: cannot read %s\n", argv[1]);
                return 1;
            }
            const size_t n = (size_t)in[0];
            mean.assign(in.begin() + 2, in.begin() + 2 + 3 * n);
            cov.assign(in.begin() + 2 + 3 * n, in.begin() + 2 + 12 * n);
            std::memcpy(pose.data(), &in[2 + 12 * n], 16 * sizeof(double));
        } else {
            // 300 cells (a tile of 256 and one of 44) on three of every five columns of the layer z = 0: rotated Gaussians of three sizes, every
            // fifth one flat (an axis below the threshold), every seventh one tiny (no axis above it)
            std::mt19937 rng(3);
            std::uniform_real_distribution<double> u(-1.0, 1.0);
            for (int k = 0; k < 300; k++) {
                const int slot = 5 * k / 3, ix = slot / 20, iy = slot % 20;
                const double c[3] = {(ix - 12) * res + 0.1 * u(rng), (iy - 10) * res + 0.1 * u(rng), 0.1 * u(rng)};
                const Eigen::Affine3d R = ndtgpu_host::affine_from_pose(0, 0, 0, u(rng), u(rng), 3.0 * u(rng));
                const double s = k % 7 == 6 ? 1e-3 : 1.0;
                const double lam[3] = {0.04 * s, 0.01 * s, (k % 5 == 4 ? 2e-5 : 2.5e-3) * s};
                for (int a = 0; a < 3; a++) mean.push_back(c[a]);
                double C[9];
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b <= a; b++) {
                        double v = 0.0;
                        for (int e = 0; e < 3; e++) v += R(a, e) * lam[e] * R(b, e);
                        C[3 * a + b] = C[3 * b + a] = v;
                    }
                cov.insert(cov.end(), C, C + 9);
            }
        }
        const size_t n_cells = mean.size() / 3;
        ndtgpu_host::check(ndtgpu_mapset_set_cells(map.handle(), map.slot(), mean.data(), cov.data(), n_cells), "ndtgpu_mapset_set_cells");

        const MarkerGPU posed = ndt_visualisation::markerNDTCells(map, pose, 4, "node");
        if (argc == 3) {
            FILE *f = std::fopen(argv[2], "wb");
            if (!f || std::fwrite(posed.points.data(), sizeof(PointGPU), posed.points.size(), f) != posed.points.size()) {
                std::printf("marker_demo: cannot write %s\n", argv[2]);
                return 1;
            }
            std::fclose(f);
            std::printf("marker_demo: %zu cells, %zu points written\n", n_cells, posed.points.size());
            return 0;
        }

        // the cells: against the reference's loop on the host
        CHECK((size_t)map.numberOfActiveCells() == n_cells, "%d cells installed", map.numberOfActiveCells());
        const MarkerGPU plain = ndt_visualisation::markerNDTCells(map, 1, "NDTMap");
        const std::vector<PointGPU> want_plain = reference_loop(map, nullptr), want_posed = reference_loop(map, &pose);
        CHECK(plain.type == MarkerGPU::LINE_LIST && plain.scale_x == 0.02 && plain.id == 1 && plain.ns == "NDTMap" && plain.frame_id == "/world" &&
                  plain.lifetime == 60.0 && plain.color[0] == 0.0 && plain.color[1] == 1.0 && plain.color[2] == 0.0 && plain.color[3] == 0.3,
              "the marker's constants");
        CHECK(differing(plain.points, want_plain) == 0, "markerNDTCells(map, id, name): %zu of %zu points differ from the loop's %zu",
              differing(plain.points, want_plain), plain.points.size(), want_plain.size());
        CHECK(differing(posed.points, want_posed) == 0, "markerNDTCells(map, pose, id, name): %zu of %zu points differ", differing(posed.points, want_posed),
              posed.points.size());
        CHECK(posed.color[0] == 0.0 && posed.color[1] == 1.0 && posed.id == 4 && posed.ns == "node", "id 4 is green");
        CHECK(plain.points.size() == posed.points.size() && plain.points.size() > 2 * n_cells && plain.points.size() < 6 * n_cells,
              "%zu points of %zu cells: some axes are below the threshold", plain.points.size(), n_cells);
        MarkerGPU twice;
        ndt_visualisation::markerNDTCells2(map, pose, -1, "a", twice);
        ndt_visualisation::markerNDTCells2(map, pose, -1, "a", twice);
        CHECK(twice.points.size() == 2 * posed.points.size() && twice.color[0] == 1.0 && twice.color[3] == 1.0 &&
                  std::memcmp(&twice.points[posed.points.size()], posed.points.data(), posed.points.size() * sizeof(PointGPU)) == 0,
              "markerNDTCells2 appends");
        // getEvals / getEvecs: ascending, unit, the largest component positive
        {
            lslgeneric::NDTCell c;
            Eigen::Matrix3d C;
            C(0, 0) = 0.02; C(1, 1) = 0.01; C(2, 2) = 0.01;
            c.setCov(C);
            const Eigen::Vector3d ev = c.getEvals();
            const Eigen::Matrix3d E = c.getEvecs();
            CHECK(ev(0) == 0.01 && ev(1) == 0.01 && ev(2) == 0.02 && E(1, 0) == 1.0 && E(2, 1) == 1.0 && E(0, 2) == 1.0, "a tie keeps the diagonal's order");
        }

        // the particles
        NDTMCL3D mcl(res, map, -5);
        mcl.scan_size[0] = 12.5; mcl.scan_size[1] = 10.0; mcl.scan_size[2] = 1.0;
        mcl.max_scan_cells = 1000;
        mcl.initializeFilter(0.2, -0.1, 0, 0, 0, 0.05, 0.5, 0.5, 0.1, 0.03, 0.03, 0.03, 300);
        const MarkerGPU pm = ndt_visualisation::markerParticlesNDTMCL3D(mcl, -1, "particles");
        size_t bad = 0;
        for (size_t i = 0; i < mcl.pf.size() && 2 * i + 1 < pm.points.size(); i++) {
            const Eigen::Affine3d &T = mcl.pf.pcloud[i].T;
            const Eigen::Vector3d t = T.translation(), p2 = T * Eigen::Vector3d(0.3, 0., 0.);
            const PointGPU a{t(0), t(1), t(2)}, b{p2(0), p2(1), p2(2)};
            bad += std::memcmp(&a, &pm.points[2 * i], sizeof a) != 0 || std::memcmp(&b, &pm.points[2 * i + 1], sizeof b) != 0;
        }
        CHECK(pm.points.size() == 600 && bad == 0 && pm.scale_x == 0.005 && pm.color[0] == 0.6 && pm.color[2] == 0.8,
              "markerParticlesNDTMCL3D: %zu points, %zu particles differ", pm.points.size(), bad);

        // the links
        DemoGraph g;
        g.nodes.resize(12);
        for (size_t i = 0; i < g.nodes.size(); i++) g.nodes[i].T = ndtgpu_host::affine_from_pose(0.7 * (double)i, 0.1 * (double)(i * i), 0.0, 0, 0, 0.2 * (double)i);
        for (size_t i = 0; i + 1 < g.nodes.size(); i++) {
            ndt_feature::NDTFeatureLink l(i, i + 1);
            l.score = -1.0;                     // (the incremental links' score, graph.cpp:180-204)
            g.links.push_back(l);
        }
        for (size_t i = 0; i + 4 < g.nodes.size(); i += 2) {
            ndt_feature::NDTFeatureLink l(i, i + 4);
            l.score = 0.05;
            g.links.push_back(l);
        }
        const MarkerGPU all = ndt_feature::markerNDTFeatureLinks(g, 0, 1, "links", false), closures = ndt_feature::markerNDTFeatureLinks(g, 0, 1, "links", true);
        CHECK(all.points.size() == 2 * g.links.size() && closures.points.size() == 2 * 4 && all.color[0] == 1.0 && all.color[1] == 0.65 && all.scale_x == 0.02,
              "links: %zu and %zu points", all.points.size(), closures.points.size());
        bad = 0;
        for (size_t i = 0; i < g.links.size() && 2 * i + 1 < all.points.size(); i++) {
            const Eigen::Vector3d a = g.nodes[g.links[i].ref_idx].T.translation(), b = g.nodes[g.links[i].mov_idx].T.translation();
            bad += !(all.points[2 * i].x == a(0) && all.points[2 * i].y == a(1) && all.points[2 * i + 1].x == b(0) && all.points[2 * i + 1].y == b(1));
        }
        CHECK(bad == 0 && closures.points[0].x == 0.0 && closures.points[1].x == g.nodes[4].T.translation()(0), "links: %zu differ", bad);
        g.links[3].mov_idx = 12;
        bool refused = false;
        try {
            ndt_feature::markerNDTFeatureLinks(g, 0, 1, "links", false);
        } catch (const ndtgpu_host::Error &e) {
            refused = e.status == NDTGPU_ERR_INVALID;
        }
        CHECK(refused, "a link to a node that is none is refused");
        std::printf("marker_demo: %zu cells, %zu cell points, %zu particle points, %zu + %zu link points, %d failures\n", n_cells, plain.points.size(),
                    pm.points.size(), all.points.size(), closures.points.size(), g_fails);
    } catch (const ndtgpu_host::Error &e) {
        if (e.status == NDTGPU_ERR_NO_DEVICE) {
            std::printf("marker_demo: no HIP device: %s (no CPU fallback)\n", e.what());
            return 3;
        }
        std::printf("marker_demo: %s\n", e.what());
        return 1;
    }
    return g_fails ? 1 : 0;
}
