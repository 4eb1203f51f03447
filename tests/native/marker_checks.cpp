// marker_checks.cpp -- the marker export's shared header (csrc/ndt_marker.h) on the host, a plain g++ program with its own main, built
// with -fsanitize=address,undefined by tests/test_host_marker.py: the residuals of the eigen-pairs, the sign rule, the stable order,
// the count at the threshold, the pose, the segments of particles and links and the refused arguments.  Every input and output lives
// in a heap block of exactly the size a call may touch.
#include "../../ndt_feature_graph_amd/csrc/ndt_marker.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

static uint32_t g_seed = 12345u;
static double rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (double)(g_seed >> 8) / 16777216.0; }   // [0, 1)

// a rotation from three angles, row-major
static void rotation(double a, double b, double c, double R[9])
{
    const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b), cc = cos(c), sc = sin(c);
    const double r[9] = {cb * cc, -cb * sc, sb, ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -sa * cb, sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb};
    memcpy(R, r, sizeof r);
}

// R diag(lam) R^T as cov6, in a heap block of six doubles
static std::unique_ptr<double[]> cov_of(const double R[9], const double lam[3])
{
    std::unique_ptr<double[]> c(new double[6]);
    int k = 0;
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) {
            double v = 0.0;
            for (int e = 0; e < 3; e++) v += R[3 * i + e] * lam[e] * R[3 * j + e];
            c[k++] = v;
        }
    return c;
}

int main()
{
    // the eigen-pairs of 4000 random SPD matrices over six decades, every tenth with a degenerate pair
    size_t pairs = 0;
    double worst_res = 0.0, worst_unit = 0.0, worst_ortho = 0.0;
    for (int n = 0; n < 4000; n++) {
        double R[9], lam[3];
        rotation(6.28 * rnd(), 6.28 * rnd(), 6.28 * rnd(), R);
        for (int k = 0; k < 3; k++) lam[k] = pow(10.0, -6.0 + 6.0 * rnd());
        if (n % 10 == 0) lam[1] = lam[0];
        const std::unique_ptr<double[]> c = cov_of(R, lam);
        double ev[3], V[3][3];
        ndt_marker_eig3(c.get(), ev, V);
        const double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
        const double lmax = fmax(lam[0], fmax(lam[1], lam[2]));
        CHECK(ev[0] <= ev[1] && ev[1] <= ev[2], "ascending: %g %g %g", ev[0], ev[1], ev[2]);
        double sorted[3] = {lam[0], lam[1], lam[2]};
        for (int a = 0; a < 3; a++)
            for (int b = a + 1; b < 3; b++)
                if (sorted[b] < sorted[a]) { const double t = sorted[a]; sorted[a] = sorted[b]; sorted[b] = t; }
        for (int j = 0; j < 3; j++) {
            CHECK(fabs(ev[j] - sorted[j]) <= 1e-9 * lmax, "eigenvalue %d: %g against %g", j, ev[j], sorted[j]);
            double norm = 0.0, res = 0.0;
            for (int i = 0; i < 3; i++) {
                norm += V[i][j] * V[i][j];
                const double r = A[i][0] * V[0][j] + A[i][1] * V[1][j] + A[i][2] * V[2][j] - ev[j] * V[i][j];
                res += r * r;
            }
            worst_unit = fmax(worst_unit, fabs(sqrt(norm) - 1.0));
            worst_res = fmax(worst_res, sqrt(res) / lmax);
            for (int i = 0; i < j; i++) worst_ortho = fmax(worst_ortho, fabs(V[0][i] * V[0][j] + V[1][i] * V[1][j] + V[2][i] * V[2][j]));
            // the sign: the component of largest magnitude is positive, the lowest row where they tie
            int m = 0;
            if (fabs(V[1][j]) > fabs(V[m][j])) m = 1;
            if (fabs(V[2][j]) > fabs(V[m][j])) m = 2;
            CHECK(V[m][j] > 0.0, "the sign of vector %d", j);
            pairs++;
        }
    }
    CHECK(worst_unit <= 1e-12 && worst_res <= 1e-9 && worst_ortho <= 1e-9, "unit %g residual %g orthogonality %g", worst_unit, worst_res, worst_ortho);

    // the stable order: a diagonal matrix does not start the solver, and values that tie keep the diagonal's order
    {
        std::unique_ptr<double[]> c(new double[6]{0.02, 0.0, 0.0, 0.01, 0.0, 0.01});
        double ev[3], V[3][3];
        ndt_marker_eig3(c.get(), ev, V);
        CHECK(ev[0] == 0.01 && ev[1] == 0.01 && ev[2] == 0.02 && V[1][0] == 1.0 && V[2][1] == 1.0 && V[0][2] == 1.0 && V[0][0] == 0.0, "the order of a tie");
        // a tie of magnitudes inside a vector: (1, 1, 0) / sqrt 2 and (1, -1, 0) / sqrt 2 both lead with row 0
        std::unique_ptr<double[]> d(new double[6]{2.0, 1.0, 0.0, 2.0, 0.0, 5.0});
        ndt_marker_eig3(d.get(), ev, V);
        CHECK(fabs(ev[0] - 1.0) <= 1e-14 && fabs(ev[1] - 3.0) <= 1e-14 && ev[2] == 5.0, "eigenvalues %g %g %g", ev[0], ev[1], ev[2]);
        CHECK(V[0][0] > 0.0 && V[1][0] < 0.0 && V[0][1] > 0.0 && V[1][1] > 0.0 && V[2][2] == 1.0, "the sign where magnitudes tie");
    }

    // the count at the threshold, the compaction and the flag
    {
        std::unique_ptr<double[]> c(new double[6]{1e-4, 0.0, 0.0, 0.01, 0.0, 5e-5}), mean(new double[3]{0.5, -0.25, 0.125});
        std::unique_ptr<double[]> T12(new double[12]{0, -1, 0, 1, 0, 0, 0, 0, 1, 10, 20, 30});       // a quarter turn about z, then (10, 20, 30)
        double seg[3][2][3], ev[3], T[12];
        memcpy(T, T12.get(), sizeof T);
        uint32_t flags = 0;
        uint32_t n = ndt_marker_cell(mean.get(), c.get(), false, T, 1e-4, seg, flags, ev);
        CHECK(n == 2 && flags == 0 && ev[0] == 5e-5 && ev[1] == 1e-4 && ev[2] == 0.01, "the threshold itself is emitted: %u segments", n);
        CHECK(seg[0][0][0] == 0.5 - sqrt(1e-4) && seg[0][1][0] == 0.5 + sqrt(1e-4) && seg[0][0][1] == -0.25 && seg[1][0][1] == -0.25 - sqrt(0.01) &&
                  seg[1][1][2] == 0.125, "the segments of a diagonal cell");
        uint32_t f2 = 0;
        CHECK(ndt_marker_cell_count(c.get(), 1e-4, f2) == 2 && ndt_marker_cell_count(c.get(), nextafter(1e-4, 1.0), f2) == 1 &&
                  ndt_marker_cell_count(c.get(), 0.0, f2) == 3 && ndt_marker_cell_count(c.get(), 1.0, f2) == 0 && f2 == 0, "the count");
        n = ndt_marker_cell(mean.get(), c.get(), true, T, 1e-4, seg, flags, ev);
        // (x, y, z) -> (-y + 10, x + 20, z + 30)
        CHECK(n == 2 && seg[0][0][0] == 0.25 + 10 && seg[0][0][1] == (0.5 - sqrt(1e-4)) + 20 && seg[0][1][2] == 0.125 + 30, "the pose");
        std::unique_ptr<double[]> bad(new double[6]{NAN, 0.0, 0.0, 0.01, 0.0, INFINITY});
        n = ndt_marker_cell(mean.get(), bad.get(), false, T, 1e-4, seg, flags, ev);
        CHECK(n == 1 && flags == NDTGPU_MARKER_NONFINITE && seg[0][1][1] == -0.25 + sqrt(0.01), "a value that is not finite: %u segments, flags %u", n, flags);
        f2 = 0;
        CHECK(ndt_marker_cell_count(bad.get(), 1e-4, f2) == 1 && f2 == NDTGPU_MARKER_NONFINITE, "... counted the same");
        // count and emit agree on every matrix of the first loop's kind
        g_seed = 99u;
        for (int k = 0; k < 500; k++) {
            double R[9], lam[3];
            rotation(6.28 * rnd(), 6.28 * rnd(), 6.28 * rnd(), R);
            for (int e = 0; e < 3; e++) lam[e] = pow(10.0, -5.0 + 2.0 * rnd());
            const std::unique_ptr<double[]> cc = cov_of(R, lam);
            uint32_t fa = 0, fb = 0;
            CHECK(ndt_marker_cell(mean.get(), cc.get(), true, T, 1e-4, seg, fa, ev) == ndt_marker_cell_count(cc.get(), 1e-4, fb), "count and emit");
        }
    }

    // the pose from a column-major 4 x 4, a particle and a link
    {
        std::unique_ptr<double[]> T16(new double[32]);
        for (int k = 0; k < 32; k++) T16[k] = 0.0;
        const double R[9] = {0.6, -0.8, 0.0, 0.8, 0.6, 0.0, 0.0, 0.0, 1.0};
        for (int n = 0; n < 2; n++) {
            for (int i = 0; i < 3; i++)
                for (int k = 0; k < 3; k++) T16[16 * n + 4 * k + i] = R[3 * i + k];
            T16[16 * n + 12] = 1.0 + n; T16[16 * n + 13] = 2.0 + n; T16[16 * n + 14] = 3.0 + n; T16[16 * n + 15] = 1.0;
        }
        double T12[12];
        ndt_marker_pose12(T16.get(), T12);
        CHECK(T12[1] == -0.8 && T12[3] == 0.8 && T12[9] == 1.0 && T12[11] == 3.0, "pose12");
        std::unique_ptr<double[]> seg6(new double[6]);
        ndt_marker_particle(T12, 0.3, seg6.get());
        CHECK(seg6[0] == 1.0 && seg6[1] == 2.0 && seg6[2] == 3.0 && seg6[3] == 0.6 * 0.3 + 1.0 && seg6[4] == 0.8 * 0.3 + 2.0 && seg6[5] == 3.0, "a particle");
        ndt_marker_link(T16.get(), 1, 0, seg6.get());
        CHECK(seg6[0] == 2.0 && seg6[2] == 4.0 && seg6[3] == 1.0 && seg6[5] == 3.0, "a link");
        std::unique_ptr<double[]> score(new double[3]{0.5, -0.5, -0.0});
        CHECK(ndt_marker_link_kept(score.get(), 0, 1) && !ndt_marker_link_kept(score.get(), 1, 1) && ndt_marker_link_kept(score.get(), 1, 0) &&
                  ndt_marker_link_kept(score.get(), 2, 1) && ndt_marker_link_kept(nullptr, 1, 1), "links kept");
        CHECK(!ndt_marker_link_bad(1, 0, 2) && ndt_marker_link_bad(2, 0, 2) && ndt_marker_link_bad(0, 2, 2) && ndt_marker_link_bad(0, 0, 0), "bad indices");
        CHECK(ndt_marker_tiles(0) == 0 && ndt_marker_tiles(256) == 1 && ndt_marker_tiles(257) == 2, "tiles");
    }

    // the refused arguments
    {
        ndtgpu_marker_params p;
        memset(&p, 0, sizeof p);
        p.min_eval = 1e-4;
        p.particle_length = 0.3;
        int refused = 0, tried = 0;
#define REFUSED(expr)                                                        \
    do {                                                                     \
        tried++;                                                             \
        if ((expr) != nullptr) refused++; else std::printf("not refused: %s\n", #expr); \
    } while (0)
        CHECK(ndt_marker_check(8, 1000, 8, 2, 3, 1000, 40, 300, 5000, p) == nullptr, "a good call: %s", ndt_marker_check(8, 1000, 8, 2, 3, 1000, 40, 300, 5000, p));
        CHECK(ndt_marker_check(1, 0, 1, 1, 0, 1, 0, 0, 0, p) == nullptr, "an empty call");
        REFUSED(ndt_marker_check(0, 1000, 8, 2, 3, 1000, 40, 300, 5000, p));
        REFUSED(ndt_marker_check((1u << 20) + 1, 1000, 8, 2, 3, 1000, 40, 300, 5000, p));
        REFUSED(ndt_marker_check(8, (1u << 28) + 1, 8, 2, 3, 1000, 40, 300, 5000, p));
        REFUSED(ndt_marker_check(8, 1000, 8, 9, 0, 1000, 40, 300, 5000, p));
        REFUSED(ndt_marker_check(8, 1000, 8, 6, 3, 1000, 40, 300, 5000, p));
        REFUSED(ndt_marker_check(8, 1000, 20, 0, 9, 1000, 40, 300, 5000, p));
        REFUSED(ndt_marker_check(8, 1000, 8, 2, 3, 1000, 40, 300, 1ull << 32, p));
        REFUSED(ndt_marker_check(1u << 20, 1000, 1u << 20, 0, 1u << 20, 1u << 20, 40, 300, 5000, p));
        REFUSED(ndt_marker_check(8, 1000, 8, 2, 3, 1000, 1ull << 32, 300, 5000, p));
        REFUSED(ndt_marker_check(8, 1000, 8, 2, 3, 1000, 40, 1001, 5000, p));
        ndtgpu_marker_params q = p;
        q.min_eval = -1e-12;
        REFUSED(ndt_marker_check_params(q));
        q.min_eval = NAN;
        REFUSED(ndt_marker_check_params(q));
        q.min_eval = INFINITY;
        REFUSED(ndt_marker_check_params(q));
        q = p;
        q.particle_length = NAN;
        REFUSED(ndt_marker_check_params(q));
        q.particle_length = -INFINITY;
        REFUSED(ndt_marker_check_params(q));
        q = p;
        q.skip_negative = 2;
        REFUSED(ndt_marker_check_params(q));
        q.skip_negative = -1;
        REFUSED(ndt_marker_check_params(q));
        q = p;
        q.particle_length = -0.3;
        q.min_eval = 0.0;
        q.skip_negative = 1;
        CHECK(ndt_marker_check_params(q) == nullptr, "a negative length, a zero threshold and skip_negative are fine");
        std::printf("marker_checks: %zu eigen-pairs, unit %.1e residual %.1e orthogonality %.1e, %d of %d bad arguments refused, %d failures\n", pairs,
                    worst_unit, worst_res, worst_ortho, refused, tried, g_fails);
        CHECK(refused == tried, "refusals");
    }
    return g_fails ? 1 : 0;
}
