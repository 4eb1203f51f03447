// ndt_marker.h -- what the marker export's kernels (csrc/ndt_marker.hip), its C-ABI (csrc/ndtgpu_marker.hip) and host programs share
// (include/ndtgpu.h "marker export"): the eigen-pairs of a cell's covariance, the axis segments of a cell, the segment of a link
// and of a particle, and the checks of a call's arguments.  Plain C++ for host and device: NDT_HD is __host__ __device__ under hipcc
// and `inline` elsewhere, so tests/native/marker_checks.cpp compiles this file with g++ alone (under the address and
// undefined-behaviour sanitizers).  tests/marker_model.py restates all of it in NumPy.
//
// THE ORDER OF OPERATIONS, part of the contract: every fp64 expression below is evaluated as written, NOT contracted (no fused
// multiply-add); the only operations are + - * /, sqrt and fabs.
//   matrix     a = the symmetric 3 x 3 of cov6 = (xx xy xz yy yz zz); v = the identity
//   sweep      at most 64 times: off = ((a01^2 + a02^2) + a12^2), diag = ((a00^2 + a11^2) + a22^2), each sum from 0.0 in that order;
//              stop where off == 0 or off <= 1e-30 * diag; else the pairs (p, q) = (0, 1), (0, 2), (1, 2) in turn
//   pair       skipped where apq == 0; theta = (aqq - app) / (2.0 * apq); t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta *
//              theta + 1.0)); c = 1.0 / sqrt(t * t + 1.0); s = t * c; then, for k = 0, 1, 2, the columns (akp, akq) <- (c * akp - s * akq,
//              s * akp + c * akq), then the rows (apk, aqk) <- (c * apk - s * aqk, s * apk + c * aqk), then the columns of v like those of a
//   order      the diagonal (a00, a11, a22) with its columns of v through the exchanges (0, 1), (1, 2), (0, 1), each made iff the later
//              value < the earlier one: ascending, and values that tie (or do not compare) keep the diagonal's order
//   sign       per column: m = the row of the largest fabs, the lowest row where they tie; the column is negated iff its entry in
//              row m is < 0
//   axis j     of a cell, j = 0, 1, 2 over the ordered eigenvalues: nothing and NDTGPU_MARKER_NONFINITE where !(fabs(lambda_j) <=
//              DBL_MAX); nothing where lambda_j < min_eval; else r = sqrt(lambda_j), o_k = v_kj * r, p1 = mean - o, p2 = mean + o
//   pose       R (row-major 3 x 3) and t from the upper three rows of a column-major 4 x 4: R_ik = T16[4 k + i], t_i = T16[12 + i];
//              a point is ((R_i0 * p0 + R_i1 * p1) + R_i2 * p2) + t_i
//   particle   (t, T * (length, 0, 0)) through the same expression;  link: (t of pose[ref], t of pose[mov]), copies
#pragma once
#include "../../include/ndtgpu.h"

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include "ndt_common.h"   // NDT_HD
#elif !defined(NDT_HD)
#define NDT_HD inline
#endif

#define NDT_MARKER_THREADS 256                    // a workgroup of every kernel
#define NDT_MARKER_WAVES (NDT_MARKER_THREADS / 64)
#define NDT_MARKER_TILE NDT_MARKER_THREADS        // cells, links or particles of a workgroup
#define NDT_MARKER_MAX_MAPS (1u << 20)            // maps of a call
#define NDT_MARKER_MAX_LINKS (1u << 28)
#define NDT_MARKER_MAX_TILES 0x500000u            // of a call: 768 segments a tile stay below 2^32
#define NDT_MARKER_MAX_CAPACITY 0xFFFFFFFFull
#define NDT_MARKER_SWEEPS 64

// one rotation of the cyclic Jacobi in the plane (P, Q): every index is a constant, so the matrices live in registers
template <int P, int Q>
NDT_HD void ndt_marker_rotate(double (&a)[3][3], double (&v)[3][3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double apq = a[P][Q];
    if (apq != 0.0) {
        const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double akp = a[k][P], akq = a[k][Q];
            a[k][P] = c * akp - s * akq;
            a[k][Q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double apk = a[P][k], aqk = a[Q][k];
            a[P][k] = c * apk - s * aqk;
            a[Q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double vkp = v[k][P], vkq = v[k][Q];
            v[k][P] = c * vkp - s * vkq;
            v[k][Q] = s * vkp + c * vkq;
        }
    }
}

// value I and its column of v behind value J and its column iff the later value is the smaller one
template <int I, int J>
NDT_HD void ndt_marker_exchange(double (&d)[3], double (&v)[3][3])
{
    if (d[J] < d[I]) {
        const double x = d[I];
        d[I] = d[J];
        d[J] = x;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double y = v[k][I];
            v[k][I] = v[k][J];
            v[k][J] = y;
        }
    }
}

// The eigen-pairs of the symmetric matrix cov6 = (xx xy xz yy yz zz): evals ascending (ties in the order of the Jacobi's diagonal),
// column j of V the unit eigenvector of evals[j], its component of largest magnitude positive.
NDT_HD void ndt_marker_eig3(const double cov6[6], double (&evals)[3], double (&V)[3][3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double a[3][3] = {{cov6[0], cov6[1], cov6[2]}, {cov6[1], cov6[3], cov6[4]}, {cov6[2], cov6[4], cov6[5]}};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < NDT_MARKER_SWEEPS; sweep++) {
        double off = 0.0, diag = 0.0;
        off += a[0][1] * a[0][1];
        off += a[0][2] * a[0][2];
        off += a[1][2] * a[1][2];
        diag += a[0][0] * a[0][0];
        diag += a[1][1] * a[1][1];
        diag += a[2][2] * a[2][2];
        if (off == 0.0 || off <= 1e-30 * diag) break;
        ndt_marker_rotate<0, 1>(a, V);
        ndt_marker_rotate<0, 2>(a, V);
        ndt_marker_rotate<1, 2>(a, V);
    }
    evals[0] = a[0][0];
    evals[1] = a[1][1];
    evals[2] = a[2][2];
    ndt_marker_exchange<0, 1>(evals, V);
    ndt_marker_exchange<1, 2>(evals, V);
    ndt_marker_exchange<0, 1>(evals, V);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double m0 = fabs(V[0][j]), m1 = fabs(V[1][j]), m2 = fabs(V[2][j]);
        double lead = V[0][j], big = m0;
        if (m1 > big) { lead = V[1][j]; big = m1; }
        if (m2 > big) { lead = V[2][j]; big = m2; }
        if (lead < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; k++) V[k][j] = -V[k][j];
        }
    }
}

// a pose as the kernels hold it: R row-major, then t (the layout of `rigid`, csrc/ndt_math.h)
NDT_HD void ndt_marker_pose12(const double T16[16], double (&T12)[12])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 3; k++) T12[3 * i + k] = T16[4 * k + i];
        T12[9 + i] = T16[12 + i];
    }
}

// R p + t, evaluated as written
NDT_HD void ndt_marker_point(const double (&T12)[12], const double (&p)[3], double *out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = ((T12[3 * i] * p[0] + T12[3 * i + 1] * p[1]) + T12[3 * i + 2] * p[2]) + T12[9 + i];
}

// does axis `lambda` of a cell give a segment; a value that is not finite raises the flag
NDT_HD bool ndt_marker_axis_kept(double lambda, double min_eval, uint32_t &flags)
{
    if (!(fabs(lambda) <= DBL_MAX)) {
        flags |= NDTGPU_MARKER_NONFINITE;
        return false;
    }
    return !(lambda < min_eval);
}

// the segments of one cell, compacted: seg[n][0] = p1, seg[n][1] = p2 of the n-th kept axis; posed: the map has the pose T12 (else T12
// is not read).  Rows at and behind the count are axes that were not kept: not part of the result.
NDT_HD uint32_t ndt_marker_cell(const double mean[3], const double cov6[6], bool posed, const double (&T12)[12], double min_eval,
                                double (&seg)[3][2][3], uint32_t &flags, double (&evals)[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double V[3][3];
    ndt_marker_eig3(cov6, evals, V);
    bool kept[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        kept[j] = ndt_marker_axis_kept(evals[j], min_eval, flags);
        const double r = sqrt(evals[j]);
        double p1[3], p2[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double o = V[k][j] * r;
            p1[k] = mean[k] - o;
            p2[k] = mean[k] + o;
        }
        if (posed) {
            ndt_marker_point(T12, p1, seg[j][0]);
            ndt_marker_point(T12, p2, seg[j][1]);
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                seg[j][0][k] = p1[k];
                seg[j][1][k] = p2[k];
            }
        }
    }
    // the kept axes to the front, in order: every index is a constant (selects, no addressing)
    const int s0 = kept[0] ? 0 : (kept[1] ? 1 : 2), s1 = (kept[0] && kept[1]) ? 1 : 2;
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double a0 = seg[0][e][k], a1 = seg[1][e][k], a2 = seg[2][e][k];
            seg[0][e][k] = s0 == 0 ? a0 : (s0 == 1 ? a1 : a2);
            seg[1][e][k] = s1 == 1 ? a1 : a2;
        }
    return (kept[0] ? 1u : 0u) + (kept[1] ? 1u : 0u) + (kept[2] ? 1u : 0u);
}

// the number of segments of one cell: what ndt_marker_cell returns, by the same eigen-solver
NDT_HD uint32_t ndt_marker_cell_count(const double cov6[6], double min_eval, uint32_t &flags)
{
    double evals[3], V[3][3];
    ndt_marker_eig3(cov6, evals, V);
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) n += ndt_marker_axis_kept(evals[j], min_eval, flags) ? 1u : 0u;
    return n;
}

// the segment of a particle: its position, and the point `length` along its x axis
NDT_HD void ndt_marker_particle(const double (&T12)[12], double length, double *seg6)
{
    const double tip[3] = {length, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; k++) seg6[k] = T12[9 + k];
    ndt_marker_point(T12, tip, seg6 + 3);
}

// a link: kept unless its score is negative and those are skipped; its node indices must be nodes
NDT_HD bool ndt_marker_link_kept(const double *score, size_t i, int skip_negative) { return !(skip_negative && score && score[i] < 0.0); }
NDT_HD bool ndt_marker_link_bad(uint32_t ref, uint32_t mov, uint32_t n_nodes) { return ref >= n_nodes || mov >= n_nodes; }
// ... its segment: the translations of its two nodes' column-major poses
NDT_HD void ndt_marker_link(const double *T16_nodes, uint32_t ref, uint32_t mov, double *seg6)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        seg6[k] = T16_nodes[16 * (size_t)ref + 12 + k];
        seg6[3 + k] = T16_nodes[16 * (size_t)mov + 12 + k];
    }
}

NDT_HD size_t ndt_marker_tiles(size_t n) { return (n + NDT_MARKER_TILE - 1) / NDT_MARKER_TILE; }

// ---- checks: NULL: fine, else the message (it names the argument) ---------------------------------------------------------------
inline const char *ndt_marker_check_params(const ndtgpu_marker_params &p)
{
    if (!(p.min_eval >= 0.0 && p.min_eval < 1e150)) return "min_eval must be finite and >= 0";
    if (!(std::fabs(p.particle_length) < 1e150)) return "particle_length must be finite";
    if (p.skip_negative != 0 && p.skip_negative != 1) return "skip_negative must be 0 or 1";
    return nullptr;
}
inline const char *ndt_marker_check_handle(size_t max_maps_per_call, size_t max_links)
{
    if (max_maps_per_call == 0 || max_maps_per_call > NDT_MARKER_MAX_MAPS) return "max_maps_per_call must be 1 .. 2^20";
    if (max_links > NDT_MARKER_MAX_LINKS) return "max_links must be 0 .. 2^28";
    return nullptr;
}
// maps [first, first + count) of a set of n_maps maps of max_cells cells each, into `capacity` segments
inline const char *ndt_marker_check_maps(size_t n_maps, size_t first, size_t count, size_t max_cells, unsigned long long capacity)
{
    if (first > n_maps || count > n_maps - first) return "maps [first, first + count) out of range";
    if (count > NDT_MARKER_MAX_MAPS) return "count must be 0 .. 2^20";
    if (capacity > NDT_MARKER_MAX_CAPACITY) return "capacity must be 0 .. 2^32 - 1";
    if ((unsigned long long)count * ndt_marker_tiles(max_cells) > NDT_MARKER_MAX_TILES) return "count * tiles of a map: more than 5 * 2^20 tiles";
    return nullptr;
}
inline const char *ndt_marker_check_links(size_t n_nodes, size_t n_links, unsigned long long capacity)
{
    if (n_nodes > 0xFFFFFFFFull) return "n_nodes must be 0 .. 2^32 - 1";
    if (n_links > NDT_MARKER_MAX_LINKS) return "n_links must be 0 .. 2^28";
    if (capacity > NDT_MARKER_MAX_CAPACITY) return "capacity must be 0 .. 2^32 - 1";
    return nullptr;
}
// everything at once (ndtgpu_marker_check): a handle's sizes, a cell call and a link call on plain numbers
inline const char *ndt_marker_check(size_t max_maps_per_call, size_t max_links, size_t n_maps, size_t first, size_t count, size_t max_cells,
                                    size_t n_nodes, size_t n_links, unsigned long long capacity, const ndtgpu_marker_params &p)
{
    const char *bad = ndt_marker_check_handle(max_maps_per_call, max_links);
    if (!bad) bad = ndt_marker_check_params(p);
    if (!bad) bad = ndt_marker_check_maps(n_maps, first, count, max_cells, capacity);
    if (!bad && count > max_maps_per_call) bad = "count: more maps than the handle was created for";
    if (!bad) bad = ndt_marker_check_links(n_nodes, n_links, capacity);
    if (!bad && n_links > max_links) bad = "n_links: more links than the handle was created for";
    return bad;
}

#if defined(__HIPCC__)
// one selection of a handle: the tile words and the count words it leaves
struct NdtMarkerSel {
    uint32_t *tile;                               // [tiles]: segments | (lanes that raised a flag) << 16, then the segments before each tile
    uint32_t *count;                              // [4]: written, true total, overflow, flags
    unsigned long long capacity;
};
struct NdtMarkerCells {
    uint32_t first, count, tiles_per_map;
    const double *T16;                            // [count][16] or NULL
    double min_eval;
    double *points;                               // [capacity][6]
    uint32_t *src;                                // [capacity][2] or NULL
};
struct NdtMarkerLinks {
    const double *T16_nodes;                      // [n_nodes][16]
    const uint32_t *ref, *mov;                    // [n_links]
    const double *score;                          // [n_links] or NULL
    uint32_t n_nodes, n_links;
    int32_t skip_negative;
    double *points;                               // [capacity][6]
};
// host launchers: plain launches on `st`
hipError_t ndt_marker_cells_launch(const NdtSetView &set, const NdtMarkerCells &c, const NdtMarkerSel &sel, hipStream_t st);
hipError_t ndt_marker_links_launch(const NdtMarkerLinks &l, const NdtMarkerSel &sel, hipStream_t st);
hipError_t ndt_marker_particles_launch(const double *T12, size_t n, double length, double *points, hipStream_t st);
#endif
