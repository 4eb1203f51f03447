// ndt_pgo_robust.hip -- robust loop-closure weighting of the SE(2) and SE(3) pose-graph banks (include/ndtgpu.h, ndtgpu_pgo_optimize_robust
// and ndtgpu_pgo3_optimize_robust): one round of iteratively re-weighted least squares is these two launches and then the
// optimiser as it is.
//
// ndt_pgo_robust_weigh_kernel / ndt_pgo3_robust_weigh_kernel: grid (tiles of 256 links) x (graphs of the call), a lane per link.
// The lane evaluates its link at the poses the graph holds with the optimiser's own per-link body (pgo_linearise_link,
// pgo3_linearise_link: the inlines of csrc/ndt_pgo.h / ndt_pgo3.h) through a graph view whose information is the copy made when the
// graph was set, so chi2 = e^T W0 e whatever weights the bank holds; it writes chi2, the weight, the inlier flag and, where the
// launch applies, weight * W0 into the bank's information.  The per-link body also stores the link's linearisation into the
// bank's SCRATCH, as it does for the optimiser: jac, and te = W0 e (with W0, not the weighted information) -- an evaluation-only
// call included.  Nothing may rely on jac / te across calls: every optimiser entry linearises again before it reads them, and the
// marginals linearise into their own area.  A tile's sums -- robust cost, chi2, the counts of links flagged out,
// of chi2 that are not finite and of half turns -- are taken in the order of ndt_block.h and stored per tile.
// ndt_pgo_robust_finish_kernel / ndt_pgo3_robust_finish_kernel: one workgroup per graph adds the per-tile sums in the order of
// ndt_pgo_wide_core.h's combiner (thread t takes t, t + 256, ...; then the workgroup sum) and writes the graph's record.  A graph
// with a chi2 that is not finite gets W0 back: this round's weights are not applied to it.
// Plain launches, the boundary between them the only synchronisation: no atomics, no grid barrier, no workgroup that waits for
// another, no spin.  The tiling follows a graph's n_edges alone, so its numbers are the same bits in any batch.
#include "ndt_pgo_robust.h"
#include "ndt_pgo_wide_core.h"

#include <algorithm>

static_assert(NDT_PGO_ROBUST_TILE == NDT_PGO_WIDE_TILE, "the finish kernels add the per-tile sums with the wide form's combiner");
typedef NdtBlockCounts<NDT_PGO_WIDE_WAVES> RobustCnt;

// the link's term of the robust cost
__device__ double robust_cost_term(int kind, double scale, double chi2)
{
    if (kind == NDTGPU_PGO_ROBUST_HUBER) {
        const double r = ndt_pgo_sqrt(chi2);
        return r <= scale ? chi2 : 2.0 * scale * r - scale * scale;
    }
    if (kind == NDTGPU_PGO_ROBUST_CAUCHY) {
        const double c2 = scale * scale;
        return c2 * log(1.0 + chi2 / c2);
    }
    const double s = ndt_pgo_robust_dcs_s(scale, chi2);
    return s * s * chi2 + scale * (1.0 - s) * (1.0 - s);
}

// What a lane does with its link's chi2, and the tile's sums; every thread of the workgroup calls it (live: the lane has a link).
// K: the doubles of a link's information in the bank's layout.
template <int K>
__device__ void robust_weigh_tile(bool live, double chi2, bool half, size_t g, unsigned e, unsigned tiles, size_t max_edges,
                                  const int32_t *ref, const int32_t *mov, double *info, const NdtPgoRobustView &r,
                                  const NdtPgoRobustParamsDev &prm, int apply, WideRed &red, RobustCnt &cnt)
{
    double sums[2] = {0.0, 0.0};
    unsigned out = 0, bad = 0;
    if (live) {
        const bool prot = ndt_pgo_robust_protected(ref[e], mov[e], prm.min_index_gap);
        const double w = prot ? 1.0 : ndt_pgo_robust_weight(prm.kind, prm.scale, chi2);
        const int in = w >= prm.inlier_weight ? 1 : 0;
        const size_t le = g * max_edges + e;
        r.chi2[le] = chi2;
        r.weight[le] = w;
        r.inlier[le] = in;
        if (apply) {
            const double *W0 = r.w0 + K * le;
            double *W = info + K * (size_t)e;
            if (prot) {
                for (int k = 0; k < K; k++) W[k] = W0[k];
            } else {
                for (int k = 0; k < K; k++) W[k] = w * W0[k];
            }
        }
        sums[0] = prot ? chi2 : robust_cost_term(prm.kind, prm.scale, chi2);
        sums[1] = chi2;
        out = in ? 0u : 1u;
        bad = (chi2 - chi2 == 0.0 && w - w == 0.0) ? 0u : 1u;
    }
    int par = 0, parc = 0;
    ndt_block_sum(sums, red, par);
    const unsigned n_out = ndt_block_count(out, cnt, parc);
    const unsigned n_bad = ndt_block_count(bad, cnt, parc);
    const unsigned n_half = ndt_block_count((live && half) ? 1u : 0u, cnt, parc);
    if (threadIdx.x == 0) {
        double *pd = r.part + g * 2 * r.tiles;
        uint32_t *pn = r.part_n + g * 3 * r.tiles;
        pd[blockIdx.x] = sums[0];
        pd[tiles + blockIdx.x] = sums[1];
        pn[blockIdx.x] = n_out;
        pn[tiles + blockIdx.x] = n_bad;
        pn[2 * tiles + blockIdx.x] = n_half;
    }
}

__global__ __launch_bounds__(NDT_PGO_ROBUST_TILE) void ndt_pgo_robust_weigh_kernel(NdtPgoView v, NdtPgoRobustView r, size_t first,
                                                                                    NdtPgoRobustParamsDev prm, int apply)
{
    __shared__ WideRed red;
    __shared__ RobustCnt cnt;
    const size_t g = first + blockIdx.y;
    const ndtgpu_pgo_result *st = v.state + g;
    const unsigned E = (unsigned)st->n_edges, tiles = (E + NDT_PGO_ROBUST_TILE - 1) / NDT_PGO_ROBUST_TILE;
    if (blockIdx.x >= tiles) return;                     // (the whole workgroup: the grid is as wide as the call's largest graph)
    PgoGraph G = ndt_pgo_graph(v, g, (unsigned)st->n_nodes, E);
    double *info = v.info + g * 6 * v.max_edges;
    G.info = r.w0 + g * 6 * v.max_edges;                 // the information as set
    const unsigned e = blockIdx.x * NDT_PGO_ROBUST_TILE + threadIdx.x;
    const bool live = e < E;
    const double chi2 = live ? pgo_linearise_link(G, e) : 0.0;
    robust_weigh_tile<6>(live, chi2, false, g, e, tiles, v.max_edges, G.ref, G.mov, info, r, prm, apply, red, cnt);
}

__global__ __launch_bounds__(NDT_PGO_ROBUST_TILE) void ndt_pgo3_robust_weigh_kernel(NdtPgo3View v, NdtPgoRobustView r, size_t first,
                                                                                     NdtPgoRobustParamsDev prm, int apply)
{
    __shared__ WideRed red;
    __shared__ RobustCnt cnt;
    const size_t g = first + blockIdx.y;
    const ndtgpu_pgo_result *st = v.state + g;
    const unsigned E = (unsigned)st->n_edges, tiles = (E + NDT_PGO_ROBUST_TILE - 1) / NDT_PGO_ROBUST_TILE;
    if (blockIdx.x >= tiles) return;
    Pgo3Graph G = ndt_pgo3_graph(v, g, (unsigned)st->n_nodes, E);
    double *info = v.info + g * 21 * v.max_edges;
    G.info = r.w0 + g * 21 * v.max_edges;
    const unsigned e = blockIdx.x * NDT_PGO_ROBUST_TILE + threadIdx.x;
    const bool live = e < E;
    const NdtPgo3ParamsDev none{};                       // (the prior's information: read for link n_edges only, which no lane has)
    bool half = false;
    const double chi2 = live ? pgo3_linearise_link(G, none, e, half) : 0.0;
    robust_weigh_tile<21>(live, chi2, half, g, e, tiles, v.max_edges, G.ref, G.mov, info, r, prm, apply, red, cnt);
}

// one workgroup per graph: the sums of its tiles, its verdict, and W0 back into the bank where the verdict is bad
template <int K>
__device__ void robust_finish(size_t g, unsigned E, size_t max_edges, double *info, const NdtPgoRobustView &r, int apply)
{
    __shared__ WideRed red;
    __shared__ RobustCnt cnt;
    int par = 0, parc = 0;
    const unsigned tiles = (E + NDT_PGO_ROBUST_TILE - 1) / NDT_PGO_ROBUST_TILE;
    double s[2];
    wide_combine(r.part + g * 2 * r.tiles, tiles, s, red, par);
    const uint32_t *pn = r.part_n + g * 3 * r.tiles;
    unsigned c[3] = {0, 0, 0};
    for (unsigned t = threadIdx.x; t < tiles; t += NDT_PGO_ROBUST_TILE)
        for (int k = 0; k < 3; k++) c[k] += pn[(size_t)k * tiles + t];
    for (int k = 0; k < 3; k++) c[k] = ndt_block_count(c[k], cnt, parc);
    const int status = c[2] ? NDTGPU_PGO3_HALF_TURN : (c[1] ? NDTGPU_PGO_NOT_FINITE : NDTGPU_PGO_CONVERGED);
    if (apply && status != NDTGPU_PGO_CONVERGED) {
        const double *W0 = r.w0 + g * K * max_edges;
        for (size_t i = threadIdx.x; i < (size_t)K * E; i += NDT_PGO_ROBUST_TILE) info[i] = W0[i];
    }
    if (threadIdx.x == 0) {
        NdtPgoRobustSum *o = r.sum + g;
        o->cost = s[0];
        o->chi2 = s[1];
        o->flagged = (int32_t)c[0];
        o->status = status;
    }
}

__global__ __launch_bounds__(NDT_PGO_ROBUST_TILE) void ndt_pgo_robust_finish_kernel(NdtPgoView v, NdtPgoRobustView r, size_t first, int apply)
{
    const size_t g = first + blockIdx.x;
    robust_finish<6>(g, (unsigned)v.state[g].n_edges, v.max_edges, v.info + g * 6 * v.max_edges, r, apply);
}

__global__ __launch_bounds__(NDT_PGO_ROBUST_TILE) void ndt_pgo3_robust_finish_kernel(NdtPgo3View v, NdtPgoRobustView r, size_t first, int apply)
{
    const size_t g = first + blockIdx.x;
    robust_finish<21>(g, (unsigned)v.state[g].n_edges, v.max_edges, v.info + g * 21 * v.max_edges, r, apply);
}

// the second grid dimension holds 65535 workgroups: a longer run of graphs takes several launches
template <class View, class Weigh, class Finish>
static hipError_t robust_launch(Weigh weigh, Finish finish, const View &v, const NdtPgoRobustView &r, size_t first, size_t count,
                                size_t max_links, const NdtPgoRobustParamsDev &prm, bool apply, hipStream_t st)
{
    const unsigned tiles = (unsigned)std::max<size_t>((max_links + NDT_PGO_ROBUST_TILE - 1) / NDT_PGO_ROBUST_TILE, 1);
    for (size_t at = 0; at < count; at += 65535) {
        const unsigned n = (unsigned)std::min<size_t>(count - at, 65535);
        hipLaunchKernelGGL(weigh, dim3(tiles, n), dim3(NDT_PGO_ROBUST_TILE), 0, st, v, r, first + at, prm, apply ? 1 : 0);
        hipLaunchKernelGGL(finish, dim3(n), dim3(NDT_PGO_ROBUST_TILE), 0, st, v, r, first + at, apply ? 1 : 0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t ndt_pgo_robust_launch(const NdtPgoView &v, const NdtPgoRobustView &r, size_t first, size_t count, size_t max_links,
                                 const NdtPgoRobustParamsDev &prm, bool apply, hipStream_t st)
{
    return robust_launch(ndt_pgo_robust_weigh_kernel, ndt_pgo_robust_finish_kernel, v, r, first, count, max_links, prm, apply, st);
}

hipError_t ndt_pgo3_robust_launch(const NdtPgo3View &v, const NdtPgoRobustView &r, size_t first, size_t count, size_t max_links,
                                  const NdtPgoRobustParamsDev &prm, bool apply, hipStream_t st)
{
    return robust_launch(ndt_pgo3_robust_weigh_kernel, ndt_pgo3_robust_finish_kernel, v, r, first, count, max_links, prm, apply, st);
}
