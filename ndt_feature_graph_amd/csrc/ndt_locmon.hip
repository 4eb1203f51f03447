// ndt_locmon.hip -- the localisation monitor on CDNA4 (gfx950): the distance field of occupancy grids, the badness of (scan, pose)
// queries, the lattice search for the pose of least badness and the pick of the best-matching reference scan
// (include/ndtgpu.h "localisation monitor").
//
// Replaces (reference, flirtlib_ros): the ScanPoseEvaluator constructor, operator() and adjustPose (localization_monitor.cpp:41-120)
// and the reference-scan loop of updateUnlocalized (localization_monitor_node.cpp:348-372) with transformPose (common.cpp:56-66).
//
// Design.  Everything that decides a result is an integer; the order of the fp64 operations that lead to a pixel is
// in csrc/ndt_locmon.h.  Plain launches in stream order, no atomics, no workgroup waits on another:
//   field     ndt_locmon_row_kernel, (tiles of 256 pixels) x (grids), a lane per pixel: the nearest obstacle along the row within R,
//             one byte per pixel into the handle's scratch (255: none).  ndt_locmon_col_kernel, the same geometry: the smallest
//             dy^2 + g^2 over |dy| <= R, kept where <= R^2, as uint16 (0xFFFF: far).
//   badness   ndt_locmon_badness_kernel, ONE WORKGROUP of 256 lanes per query, lanes over beams: a lane computes the keys of its
//             beams into LDS (4 bytes a beam, sized by the call's n_beams); n_kept and n_offmap with ndt_block_count; the
//             (n_kept / 2)-th key by a most-significant-bit-first radix select, 17 rounds of one ndt_block_count each.
//   adjust    the same kernel with the query made from the lattice tables (a workgroup per candidate) writes the candidate's key to
//             the handle's scratch; ndt_locmon_finish_kernel, a lane per candidate: the volume and the tile's smallest
//             (key, index) word; ndt_locmon_winner_kernel, one workgroup over the tile words.  Badness and finish repeat per chunk.
//   pick      ndt_locmon_pick_kernel, one workgroup: the largest (n_inliers, -pair) word over the qualifying pairs, the composed
//             pose, the query and pick records.
// A query's result depends on its own scan, grid and pose alone: the same bits in any batch, at any position, on any run.
#include "ndt_locmon.h"
#include "ndt_block.h"

extern "C" __global__ __launch_bounds__(NDT_LOCMON_THREADS) void ndt_locmon_row_kernel(const int8_t *grids, uint8_t *rowdist, uint32_t width,
                                                                                      uint32_t height, int R, int occupied_min)
{
    const size_t wh = (size_t)width * height, idx = (size_t)blockIdx.x * NDT_LOCMON_TILE + threadIdx.x;
    if (idx >= wh) return;
    const uint32_t y = (uint32_t)(idx / width), x = (uint32_t)(idx - (size_t)y * width);
    const int8_t *row = grids + (size_t)blockIdx.y * wh + (size_t)y * width;
    rowdist[(size_t)blockIdx.y * wh + idx] = (uint8_t)ndt_locmon_row_dist(row, x, width, R, occupied_min);
}

extern "C" __global__ __launch_bounds__(NDT_LOCMON_THREADS) void ndt_locmon_col_kernel(const uint8_t *rowdist, uint16_t *field, uint32_t width,
                                                                                      uint32_t height, int R)
{
    const size_t wh = (size_t)width * height, idx = (size_t)blockIdx.x * NDT_LOCMON_TILE + threadIdx.x;
    if (idx >= wh) return;
    const uint32_t y = (uint32_t)(idx / width), x = (uint32_t)(idx - (size_t)y * width);
    field[(size_t)blockIdx.y * wh + idx] = (uint16_t)ndt_locmon_col_dist(rowdist + (size_t)blockIdx.y * wh, x, y, width, height, R);
}

// LATTICE: the query is candidate cand0 + blockIdx.x of the search; its key goes to s.cand_key[blockIdx.x].
// Otherwise the query is queries[blockIdx.x] and its record goes to results[blockIdx.x].
template <bool LATTICE>
__global__ __launch_bounds__(NDT_LOCMON_THREADS) void ndt_locmon_badness_kernel(NdtLocmonMap m, const double *ranges, uint32_t n_scans,
                                                                               const ndtgpu_locmon_query *queries, NdtLocmonSearch s,
                                                                               uint32_t cand0, double r_min, double r_max,
                                                                               ndtgpu_locmon_result *results)
{
    extern __shared__ uint32_t keys[];                                     // [n_beams]
    __shared__ NdtBlockCounts<NDT_LOCMON_WAVES> cnt;
    int par = 0;
    double x, y, c, sn;
    uint32_t scan, grid;
    if (LATTICE) {
        const uint32_t cand = cand0 + blockIdx.x;                          // (< n_candidates: the launch has one workgroup per candidate)
        const uint32_t iyaw = cand % s.nyaw, q = cand / s.nyaw, iy = q % s.ny, ix = q / s.ny;
        x = s.xs[ix];
        y = s.ys[iy];
        c = s.cs[iyaw];
        sn = s.sn[iyaw];
        scan = s.scan;
        grid = s.grid;
    } else {
        const ndtgpu_locmon_query &qr = queries[blockIdx.x];
        x = qr.x;
        y = qr.y;
        c = qr.c;
        sn = qr.s;
        scan = qr.scan;
        grid = qr.grid;
    }
    uint32_t flags = 0, key = NDT_LOCMON_KEY_OFFMAP, n_kept = 0, n_off = 0;
    if (scan == NDT_LOCMON_NO_SCAN) flags = NDTGPU_LOCMON_NO_QUERY;
    else if (scan >= n_scans || grid >= m.n_grids) flags = NDTGPU_LOCMON_BAD_INDEX;
    if (!flags) {                                                          // (the same in every thread: so are the barriers below)
        const double *rr = ranges + (size_t)scan * m.n_beams;
        const uint16_t *field = m.field + (size_t)grid * m.width * m.height;
        const double ox = m.origin[2 * grid], oy = m.origin[2 * grid + 1];
        uint32_t kept = 0, off = 0;
        for (uint32_t i = threadIdx.x; i < m.n_beams; i += NDT_LOCMON_THREADS) {
            const double r = rr[i];
            uint32_t k = 0xFFFFFFFFu;                                      // a dropped beam: matches no prefix of the select
            if (ndt_locmon_kept(r, r_min, r_max)) {
                uint32_t fi, fj;
                kept++;
                if (ndt_locmon_pixel(x, y, c, sn, m.beams[2 * i], m.beams[2 * i + 1], r, ox, oy, m.resolution, m.width, m.height, fi, fj)) {
                    k = ndt_locmon_key_of_field(field[(size_t)fj * m.width + fi]);
                } else {
                    k = NDT_LOCMON_KEY_OFFMAP;
                    off++;
                }
            }
            keys[i] = k;
        }
        n_kept = ndt_block_count(kept, cnt, par);                          // (its barrier also publishes keys[])
        n_off = ndt_block_count(off, cnt, par);
        if (n_kept == 0) {
            flags = NDTGPU_LOCMON_NO_BEAMS;
        } else {
            uint32_t want = n_kept / 2, prefix = 0;
            for (int b = NDT_LOCMON_KEY_BITS - 1; b >= 0; b--) {
                const uint32_t high = ~((2u << b) - 1u), bit = 1u << b;    // the bits above b are decided: they equal prefix
                uint32_t zeros = 0;
                for (uint32_t i = threadIdx.x; i < m.n_beams; i += NDT_LOCMON_THREADS) {
                    const uint32_t k = keys[i];
                    zeros += ((k & high) == prefix && !(k & bit)) ? 1u : 0u;
                }
                zeros = ndt_block_count(zeros, cnt, par);
                if (want >= zeros) { prefix |= bit; want -= zeros; }
            }
            key = prefix;
        }
    }
    if (threadIdx.x != 0) return;
    if (LATTICE) {
        s.cand_key[blockIdx.x] = key;
    } else {
        ndtgpu_locmon_result &out = results[blockIdx.x];
        out.badness = ndt_locmon_metres(key, m.resolution, m.max_dist);
        out.key = key;
        out.n_kept = n_kept;
        out.n_offmap = n_off;
        out.flags = flags;
    }
}

// the smallest word of the workgroup, in every thread: a shuffle tree per wave, then the waves.  ONE __syncthreads.
NDT_D unsigned long long ndt_locmon_block_min(unsigned long long w, unsigned long long (&lds)[NDT_LOCMON_WAVES])
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(w, o);
        w = v < w ? v : w;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = w;
    __syncthreads();
    w = lds[0];
    for (int k = 1; k < NDT_LOCMON_WAVES; k++) w = lds[k] < w ? lds[k] : w;
    return w;
}

// candidates [cand0, cand0 + n) of the lattice, their keys in s.cand_key[0 .. n); cand0 is a multiple of the tile
extern "C" __global__ __launch_bounds__(NDT_LOCMON_THREADS) void ndt_locmon_finish_kernel(NdtLocmonSearch s, uint32_t cand0, uint32_t n)
{
    __shared__ unsigned long long lds[NDT_LOCMON_WAVES];
    const uint32_t local = blockIdx.x * NDT_LOCMON_TILE + threadIdx.x;
    unsigned long long w = ~0ull;
    if (local < n) {
        const uint32_t key = s.cand_key[local];
        w = ndt_locmon_min_word(key, cand0 + local);
        if (s.volume) s.volume[cand0 + local] = key;
    }
    w = ndt_locmon_block_min(w, lds);
    if (threadIdx.x == 0) s.tile_word[cand0 / NDT_LOCMON_TILE + blockIdx.x] = w;
}

extern "C" __global__ __launch_bounds__(NDT_LOCMON_THREADS) void ndt_locmon_winner_kernel(NdtLocmonSearch s, uint32_t n_tiles, double resolution,
                                                                                         double max_dist)
{
    __shared__ unsigned long long lds[NDT_LOCMON_WAVES];
    unsigned long long w = ~0ull;
    for (uint32_t t = threadIdx.x; t < n_tiles; t += NDT_LOCMON_THREADS) w = s.tile_word[t] < w ? s.tile_word[t] : w;
    w = ndt_locmon_block_min(w, lds);
    if (threadIdx.x == 0) {
        const uint32_t key = (uint32_t)(w >> 32);
        const double badness = ndt_locmon_metres(key, resolution, max_dist);
        s.result->badness = badness;
        s.result->key = key;
        s.result->index = (uint32_t)w;
        s.result->flags = badness >= NDT_LOCMON_NO_RESULT_BADNESS ? NDTGPU_LOCMON_NO_RESULT : 0u;
        s.result->reserved = 0;
    }
}

extern "C" __global__ __launch_bounds__(NDT_LOCMON_THREADS) void ndt_locmon_pick_kernel(const ndtgpu_featmatch_result *matches, const double *ref_poses,
                                                                                       uint32_t n_pairs, uint32_t scan, uint32_t grid,
                                                                                       int32_t min_num_matches, double post_x, double post_y,
                                                                                       ndtgpu_locmon_query *query, ndtgpu_locmon_pick *pick)
{
    __shared__ unsigned long long lds[NDT_LOCMON_WAVES];
    unsigned long long w = 0ull;
    for (uint32_t p = threadIdx.x; p < n_pairs; p += NDT_LOCMON_THREADS) {
        const unsigned long long v = ndt_locmon_pick_word(matches[p].status, matches[p].n_inliers, min_num_matches, p);
        w = v > w ? v : w;
    }
    w = ~ndt_locmon_block_min(~w, lds);                                    // (the largest word)
    if (threadIdx.x != 0) return;
    if (w == 0ull) {
        query->x = 0.0;
        query->y = 0.0;
        query->c = 1.0;
        query->s = 0.0;
        query->scan = NDT_LOCMON_NO_SCAN;
        query->grid = grid;
        pick->pair = -1;
        pick->n_inliers = 0;
        pick->flags = NDTGPU_LOCMON_NO_PICK;
        pick->reserved = 0;
        return;
    }
    const uint32_t p = 0xFFFFFFFFu - (uint32_t)w;
    const double mp[4] = {matches[p].x, matches[p].y, matches[p].c, matches[p].s};
    double out[4];
    ndt_locmon_compose(ref_poses + 4 * (size_t)p, mp, post_x, post_y, out);
    query->x = out[0];
    query->y = out[1];
    query->c = out[2];
    query->s = out[3];
    query->scan = scan;
    query->grid = grid;
    pick->pair = (int32_t)p;
    pick->n_inliers = (int32_t)(w >> 32);
    pick->flags = 0;
    pick->reserved = 0;
}

hipError_t ndt_locmon_field_launch(const int8_t *grids, uint8_t *rowdist, uint16_t *field, uint32_t n_grids, uint32_t width, uint32_t height, int R,
                                   int occupied_min, hipStream_t st)
{
    const dim3 grid((unsigned)ndt_locmon_tiles((size_t)width * height), n_grids), threads(NDT_LOCMON_THREADS);
    hipLaunchKernelGGL(ndt_locmon_row_kernel, grid, threads, 0, st, grids, rowdist, width, height, R, occupied_min);
    hipLaunchKernelGGL(ndt_locmon_col_kernel, grid, threads, 0, st, (const uint8_t *)rowdist, field, width, height, R);
    return hipGetLastError();
}

hipError_t ndt_locmon_evaluate_launch(const NdtLocmonMap &m, const double *ranges, uint32_t n_scans, const ndtgpu_locmon_query *queries,
                                      uint32_t n_queries, double r_min, double r_max, ndtgpu_locmon_result *results, hipStream_t st)
{
    if (n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(ndt_locmon_badness_kernel<false>, dim3(n_queries), dim3(NDT_LOCMON_THREADS), m.n_beams * sizeof(uint32_t), st, m, ranges,
                       n_scans, queries, NdtLocmonSearch{}, 0u, r_min, r_max, results);
    return hipGetLastError();
}

hipError_t ndt_locmon_adjust_launch(const NdtLocmonMap &m, const double *ranges, uint32_t n_scans, const NdtLocmonSearch &s, uint32_t chunk,
                                    double r_min, double r_max, hipStream_t st)
{
    const dim3 threads(NDT_LOCMON_THREADS);
    for (size_t first = 0; first < s.n_candidates; first += chunk) {
        const uint32_t n = (uint32_t)(s.n_candidates - first < chunk ? s.n_candidates - first : chunk);
        hipLaunchKernelGGL(ndt_locmon_badness_kernel<true>, dim3(n), threads, m.n_beams * sizeof(uint32_t), st, m, ranges, n_scans,
                           (const ndtgpu_locmon_query *)nullptr, s, (uint32_t)first, r_min, r_max, (ndtgpu_locmon_result *)nullptr);
        hipLaunchKernelGGL(ndt_locmon_finish_kernel, dim3((unsigned)ndt_locmon_tiles(n)), threads, 0, st, s, (uint32_t)first, n);
    }
    hipLaunchKernelGGL(ndt_locmon_winner_kernel, dim3(1), threads, 0, st, s, (uint32_t)ndt_locmon_tiles(s.n_candidates), m.resolution, m.max_dist);
    return hipGetLastError();
}

hipError_t ndt_locmon_pick_launch(const ndtgpu_featmatch_result *matches, const double *ref_poses, uint32_t n_pairs, uint32_t scan, uint32_t grid,
                                  int32_t min_num_matches, double post_x, double post_y, ndtgpu_locmon_query *query, ndtgpu_locmon_pick *pick,
                                  hipStream_t st)
{
    hipLaunchKernelGGL(ndt_locmon_pick_kernel, dim3(1), dim3(NDT_LOCMON_THREADS), 0, st, matches, ref_poses, n_pairs, scan, grid, min_num_matches,
                       post_x, post_y, query, pick);
    return hipGetLastError();
}
