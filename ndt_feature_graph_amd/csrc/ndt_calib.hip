// ndt_calib.hip -- laser-to-base extrinsic calibration on CDNA4 (gfx950): the brute-force search over sensor offsets
// (include/ndtgpu.h "extrinsic calibration").
//
// Replaces (reference): bruteForceOptimization (laser2d_extrinsic_calibration.cpp:176-204), errorFunction (:146-152) and
// ScanPair::scoreICP (:85-122) -- per candidate and pair two cloud transforms, a kd-tree build and a truncated 1-NN query per point.
//
// Design.  Distances do not change under a common rigid motion, and rotations of the plane commute: for the
// candidate Ts the pair's score is that of cloud1 AS IT IS against cloud2 rotated by the pair's own rotation -- once per pair -- and
// translated by t(Ts).  A candidate is a 2-D translation.  The order of every operation is in csrc/ndt_calib.h.
// Plain launches in stream order, no atomics, no workgroup waits on another:
//   1. ndt_calib_prepare_kernel, a workgroup per pair: the usable rows of cloud1 widened to double, those of cloud2 widened and
//      rotated, both compacted in row order (ndt_block_rank); the pair's motion; the counts.
//   2. ndt_calib_score_kernel, (candidate tiles) x (pairs) workgroups, a lane per candidate: the lane walks the rows of cloud2 in
//      order -- the order of the sum is the loop -- and for each the rows of cloud1.  The rows are the same for every lane of a
//      wave: their addresses are uniform and the loads scalar.  The lane's sum goes to partial[pair][candidate].
//   3. ndt_calib_finish_kernel, a lane per candidate: the pairs' sums added in pair order, the volume where it is asked for, and
//      the tile's ordered arg-min (smallest score, then lowest index) into the tile winners.
//   4. ndt_calib_winner_kernel, one workgroup: the same arg-min over the tile winners, the flags and the count of skipped rows.
// 2 and 3 repeat per chunk of candidates where pairs x candidates exceeds the scratch (ndt_calib_chunk).  A candidate's score
// depends on its pairs' clouds, poses and its own table entries alone: the same bits in any bank, chunk, tile and stream.
// The walk is not pruned: every row of cloud1 is visited for every row of cloud2.
#include "ndt_calib.h"
#include "ndt_block.h"

// the waves' winners of one arg-min
struct NdtCalibBest {
    double score[NDT_CALIB_WAVES];
    uint32_t index[NDT_CALIB_WAVES];
};

// the best (score, index) of the workgroup in the order of ndt_calib_better, in every thread: a shuffle tree per wave, then the
// waves in ascending order.  The order is total (no NaN among the scores), so the result does not depend on the tree's shape.
// ONE __syncthreads: a kernel calls it once per NdtCalibBest.
NDT_D void ndt_calib_block_argmin(double &score, uint32_t &index, NdtCalibBest &lds)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double s = __shfl_xor(score, o);
        const uint32_t i = (uint32_t)__shfl_xor((int)index, o);
        if (ndt_calib_better(s, i, score, index)) { score = s; index = i; }
    }
    if ((threadIdx.x & 63) == 0) { lds.score[threadIdx.x >> 6] = score; lds.index[threadIdx.x >> 6] = index; }
    __syncthreads();
    score = lds.score[0];
    index = lds.index[0];
    for (int w = 1; w < NDT_CALIB_WAVES; w++)
        if (ndt_calib_better(lds.score[w], lds.index[w], score, index)) { score = lds.score[w]; index = lds.index[w]; }
}

// the usable rows among the first `rows` of a scan, widened (ROTATE: and rotated by (cd, sd)), in row order -> their count
template <bool ROTATE>
NDT_D unsigned ndt_calib_compact(const uint32_t *scan, unsigned long long stride_words, uint32_t rows, double cd, double sd, double *out,
                                 NdtBlockCounts<NDT_CALIB_WAVES> &cnt, int &par)
{
    unsigned at = 0;
    for (uint32_t r0 = 0; r0 < rows; r0 += NDT_CALIB_THREADS) {       // (rows is the same for every thread: so are the barriers)
        const uint32_t r = r0 + threadIdx.x;
        float x = 0.f, y = 0.f, z = 0.f;
        bool keep = false;
        if (r < rows) {
            const uint32_t *w = scan + r * stride_words;
            x = __uint_as_float(w[0]);
            y = __uint_as_float(w[1]);
            z = __uint_as_float(w[2]);
            keep = ndt_calib_usable(x, y, z);
        }
        unsigned run;
        const unsigned row = at + ndt_block_rank(keep, cnt, par, run);
        at += run;
        if (!keep) continue;
        double px = (double)x, py = (double)y;
        if (ROTATE) ndt_calib_rotate(cd, sd, (double)x, (double)y, px, py);
        out[3 * (size_t)row] = px;                                      // row < rows <= n_points: inside the pair's block
        out[3 * (size_t)row + 1] = py;
        out[3 * (size_t)row + 2] = (double)z;
    }
    return at;
}

extern "C" __global__ __launch_bounds__(NDT_CALIB_THREADS) void ndt_calib_prepare_kernel(NdtCalibArgs a)
{
    __shared__ NdtBlockCounts<NDT_CALIB_WAVES> cnt;
    int par = 0;
    const uint32_t p = blockIdx.x;
    const uint32_t i1 = a.pairs[2 * p], i2 = a.pairs[2 * p + 1];
    const bool bad = i1 >= a.n_scans || i2 >= a.n_scans;
    double D[4] = {0.0, 0.0, 1.0, 0.0};
    uint32_t rows1 = 0, rows2 = 0;
    if (!bad) {
        ndt_calib_pair_motion(a.poses + 4 * (size_t)i1, a.poses + 4 * (size_t)i2, D);
        rows1 = a.n_kept[i1] < a.n_points ? a.n_kept[i1] : a.n_points;
        rows2 = a.n_kept[i2] < a.n_points ? a.n_kept[i2] : a.n_points;
    }
    const size_t block = (size_t)p * a.n_points * 3;
    const unsigned n1 = ndt_calib_compact<false>(a.xyz + (bad ? 0 : i1 * a.map_stride_words), a.stride_words, rows1, 1.0, 0.0, a.a3 + block, cnt, par);
    const unsigned n2 = ndt_calib_compact<true>(a.xyz + (bad ? 0 : i2 * a.map_stride_words), a.stride_words, rows2, D[2], D[3], a.b3 + block, cnt, par);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; k++) a.motion[4 * (size_t)p + k] = D[k];
        a.counts[4 * (size_t)p] = n1;
        a.counts[4 * (size_t)p + 1] = n2;
        a.counts[4 * (size_t)p + 2] = (rows1 - n1) + (rows2 - n2);
        a.counts[4 * (size_t)p + 3] = bad ? 1u : 0u;
    }
}

// candidates [cand0, cand0 + gridDim.x * TILE) of the lattice; partial: [n_pairs][stride]
extern "C" __global__ __launch_bounds__(NDT_CALIB_THREADS) void ndt_calib_score_kernel(NdtCalibArgs a, uint32_t cand0, uint32_t stride)
{
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.y;
    const uint32_t local = blockIdx.x * NDT_CALIB_TILE + threadIdx.x;
    const uint32_t cand = cand0 + local;
    const uint32_t cc = cand < a.n_candidates ? cand : a.n_candidates - 1;   // (a lane past the end computes the last candidate, and stores nothing)
    const uint32_t iyaw = cc % a.nyaw, q = cc / a.nyaw, iy = q % a.ny, ix = q / a.ny;
    const double *mo = a.motion + 4 * (size_t)p;
    const double D[4] = {mo[0], mo[1], mo[2], mo[3]};
    double tx, ty;
    ndt_calib_translation(D, a.xs[ix], a.ys[iy], a.cs[iyaw], a.sn[iyaw], tx, ty);
    const uint32_t n1 = a.counts[4 * (size_t)p], n2 = a.counts[4 * (size_t)p + 1];
    const double *__restrict__ pa = a.a3 + (size_t)p * a.n_points * 3;
    const double *__restrict__ pb = a.b3 + (size_t)p * a.n_points * 3;
    const double th2 = a.th2;
    double sum = 0.0;
    if (n1 > 0) {
        for (uint32_t j = 0; j < n2; j++) {
            const double bx = pb[3 * j] + tx, by = pb[3 * j + 1] + ty, bz = pb[3 * j + 2];
            double m = ndt_calib_d2(pa[0], pa[1], pa[2], bx, by, bz);
#pragma unroll 4
            for (uint32_t i = 1; i < n1; i++) {
                const double d = ndt_calib_d2(pa[3 * i], pa[3 * i + 1], pa[3 * i + 2], bx, by, bz);
                m = fmin(d, m);                                       // (no NaN among them: the rows are finite)
            }
            sum += ndt_calib_term(m, th2);
        }
    }
    if (cand < a.n_candidates) a.partial[(size_t)p * stride + local] = sum;
}

extern "C" __global__ __launch_bounds__(NDT_CALIB_THREADS) void ndt_calib_finish_kernel(NdtCalibArgs a, uint32_t cand0, uint32_t stride)
{
    __shared__ NdtCalibBest lds;
    const uint32_t local = blockIdx.x * NDT_CALIB_TILE + threadIdx.x;
    const uint32_t cand = cand0 + local;
    double score = __builtin_huge_val();
    uint32_t index = 0xFFFFFFFFu;
    if (cand < a.n_candidates) {
        score = 0.0;
        for (uint32_t p = 0; p < a.n_pairs; p++) score += a.partial[(size_t)p * stride + local];
        index = cand;
        if (a.volume) a.volume[cand] = score;
    }
    ndt_calib_block_argmin(score, index, lds);
    if (threadIdx.x == 0) {
        const uint32_t tile = cand0 / NDT_CALIB_TILE + blockIdx.x;       // (cand0 is a multiple of the tile)
        a.tile_score[tile] = score;
        a.tile_index[tile] = index;
    }
}

extern "C" __global__ __launch_bounds__(NDT_CALIB_THREADS) void ndt_calib_winner_kernel(NdtCalibArgs a, uint32_t n_tiles)
{
    __shared__ NdtCalibBest lds;
    __shared__ NdtBlockCounts<NDT_CALIB_WAVES> cnt;
    int par = 0;
    double score = __builtin_huge_val();
    uint32_t index = 0xFFFFFFFFu;
    for (uint32_t t = threadIdx.x; t < n_tiles; t += NDT_CALIB_THREADS)
        if (ndt_calib_better(a.tile_score[t], a.tile_index[t], score, index)) { score = a.tile_score[t]; index = a.tile_index[t]; }
    ndt_calib_block_argmin(score, index, lds);
    unsigned skipped = 0, bad = 0;
    for (uint32_t p = threadIdx.x; p < a.n_pairs; p += NDT_CALIB_THREADS) {
        skipped += a.counts[4 * (size_t)p + 2];
        bad += a.counts[4 * (size_t)p + 3];
    }
    skipped = ndt_block_count(skipped, cnt, par);
    bad = ndt_block_count(bad, cnt, par);
    if (threadIdx.x == 0) {
        a.result->score = score;
        a.result->index = index;
        a.result->flags = (score >= NDT_CALIB_CAP ? NDT_CALIB_FLAG_NO_RESULT : 0u) | (bad ? NDT_CALIB_FLAG_BAD_PAIR : 0u);
        a.result->n_skipped = skipped;
    }
}

hipError_t ndt_calib_launch(const NdtCalibArgs &a, hipStream_t st)
{
    const dim3 threads(NDT_CALIB_THREADS);
    hipLaunchKernelGGL(ndt_calib_prepare_kernel, dim3(a.n_pairs), threads, 0, st, a);
    const uint32_t stride = a.chunk;                                      // the handle's: n_pairs x chunk sums fit its scratch
    for (size_t first = 0; first < a.n_candidates; first += stride) {
        const size_t n = a.n_candidates - first < stride ? a.n_candidates - first : stride;
        const unsigned tiles = (unsigned)ndt_calib_tiles(n);
        hipLaunchKernelGGL(ndt_calib_score_kernel, dim3(tiles, a.n_pairs), threads, 0, st, a, (uint32_t)first, stride);
        hipLaunchKernelGGL(ndt_calib_finish_kernel, dim3(tiles), threads, 0, st, a, (uint32_t)first, stride);
    }
    hipLaunchKernelGGL(ndt_calib_winner_kernel, dim3(1), threads, 0, st, a, (uint32_t)ndt_calib_tiles(a.n_candidates));
    return hipGetLastError();
}
