// ndt_featmatch.hip -- batched feature-set RANSAC matching (include/ndtgpu.h, ndtgpu_featbank_*): flirtlib's
// RansacFeatureSetMatcher::matchSets as matchFeatureMap calls it (ndt_feature_map.h:104-122), restated; steps 1-8 of the header.
//
// ndt_featmatch_kernel: ONE workgroup of NDT_FEATMATCH_THREADS matches ONE (ref, mov) pair of sets from start to finish; n_pairs
// pairs are n_pairs workgroups that never look at each other.  Inside a workgroup only __syncthreads orders the phases: no grid
// barrier, no queue, no spin on memory, no atomics.
//   phase A (steps 1-2): a lane per mov point (256 at a time); the ref descriptors stream through an LDS tile of
//     NDT_FEATMATCH_TILE descriptors laid out [bin][ref], so a lane reads a bin of its own descriptor once per tile (coalesced:
//     the bank stores descriptors transposed) and the tile's 16 values of the bin from LDS, all lanes the same address.  Each
//     (mov, ref) distance is summed by ONE lane in ascending bin order.  The kept candidates are compacted in ascending i
//     (ndt_block.h: a ballot prefix per wave, the waves' counts in order).
//   phase B (steps 3-7): a wave per hypothesis, four at a time.  Lanes stride the mov points, two per lane per pass over the ref
//     positions in LDS (every lane reads the same address).  A lane's score terms are added in ascending i, then summed over the
//     wave in the order of ndt_block.h; a wave keeps the best of its hypotheses (ascending h, strict <), the four waves' bests
//     are reduced lexicographically on (score, h).
//   phase C (step 8): the whole workgroup sweeps with the best hypothesis's pose, refines it over the inliers, sweeps again and
//     compacts the inliers in ascending i.
// Every sum's order depends on n_ref and n_mov of the pair alone, so a pair's outputs are the same bits whichever batch it runs in.
// Contraction is off throughout: tests/featmatch_model.py restates the arithmetic operation for operation, and the integer
// outputs (candidates, best hypothesis, inliers) rest on comparisons of such values.
#include "ndt_featmatch.h"
#include "ndt_block.h"

struct FmPose {
    double c, s, tx, ty;
};

struct FmShared {
    double2 ref[NDT_FEATMATCH_MAX_POINTS], mov[NDT_FEATMATCH_MAX_POINTS];
    double tile[NDT_FEATMATCH_MAX_DESC * NDT_FEATMATCH_TILE];       // [bin][ref of the tile]
    unsigned short cand_i[NDT_FEATMATCH_MAX_POINTS], cand_j[NDT_FEATMATCH_MAX_POINTS];
    unsigned short nn[NDT_FEATMATCH_MAX_POINTS];                    // the last sweep's nearest ref point of each mov point
    unsigned char inl[NDT_FEATMATCH_MAX_POINTS];                    // ... and whether it is an inlier
    NdtBlockSums<NDT_FEATMATCH_WAVES, 4> red;
    NdtBlockCounts<NDT_FEATMATCH_WAVES> wcount;
    double wbest[NDT_FEATMATCH_WAVES];
    int wbest_h[NDT_FEATMATCH_WAVES], wtested[NDT_FEATMATCH_WAVES];
};

// step 5 over two correspondences (p: mov, q: ref), the sums in the order of the general form
NDT_D FmPose fm_pose2(double2 p1, double2 p2, double2 q1, double2 q2)
{
#pragma clang fp contract(off)
    const double mpx = (p1.x + p2.x) / 2.0, mpy = (p1.y + p2.y) / 2.0, mqx = (q1.x + q2.x) / 2.0, mqy = (q1.y + q2.y) / 2.0;
    const double ax = p1.x - mpx, ay = p1.y - mpy, bx = q1.x - mqx, by = q1.y - mqy;
    const double cx = p2.x - mpx, cy = p2.y - mpy, dx = q2.x - mqx, dy = q2.y - mqy;
    const double A = (ax * bx + ay * by) + (cx * dx + cy * dy);
    const double B = (ax * by - ay * bx) + (cx * dy - cy * dx);
    const double h = __dsqrt_rn(A * A + B * B);
    FmPose T;
    T.c = h == 0.0 ? 1.0 : A / h;
    T.s = h == 0.0 ? 0.0 : B / h;
    T.tx = mqx - (T.c * mpx - T.s * mpy);
    T.ty = mqy - (T.s * mpx + T.c * mpy);
    return T;
}

// hypothesis h of the pair (steps 3-5); false: skipped by the rigidity test
NDT_D bool fm_hypothesis(const FmShared &sh, const NdtFeatMatchParamsDev &prm, unsigned h, unsigned n_c, FmPose &T)
{
#pragma clang fp contract(off)
    unsigned a, b;
    ndt_featmatch_sample(prm.seed, h, n_c, a, b);
    a = min(a, n_c - 1);                                   // (never taken: the draws are < 1; an LDS index all the same)
    b = min(b, n_c - 1);
    const double2 p1 = sh.mov[sh.cand_i[a]], p2 = sh.mov[sh.cand_i[b]], q1 = sh.ref[sh.cand_j[a]], q2 = sh.ref[sh.cand_j[b]];
    const double fx = p1.x - p2.x, fy = p1.y - p2.y, gx = q1.x - q2.x, gy = q1.y - q2.y;
    const double f = fx * fx + fy * fy, g = gx * gx + gy * gy;
    if (f + g == 0.0) return false;
    const double d = f - g;
    if (d * d / (8.0 * (f + g)) > prm.rigidity_threshold) return false;
    T = fm_pose2(p1, p2, q1, q2);
    return true;
}

// Step 6 for the mov points first, first + stride, first + 2 stride, ...: this lane's part of the score, its terms added in
// ascending i.  Two points per pass over the ref positions.  RECORD: nn / inl of the points as well.
template <bool RECORD>
NDT_D double fm_sweep(FmShared &sh, unsigned n_ref, unsigned n_mov, const FmPose &T, double acceptance, unsigned first, unsigned stride)
{
#pragma clang fp contract(off)
    double score = 0.0;
    for (unsigned i0 = first; i0 < n_mov; i0 += 2 * stride) {
        const unsigned ia = i0, ib = i0 + stride;
        const bool has_b = ib < n_mov;
        const double2 pa = sh.mov[ia], pb = sh.mov[has_b ? ib : ia];
        const double ax = (T.c * pa.x - T.s * pa.y) + T.tx, ay = (T.s * pa.x + T.c * pa.y) + T.ty;
        const double bx = (T.c * pb.x - T.s * pb.y) + T.tx, by = (T.s * pb.x + T.c * pb.y) + T.ty;
        double best_a = INFINITY, best_b = INFINITY;
        unsigned ja = 0, jb = 0;
        for (unsigned j = 0; j < n_ref; j++) {
            const double2 q = sh.ref[j];
            const double dax = ax - q.x, day = ay - q.y, dbx = bx - q.x, dby = by - q.y;
            const double da = dax * dax + day * day, db = dbx * dbx + dby * dby;
            if (da < best_a) {
                best_a = da;
                if (RECORD) ja = j;
            }
            if (db < best_b) {
                best_b = db;
                if (RECORD) jb = j;
            }
        }
        const bool in_a = best_a < acceptance, in_b = best_b < acceptance;
        score += in_a ? best_a : acceptance;
        if (has_b) score += in_b ? best_b : acceptance;
        if (RECORD) {
            sh.nn[ia] = (unsigned short)ja;
            sh.inl[ia] = in_a ? 1 : 0;
            if (has_b) {
                sh.nn[ib] = (unsigned short)jb;
                sh.inl[ib] = in_b ? 1 : 0;
            }
        }
    }
    return score;
}

NDT_D void fm_write(ndtgpu_featmatch_result *out, double *T16, int status, double score, const FmPose &T, int n_c, int H, int n_tested,
                    int best_h, int n_inliers)
{
    out->score = score;
    out->x = T.tx;
    out->y = T.ty;
    out->theta = atan2(T.s, T.c);
    out->c = T.c;
    out->s = T.s;
    out->n_candidates = n_c;
    out->n_hypotheses = H;
    out->n_tested = n_tested;
    out->best_hypothesis = best_h;
    out->n_inliers = n_inliers;
    out->status = status;
    if (T16) {
        for (int k = 0; k < 16; k++) T16[k] = 0.0;
        T16[0] = T.c; T16[1] = T.s; T16[4] = -T.s; T16[5] = T.c; T16[10] = 1.0;
        T16[12] = T.tx; T16[13] = T.ty; T16[15] = 1.0;
    }
}

__global__ __launch_bounds__(NDT_FEATMATCH_THREADS) void ndt_featmatch_kernel(NdtFeatBankView v, const uint32_t *ref_idx,
                                                                               const uint32_t *mov_idx, NdtFeatMatchParamsDev prm,
                                                                               ndtgpu_featmatch_result *results, double *T16_all,
                                                                               uint32_t *corr_all)
{
#pragma clang fp contract(off)
    __shared__ FmShared sh;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pair = blockIdx.x;
    ndtgpu_featmatch_result *out = results + pair;
    double *T16 = T16_all ? T16_all + 16 * pair : nullptr;
    const FmPose identity = {1.0, 0.0, 0.0, 0.0};
    const int H = prm.n_hypotheses;

    // every exit below is taken by the whole workgroup: its condition is the same in every thread
    const uint32_t rs = ref_idx[pair], ms = mov_idx[pair];
    if (rs >= v.n_sets || ms >= v.n_sets) {
        if (tid == 0) fm_write(out, T16, NDTGPU_FEATMATCH_BAD_INDEX, NDT_FEATMATCH_FAIL_SCORE, identity, 0, H, 0, -1, 0);
        return;
    }
    const unsigned MP = v.max_points;
    const unsigned n_ref = min(v.count[rs], MP), n_mov = min(v.count[ms], MP);
    if (n_ref == 0 || n_mov == 0) {
        if (tid == 0) fm_write(out, T16, NDTGPU_FEATMATCH_TOO_FEW, NDT_FEATMATCH_FAIL_SCORE, identity, 0, H, 0, -1, 0);
        return;
    }
    const double *rpos = v.pos + (size_t)rs * MP * 3, *mpos = v.pos + (size_t)ms * MP * 3;
    for (unsigned i = tid; i < n_ref; i += NDT_FEATMATCH_THREADS) sh.ref[i] = make_double2(rpos[3 * i], rpos[3 * i + 1]);
    for (unsigned i = tid; i < n_mov; i += NDT_FEATMATCH_THREADS) sh.mov[i] = make_double2(mpos[3 * i], mpos[3 * i + 1]);

    // ---- phase A: the nearest ref descriptor of every mov point, the candidates in ascending i ------------------------------
    const double *rdesc = v.desc + (size_t)rs * v.desc_len * MP, *mdesc = v.desc + (size_t)ms * v.desc_len * MP;
    const unsigned D = v.desc_len;
    unsigned n_c = 0;
    int cpar = 0;
    for (unsigned base = 0; base < n_mov; base += NDT_FEATMATCH_THREADS) {
        const unsigned i = base + tid;
        const bool live = i < n_mov;
        double best = INFINITY;
        unsigned best_j = 0;
        for (unsigned j0 = 0; j0 < n_ref; j0 += NDT_FEATMATCH_TILE) {
            __syncthreads();                                      // (the previous tile has been read)
            for (unsigned e = tid; e < D * NDT_FEATMATCH_TILE; e += NDT_FEATMATCH_THREADS) {
                const unsigned k = e / NDT_FEATMATCH_TILE, j = j0 + e % NDT_FEATMATCH_TILE;
                sh.tile[e] = j < n_ref ? rdesc[(size_t)k * MP + j] : 0.0;
            }
            __syncthreads();
            double acc[NDT_FEATMATCH_TILE];
#pragma unroll
            for (int r = 0; r < NDT_FEATMATCH_TILE; r++) acc[r] = 0.0;
            for (unsigned k = 0; k < D; k++) {
                const double a = live ? mdesc[(size_t)k * MP + i] : 0.0;
                const double *t = &sh.tile[k * NDT_FEATMATCH_TILE];
#pragma unroll
                for (int r = 0; r < NDT_FEATMATCH_TILE; r++) {
                    const double b = t[r], sum = a + b, diff = a - b;
                    const double term = diff * diff / sum;
                    acc[r] = acc[r] + (sum > 0.0 ? term : 0.0);
                }
            }
#pragma unroll
            for (int r = 0; r < NDT_FEATMATCH_TILE; r++)
                if (j0 + r < n_ref && acc[r] < best) {
                    best = acc[r];
                    best_j = j0 + r;
                }
        }
        const bool keep = live && 0.5 * best < prm.distance_threshold;
        unsigned kept;
        const unsigned at = n_c + ndt_block_rank(keep, sh.wcount, cpar, kept);
        if (keep) {
            sh.cand_i[at] = (unsigned short)i;
            sh.cand_j[at] = (unsigned short)best_j;
        }
        n_c += kept;
    }
    __syncthreads();                                              // (positions and candidates are visible)
    if (n_c < 2 || (double)n_c * prm.inlier_probability < 2.0) {
        if (tid == 0) fm_write(out, T16, NDTGPU_FEATMATCH_TOO_FEW, NDT_FEATMATCH_FAIL_SCORE, identity, (int)n_c, H, 0, -1, 0);
        return;
    }

    // ---- phase B: a wave per hypothesis -----------------------------------------------------------------------------------------
    double wbest = INFINITY;
    int wbest_h = -1, tested = 0;
    for (int h = (int)wave; h < H; h += NDT_FEATMATCH_WAVES) {
        FmPose T;
        if (!fm_hypothesis(sh, prm, (unsigned)h, n_c, T)) continue;
        tested++;
        const double score = ndt_wave_sum(fm_sweep<false>(sh, n_ref, n_mov, T, prm.acceptance_threshold, lane, 64));
        if (wbest_h < 0 || score < wbest) {
            wbest = score;
            wbest_h = h;
        }
    }
    if (lane == 0) {
        sh.wbest[wave] = wbest;
        sh.wbest_h[wave] = wbest_h;
        sh.wtested[wave] = tested;
    }
    __syncthreads();
    double best_score = INFINITY;
    int best_h = -1, n_tested = 0;
    for (int w = 0; w < NDT_FEATMATCH_WAVES; w++) {
        const int hw = sh.wbest_h[w];
        n_tested += sh.wtested[w];
        if (hw < 0) continue;
        const double sw = sh.wbest[w];
        if (best_h < 0 || sw < best_score || (sw == best_score && hw < best_h)) {
            best_score = sw;
            best_h = hw;
        }
    }
    if (best_h < 0) {
        if (tid == 0) fm_write(out, T16, NDTGPU_FEATMATCH_NO_HYPOTHESIS, NDT_FEATMATCH_FAIL_SCORE, identity, (int)n_c, H, 0, -1, 0);
        return;
    }

    // ---- phase C: refine over the best hypothesis's inliers, the final sweep, the correspondences --------------------------------
    FmPose T;
    (void)fm_hypothesis(sh, prm, (unsigned)best_h, n_c, T);
    (void)fm_sweep<true>(sh, n_ref, n_mov, T, prm.acceptance_threshold, tid, NDT_FEATMATCH_THREADS);
    // (a thread reads back only the nn / inl entries it wrote itself: no barrier)
    int par = 0;
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned mine = 0;
    for (unsigned i = tid; i < n_mov; i += NDT_FEATMATCH_THREADS)
        if (sh.inl[i]) {
            const double2 p = sh.mov[i], q = sh.ref[sh.nn[i]];
            m[0] += p.x; m[1] += p.y; m[2] += q.x; m[3] += q.y;
            mine++;
        }
    ndt_block_sum(m, sh.red, par);
    const unsigned n_in = ndt_block_count(mine, sh.wcount, cpar);             // (the inlier count)
    if (n_in > 0) {
        const double mpx = m[0] / (double)n_in, mpy = m[1] / (double)n_in, mqx = m[2] / (double)n_in, mqy = m[3] / (double)n_in;
        double ab[2] = {0.0, 0.0};
        for (unsigned i = tid; i < n_mov; i += NDT_FEATMATCH_THREADS)
            if (sh.inl[i]) {
                const double2 p = sh.mov[i], q = sh.ref[sh.nn[i]];
                const double px = p.x - mpx, py = p.y - mpy, qx = q.x - mqx, qy = q.y - mqy;
                ab[0] += px * qx + py * qy;
                ab[1] += px * qy - py * qx;
            }
        ndt_block_sum(ab, sh.red, par);
        const double hh = __dsqrt_rn(ab[0] * ab[0] + ab[1] * ab[1]);
        T.c = hh == 0.0 ? 1.0 : ab[0] / hh;
        T.s = hh == 0.0 ? 0.0 : ab[1] / hh;
        T.tx = mqx - (T.c * mpx - T.s * mpy);
        T.ty = mqy - (T.s * mpx + T.c * mpy);
    }
    const double mine_fin = fm_sweep<true>(sh, n_ref, n_mov, T, prm.acceptance_threshold, tid, NDT_FEATMATCH_THREADS);
    const double fin = ndt_block_sum(mine_fin, sh.red, par);
    uint32_t *corr = corr_all ? corr_all + pair * (size_t)MP * 2 : nullptr;
    unsigned n_inliers = 0;
    for (unsigned base = 0; base < n_mov; base += NDT_FEATMATCH_THREADS) {
        const unsigned i = base + tid;
        const bool keep = i < n_mov && sh.inl[i];
        unsigned kept;
        const unsigned at = n_inliers + ndt_block_rank(keep, sh.wcount, cpar, kept);
        if (keep && corr) {
            corr[2 * (size_t)at] = i;
            corr[2 * (size_t)at + 1] = sh.nn[i];
        }
        n_inliers += kept;
    }
    if (tid == 0) fm_write(out, T16, NDTGPU_FEATMATCH_OK, fin, T, (int)n_c, H, n_tested, best_h, (int)n_inliers);
}

hipError_t ndt_featmatch_launch(const NdtFeatBankView &v, const uint32_t *ref_idx_dev, const uint32_t *mov_idx_dev, size_t n_pairs,
                                const NdtFeatMatchParamsDev &prm, ndtgpu_featmatch_result *results_dev, double *T16_dev,
                                uint32_t *corr_dev, hipStream_t st)
{
    if (!n_pairs) return hipSuccess;
    hipLaunchKernelGGL(ndt_featmatch_kernel, dim3((unsigned)n_pairs), dim3(NDT_FEATMATCH_THREADS), 0, st, v, ref_idx_dev, mov_idx_dev, prm,
                       results_dev, T16_dev, corr_dev);
    return hipGetLastError();
}
