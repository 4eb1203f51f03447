// ndt_featextract.hip -- batched feature extraction from laser scans (include/ndtgpu.h, ndtgpu_featbank_extract*): a curvature
// detector on the chain of consecutive valid beams and the BetaGrid descriptor with the parameters the reference hands to flirtlib
// (flirtlib_utils.h:15-42), restated; steps 1-8 of the header.
//
// ndt_featextract_kernel: ONE workgroup of NDT_FEATEXTRACT_THREADS takes ONE scan from its ranges to a filled set of the feature
// bank; n_scans scans are n_scans workgroups that never look at each other.  Inside a workgroup only __syncthreads orders the
// phases: no grid barrier, no queue, no spin on memory.  The only atomics are integer adds on LDS counters (step 8), which are
// exact and free of order.
//   steps 1-2: the valid beams are compacted in beam order (ndt_block.h: a ballot prefix per wave, the waves' counts in order); a thread
//     then owns ceil(m / 256) consecutive points: it sums their chord lengths and counts their breaks, the threads' sums are
//     scanned over the wave (shuffle-up, a fixed tree) and the waves' totals added in order, and a second walk over the same
//     points writes the arc length g and the segment number of each.
//   steps 3-5: level by level, a lane per point.  The window is found by walking from k (g is monotone) while the segment
//     number stays the same, which also tells whether the segment's end was reached: eligibility needs no stored segment ends.
//     The window is then summed in ascending j.  R of the level goes to LDS for the neighbours' peak tests; a point keeps its
//     best level and response only -- the smoothed point of a found keypoint is computed again by the same code in step 7.
//   step 6: a lane per kept point walks both ways while the arc length stays below min_separation.
//   step 7: ordered compaction of the survivors, then a lane per stored point.
//   step 8: a wave per keypoint, four at a time, a lane per beam.  The bins that a beam's samples visit are a 64-bit mask in
//     registers, the hit bin is cleared from it, and the counts are added with integer LDS atomics; the divisions come last.
//     Only the samples within max_rho (+ 1e-6) of the keypoint are visited: the others have no bin.
// LDS: 48 B per beam + 2.5 KB, sized by the call's n_beams (dynamic): 19 KB at 360 beams, 36 KB at 720, 70 KB at 1440, 98.5 KB
// at 2048 -- above 64 KB the launcher raises the kernel's dynamic-LDS limit.
// Every sum's order depends on the scan's own valid points alone, so a scan's outputs are the same bits whichever batch it runs in.
// Contraction is off throughout: tests/flirt_model.py restates the arithmetic operation for operation, and the integer outputs
// rest on comparisons of such values.
#include "ndt_featextract.h"
#include "ndt_block.h"

#define FX_NO_LEVEL 0xFFu

struct FxFixed {
    unsigned hit[NDT_FEATEXTRACT_WAVES][NDT_FEATEXTRACT_MAX_BINS], miss[NDT_FEATEXTRACT_WAVES][NDT_FEATEXTRACT_MAX_BINS];
    double wsum[NDT_FEATEXTRACT_WAVES];
    NdtBlockCounts<NDT_FEATEXTRACT_WAVES> wint;
};
static_assert(sizeof(FxFixed) <= NDT_FEATEXTRACT_FIXED_BYTES && NDT_FEATEXTRACT_FIXED_BYTES % 16 == 0, "ndt_featextract_lds_bytes");

// the per-point arrays behind FxFixed, each of nb = n_beams rounded up to 8 entries
struct FxLayout {
    double2 *p;               // the valid points in beam order
    double *g;                // arc length
    double *R;                // the current level's response; from step 7 on: theta of stored point t
    double *best;             // the response at the kept level
    unsigned short *seg;      // segment number
    unsigned short *beam;     // beam of valid point k
    unsigned short *kp;       // the found points, ascending
    unsigned char *lvl;       // the kept level, FX_NO_LEVEL: no peak
    unsigned char *flag;      // steps 3-5: eligible at the current level; step 6: survives
};
static_assert(sizeof(double2) + 3 * sizeof(double) + 3 * sizeof(unsigned short) + 2 == NDT_FEATEXTRACT_POINT_BYTES, "FxLayout");

NDT_D FxLayout fx_layout(unsigned char *base, unsigned nb)
{
    FxLayout L;
    unsigned char *at = base + NDT_FEATEXTRACT_FIXED_BYTES;
    L.p = (double2 *)at;            at += (size_t)nb * sizeof(double2);
    L.g = (double *)at;             at += (size_t)nb * sizeof(double);
    L.R = (double *)at;             at += (size_t)nb * sizeof(double);
    L.best = (double *)at;          at += (size_t)nb * sizeof(double);
    L.seg = (unsigned short *)at;   at += (size_t)nb * sizeof(unsigned short);
    L.beam = (unsigned short *)at;  at += (size_t)nb * sizeof(unsigned short);
    L.kp = (unsigned short *)at;    at += (size_t)nb * sizeof(unsigned short);
    L.lvl = at;                     at += nb;
    L.flag = at;
    return L;
}

// step 3 for point k at the level of `sigma`: n = S - p_k, R = |n| / sigma, and whether k is eligible
NDT_D void fx_smooth(const FxLayout &L, unsigned m, unsigned k, double sigma, double &nx, double &ny, double &R, bool &eligible)
{
#pragma clang fp contract(off)
    const double h = 3.0 * sigma, two_s2 = (2.0 * sigma) * sigma;
    const double gk = L.g[k];
    const unsigned sk = L.seg[k];
    unsigned lo = k, hi = k;
    while (lo > 0 && L.seg[lo - 1] == sk && gk - L.g[lo - 1] <= h) lo--;
    while (hi + 1 < m && L.seg[hi + 1] == sk && L.g[hi + 1] - gk <= h) hi++;
    // a walk that stopped inside the segment stopped at a point more than 3 sigma away, and the segment's end is farther still
    const bool at_first = lo == 0 || L.seg[lo - 1] != sk, at_last = hi + 1 >= m || L.seg[hi + 1] != sk;
    eligible = (!at_first || gk - L.g[lo] >= h) && (!at_last || L.g[hi] - gk >= h);
    double sw = 0.0, sx = 0.0, sy = 0.0;
    for (unsigned j = lo; j <= hi; j++) {
        const double dg = L.g[j] - gk;
        const double w = exp(-(dg * dg) / two_s2);
        const double2 q = L.p[j];
        sw += w;
        sx += w * q.x;
        sy += w * q.y;
    }
    const double2 pk = L.p[k];
    nx = sx / sw - pk.x;
    ny = sy / sw - pk.y;
    R = __dsqrt_rn(nx * nx + ny * ny) / sigma;
}

struct FxGrid {
    double x, y, c, s;        // the keypoint and the cosine / sine of its theta
};

// step 8's bin of the location (qx, qy), -1: none
NDT_D int fx_bin(const FxGrid &G, const NdtFeatExtractParamsDev &prm, double qx, double qy)
{
#pragma clang fp contract(off)
    const double dx = qx - G.x, dy = qy - G.y;
    const double lx = G.c * dx + G.s * dy, ly = G.c * dy - G.s * dx;
    const double rho = __dsqrt_rn(lx * lx + ly * ly);
    if (!(rho >= prm.min_rho && rho < prm.max_rho)) return -1;
    const double phi = atan2(ly, lx);
    int a = (int)floor((rho - prm.min_rho) / prm.drho), c = (int)floor((phi + 3.14159265358979323846) / prm.dphi);
    a = max(0, min(a, prm.bin_rho - 1));
    c = max(0, min(c, prm.bin_phi - 1));
    return a * prm.bin_phi + c;                             // (< bin_rho * bin_phi <= 64)
}

// the bins that the samples of the beam of q visit.  Only the samples within max_rho + 1e-6 of the keypoint are looked at: the
// part of the beam inside that disc, with a sample to spare at either end; every other sample has no bin.
NDT_D unsigned long long fx_ray_mask(const FxGrid &G, const NdtFeatExtractParamsDev &prm, double qx, double qy)
{
#pragma clang fp contract(off)
    const double qn = __dsqrt_rn(qx * qx + qy * qy);
    if (!(qn > 0.0)) return 0ull;
    const double ux = qx / qn, uy = qy / qn;
    const double along = ux * G.x + uy * G.y;               // the keypoint's foot on the beam, from the sensor
    const double reach = prm.max_rho + 1e-6;
    const double disc = reach * reach - ((G.x * G.x + G.y * G.y) - along * along);
    if (!(disc >= 0.0)) return 0ull;
    const double half = __dsqrt_rn(disc);
    double u_lo = floor((qn - (along + half)) / prm.delta) - 1.0, u_hi = ceil((qn - (along - half)) / prm.delta) + 1.0;
    if (!(u_lo >= 1.0)) u_lo = 1.0;
    if (!(u_hi <= 16777216.0)) u_hi = 16777216.0;
    unsigned long long mask = 0ull;
    for (double u = u_lo; u <= u_hi; u += 1.0) {
        const double ud = u * prm.delta;
        if (!(ud < qn)) break;
        const double t = 1.0 - ud / qn;
        const int b = fx_bin(G, prm, qx * t, qy * t);
        if (b >= 0) mask |= 1ull << b;
    }
    return mask;
}

NDT_D void fx_write(ndtgpu_featextract_result *out, int status, unsigned n_valid, unsigned n_segments, unsigned n_peaks, unsigned n_found,
                    unsigned n_stored)
{
    out->n_valid = (int)n_valid;
    out->n_segments = (int)n_segments;
    out->n_peaks = (int)n_peaks;
    out->n_found = (int)n_found;
    out->n_stored = (int)n_stored;
    out->status = status;
}

__global__ __launch_bounds__(NDT_FEATEXTRACT_THREADS) void ndt_featextract_kernel(NdtFeatBankView v, uint32_t *count, double *pos,
                                                                                 double *desc, const uint32_t *set_idx,
                                                                                 const double *ranges, unsigned n_beams, double angle_min,
                                                                                 double angle_increment, NdtFeatExtractParamsDev prm,
                                                                                 ndtgpu_featextract_result *results, uint32_t *beam_out,
                                                                                 int32_t *level_out, double *response_out)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char fx_lds[];
    FxFixed &F = *(FxFixed *)fx_lds;
    const FxLayout L = fx_layout(fx_lds, (n_beams + 7u) & ~7u);
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t scan = blockIdx.x;
    ndtgpu_featextract_result *out = results + scan;

    // every exit below is taken by the whole workgroup: its condition is the same in every thread
    const uint32_t set = set_idx[scan];
    if (set >= v.n_sets) {
        if (tid == 0) fx_write(out, NDTGPU_FEATEXTRACT_BAD_INDEX, 0, 0, 0, 0, 0);
        return;
    }
    const unsigned MP = v.max_points, D = v.desc_len;

    // ---- step 1: the valid points in beam order ------------------------------------------------------------------------------
    const double *rr = ranges + scan * (size_t)n_beams;
    unsigned m = 0;
    int ipar = 0;
    for (unsigned base = 0; base < n_beams; base += NDT_FEATEXTRACT_THREADS) {
        const unsigned i = base + tid;
        const double r = i < n_beams ? rr[i] : 0.0;
        const bool ok = i < n_beams && r > prm.r_min && r < prm.r_max;          // (NaN and the infinities fail one of the two)
        unsigned kept;
        const unsigned at = m + ndt_block_rank(ok, F.wint, ipar, kept);
        if (ok) {
            const double phi = angle_min + (double)i * angle_increment;
            L.p[at] = make_double2(r * cos(phi), r * sin(phi));
            L.beam[at] = (unsigned short)i;
        }
        m += kept;
    }
    __syncthreads();
    if (m < 3) {
        if (tid == 0) {
            count[set] = 0;
            fx_write(out, NDTGPU_FEATEXTRACT_TOO_FEW_POINTS, m, 0, 0, 0, 0);
        }
        return;
    }

    // ---- step 2: arc length and segment numbers: a thread owns the points [k0, k1) ---------------------------------------------
    const unsigned per = (m + NDT_FEATEXTRACT_THREADS - 1) / NDT_FEATEXTRACT_THREADS;
    const unsigned k0 = min(tid * per, m), k1 = min(k0 + per, m);
    double own = 0.0;
    unsigned own_breaks = 0;
    for (unsigned k = max(k0, 1u); k < k1; k++) {
        const double2 a = L.p[k - 1], b = L.p[k];
        const double ex = b.x - a.x, ey = b.y - a.y;
        const double d = __dsqrt_rn(ex * ex + ey * ey);
        own += d;
        own_breaks += d > prm.dmst ? 1u : 0u;
    }
    double incl = own;
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(incl, o);
        if ((int)lane >= o) incl += t;
    }
    const double before_in_wave = __shfl_up(incl, 1);
    const unsigned incl_breaks = ndt_wave_incl_scan(own_breaks);
    if (lane == 63) {
        F.wsum[wave] = incl;
        F.wint.v[ipar][wave] = incl_breaks;               // (ndt_block.h's discipline: this half, one barrier, then the other)
    }
    __syncthreads();
    double run = 0.0;
    unsigned seg = 0, n_segments = 1;
    for (unsigned w = 0; w < NDT_FEATEXTRACT_WAVES; w++) {
        if (w < wave) {
            run += F.wsum[w];
            seg += F.wint.v[ipar][w];
        }
        n_segments += F.wint.v[ipar][w];
    }
    ipar ^= 1;
    if (lane > 0) run += before_in_wave;
    seg += incl_breaks - own_breaks;
    for (unsigned k = k0; k < k1; k++) {
        if (k > 0) {
            const double2 a = L.p[k - 1], b = L.p[k];
            const double ex = b.x - a.x, ey = b.y - a.y;
            const double d = __dsqrt_rn(ex * ex + ey * ey);
            run += d;
            seg += d > prm.dmst ? 1u : 0u;
        }
        L.g[k] = run;
        L.seg[k] = (unsigned short)seg;
    }
    for (unsigned k = tid; k < m; k += NDT_FEATEXTRACT_THREADS) {
        L.lvl[k] = FX_NO_LEVEL;
        L.best[k] = 0.0;
    }
    __syncthreads();

    // ---- steps 3-5: level by level, a lane per point ------------------------------------------------------------------------------
    unsigned my_peaks = 0;
    for (int s = 0; s < prm.scales; s++) {
        const double sigma = prm.sigma[s];
        for (unsigned k = tid; k < m; k += NDT_FEATEXTRACT_THREADS) {
            double nx, ny, R;
            bool eligible;
            fx_smooth(L, m, k, sigma, nx, ny, R, eligible);
            L.R[k] = R;
            L.flag[k] = eligible ? 1 : 0;
        }
        __syncthreads();
        for (unsigned k = tid; k < m; k += NDT_FEATEXTRACT_THREADS) {
            if (!L.flag[k] || k == 0 || k + 1 >= m) continue;   // (an eligible point has both neighbours in its segment)
            const double Rk = L.R[k];
            if (Rk > prm.min_value && Rk - L.R[k - 1] > prm.min_diff && Rk - L.R[k + 1] > prm.min_diff) {
                my_peaks++;
                if (L.lvl[k] == FX_NO_LEVEL || Rk > L.best[k]) {
                    L.best[k] = Rk;
                    L.lvl[k] = (unsigned char)s;
                }
            }
        }
        __syncthreads();
    }
    const unsigned n_peaks = ndt_block_count(my_peaks, F.wint, ipar);

    // ---- step 6: one pass over the step-5 set ---------------------------------------------------------------------------------------
    for (unsigned k = tid; k < m; k += NDT_FEATEXTRACT_THREADS) {
        bool keep = false;
        if (L.lvl[k] != FX_NO_LEVEL) {
            const double gk = L.g[k], Rk = L.best[k];
            const unsigned sk = L.seg[k];
            keep = true;
            for (unsigned j = k; j > 0;) {
                j--;
                if (L.seg[j] != sk || !(gk - L.g[j] < prm.min_separation)) break;
                if (L.lvl[j] != FX_NO_LEVEL && L.best[j] >= Rk) keep = false;     // (R' == R and k' < k)
            }
            for (unsigned j = k + 1; j < m; j++) {
                if (L.seg[j] != sk || !(L.g[j] - gk < prm.min_separation)) break;
                if (L.lvl[j] != FX_NO_LEVEL && L.best[j] > Rk) keep = false;
            }
        }
        L.flag[k] = keep ? 1 : 0;                                               // (nobody reads another point's flag in this step)
    }

    // ---- step 7: the survivors in beam order -------------------------------------------------------------------------------------------
    unsigned n_found = 0;
    for (unsigned base = 0; base < m; base += NDT_FEATEXTRACT_THREADS) {
        const unsigned k = base + tid;
        const bool keep = k < m && L.flag[k];
        unsigned kept;
        const unsigned at = n_found + ndt_block_rank(keep, F.wint, ipar, kept);
        if (keep) L.kp[at] = (unsigned short)k;
        n_found += kept;
    }
    __syncthreads();
    const unsigned n_stored = min(n_found, MP);
    for (unsigned t = tid; t < n_stored; t += NDT_FEATEXTRACT_THREADS) {
        const unsigned k = L.kp[t], s = L.lvl[k];
        double nx, ny, R;
        bool eligible;
        fx_smooth(L, m, k, prm.sigma[s], nx, ny, R, eligible);
        const double theta = atan2(ny, nx);
        const double2 pk = L.p[k];
        double *o = pos + ((size_t)set * MP + t) * 3;
        o[0] = pk.x;
        o[1] = pk.y;
        o[2] = theta;
        if (beam_out) beam_out[scan * MP + t] = L.beam[k];
        if (level_out) level_out[scan * MP + t] = (int32_t)s;
        if (response_out) response_out[scan * MP + t] = L.best[k];
        L.R[t] = theta;      // (the last level's R was read before that level's closing barrier; step 8's first barrier publishes this)
    }

    // ---- step 8: a wave per keypoint, four at a time, a lane per beam ------------------------------------------------------------
    double *dset = desc + (size_t)set * D * MP;
    for (unsigned t0 = 0; t0 < n_stored; t0 += NDT_FEATEXTRACT_WAVES) {
        const unsigned t = t0 + wave;
        const bool active = t < n_stored;
        F.hit[wave][lane] = 0;
        F.miss[wave][lane] = 0;
        __syncthreads();
        if (active) {
            const double2 c = L.p[L.kp[t]];
            const double theta = L.R[t];
            const FxGrid G = {c.x, c.y, cos(theta), sin(theta)};
            for (unsigned j = lane; j < m; j += 64) {
                const double2 q = L.p[j];
                const int hb = fx_bin(G, prm, q.x, q.y);
                unsigned long long mask = fx_ray_mask(G, prm, q.x, q.y);
                if (hb >= 0) {
                    atomicAdd(&F.hit[wave][hb], 1u);
                    mask &= ~(1ull << hb);                                      // the bin that q itself hits gets no miss from its beam
                }
                while (mask) {
                    atomicAdd(&F.miss[wave][__ffsll((long long)mask) - 1], 1u);
                    mask &= mask - 1ull;
                }
            }
        }
        __syncthreads();
        if (active && lane < D) {
            const unsigned h = F.hit[wave][lane], ms = F.miss[wave][lane];
            dset[(size_t)lane * MP + t] = ((double)h + 1.0) / ((double)(h + ms) + 2.0);
        }
        __syncthreads();                                                        // (the counts have been read before they are cleared)
    }
    if (tid == 0) {
        count[set] = n_stored;
        fx_write(out, n_found > n_stored ? NDTGPU_FEATEXTRACT_OVERFLOW : NDTGPU_FEATEXTRACT_OK, m, n_segments, n_peaks, n_found, n_stored);
    }
}

hipError_t ndt_featextract_launch(const NdtFeatBankView &v, uint32_t *count, double *pos, double *desc, const uint32_t *set_idx_dev,
                                  const double *ranges_dev, size_t n_scans, size_t n_beams, double angle_min, double angle_increment,
                                  const NdtFeatExtractParamsDev &prm, ndtgpu_featextract_result *results_dev, uint32_t *beam_dev,
                                  int32_t *level_dev, double *response_dev, hipStream_t st)
{
    if (!n_scans) return hipSuccess;
    const size_t lds = ndt_featextract_lds_bytes(n_beams);
    if (lds > 65536) {
        // above 64 KB a kernel has to ask for its dynamic LDS (per device, so on every such launch); one workgroup a CU then
        const hipError_t e = hipFuncSetAttribute((const void *)ndt_featextract_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ndt_featextract_kernel, dim3((unsigned)n_scans), dim3(NDT_FEATEXTRACT_THREADS), lds, st, v, count, pos, desc,
                       set_idx_dev, ranges_dev, (unsigned)n_beams, angle_min, angle_increment, prm, results_dev, beam_dev, level_dev,
                       response_dev);
    return hipGetLastError();
}
