// ndt_mcl.hip -- the device side of the NDT Monte Carlo localisation bank (csrc/ndtgpu_mcl.hip): NDTMCL3D::initializeFilter and
// updateAndPredictEff of perception_oru's ndt_mcl (call sites ndt_feature/src/ndt_feature_mcl_node.cpp:335, 361), restated in
// include/ndtgpu.h.  The scan's local map is built by the library's build kernels; what is here: draw the initial particles,
// predict, score every particle against the map, normalise / resample, and the weighted mean.
//
// Every sum is formed in an order fixed by the handle alone (particle count, chunk size): never by the launch shape, the CU
// count, the range of filters a call covers or how many filters the handle holds -- a particle's likelihood, weight and pose
// are the same bits whichever batch it runs in.  The sums over a workgroup are ndt_block.h's, in its order.
#include "ndt_mcl.h"
#include "ndt_block.h"

// LazyGrid::getIndexForPoint with the quotient as a product when the cell size is a power of two (the same bits: both are the
// correctly rounded value of one real number; csrc/ndt_match.hip lazygrid_index_p2)
NDT_D int mcl_grid_index(double p, double centre, double res, double inv_res, double half)
{
#pragma clang fp contract(off)
    const double q = inv_res != 0.0 ? (p - centre) * inv_res : (p - centre) / res;
    const double v = floor(q + 0.5) + half;
    if (!(v > -2.0e9 && v < 2.0e9)) return -1;
    return (int)v;
}

// initializeFilter: T = Translation(x + sx n0, ..) * AngleAxis(r + sr n3, X) * AngleAxis(p + sp n4, Y) * AngleAxis(t + st n5, Z),
// p = 1/N.  pose12: per filter {pose6, sigma6}
__global__ __launch_bounds__(NDT_MCL_THREADS) void ndt_mcl_init_kernel(unsigned first, unsigned n_particles, unsigned tiles,
                                                                       const double *__restrict__ pose12, unsigned long long seed,
                                                                       const NdtMclState *__restrict__ state, rigid *__restrict__ T,
                                                                       double *__restrict__ w)
{
#pragma clang fp contract(off)
    const unsigned fl = blockIdx.x / tiles, i = (blockIdx.x % tiles) * NDT_MCL_THREADS + threadIdx.x;
    if (i >= n_particles) return;
    const unsigned f = first + fl;
    const double *p = pose12 + (size_t)fl * 12;
    const unsigned long long c = state[f].draws;
    double v[6];
    for (int d = 0; d < 6; d++) v[d] = p[d] + p[6 + d] * ndt_hash_normal(seed, ndt_mcl_stream(f, c, NDT_MCL_DRAW_POSE + d), i);
    rigid R;
    ndt_mcl_xyz_rigid(v[0], v[1], v[2], v[3], v[4], v[5], R);
    const size_t k = (size_t)f * n_particles + i;
    T[k] = R;
    w[k] = 1.0 / (double)n_particles;
}

// one more draw counter value used up by every filter of the range (after an initialisation; an update's normalise kernel
// counts its own)
__global__ void ndt_mcl_bump_kernel(unsigned first, unsigned count, NdtMclState *__restrict__ state)
{
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) state[first + k].draws += 1ull;
}

// updateAndPredictEff step 4: T <- T * (Translation(tr + s0..2 n) * AngleAxis(rot0 + s3 n3, X) * AngleAxis(rot1 + s4 n4, Y) *
// AngleAxis(rot2 + s5 n5, Z)).  Also clears the filter's term counter for the likelihood kernel that follows.
__global__ __launch_bounds__(NDT_MCL_THREADS) void ndt_mcl_predict_kernel(unsigned first, unsigned n_particles, unsigned tiles,
                                                                          const NdtMclMotion *__restrict__ motion,
                                                                          unsigned long long seed, NdtMclState *__restrict__ state,
                                                                          rigid *__restrict__ T)
{
#pragma clang fp contract(off)
    const unsigned fl = blockIdx.x / tiles, i = (blockIdx.x % tiles) * NDT_MCL_THREADS + threadIdx.x;
    if (i >= n_particles) return;
    const unsigned f = first + fl;
    if (i == 0) state[f].terms = 0ull;
    const NdtMclMotion mo = motion[f];
    const unsigned long long c = state[f].draws;
    double v[6];
    for (int d = 0; d < 3; d++) v[d] = mo.tr[d] + mo.sigma[d] * ndt_hash_normal(seed, ndt_mcl_stream(f, c, NDT_MCL_DRAW_POSE + d), i);
    for (int d = 3; d < 6; d++)
        v[d] = mo.rot[d - 3] + mo.sigma[d] * ndt_hash_normal(seed, ndt_mcl_stream(f, c, NDT_MCL_DRAW_POSE + d), i);
    rigid inc;
    ndt_mcl_xyz_rigid(v[0], v[1], v[2], v[3], v[4], v[5], inc);
    const size_t k = (size_t)f * n_particles + i;
    rigid Tk = T[k];
    rigid_mul(Tk, inc, Tk);
    T[k] = Tk;
}

// updateAndPredictEff steps 5-6 for one (filter, tile of 256 particles, chunk of scan cells): each lane holds one particle's
// pose in registers; the chunk's scan cells pass through LDS in stages and are read by every lane (broadcast).  The lane's
// sum over the chunk, in cell order, goes to partial[(f * n_chunks + chunk) * N + particle]; the normalise kernel adds the
// chunks in order.  Cells the subsample drops are staged as NaN means: no term.
__global__ __launch_bounds__(NDT_MCL_THREADS) void ndt_mcl_likelihood_kernel(NdtSetView map, const uint32_t *__restrict__ map_idx,
                                                                             NdtSetView scan, unsigned first, unsigned n_particles,
                                                                             unsigned tiles, unsigned chunk, unsigned n_chunks,
                                                                             NdtMclParamsDev prm, NdtMclState *__restrict__ state,
                                                                             const rigid *__restrict__ T, double *__restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double s_cell[9][NDT_MCL_STAGE];
    __shared__ NdtBlockCounts<NDT_MCL_THREADS / 64> s_cnt;
    const unsigned per_filter = tiles * n_chunks;
    const unsigned fl = blockIdx.x / per_filter, r = blockIdx.x % per_filter;
    const unsigned tile = r / n_chunks, ck = r % n_chunks;
    const unsigned f = first + fl;
    unsigned n_cells = scan.counters[f].n_cells;
    if (n_cells > scan.grid.max_cells) n_cells = scan.grid.max_cells;
    const unsigned c0 = ck * chunk;
    if (c0 >= n_cells) return;                                        // (uniform over the workgroup)
    const unsigned c1 = min(c0 + chunk, n_cells);
    const unsigned tid = threadIdx.x, i = tile * NDT_MCL_THREADS + tid;
    const bool active = i < n_particles;
    rigid P;
    if (active) P = T[(size_t)f * n_particles + i];
    else P = rigid{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};

    const unsigned m = map_idx[f];
    const NdtGrid g = map.grid;
    const uint2 *rankmap = map.rankmap + (size_t)m * ndt_rm_stride(g);
    const NdtCell *mcells = ndt_cells_of(map, m, map.cell_sel ? map.cell_sel[m] : 0u);
    const double cx = map.centres[m * 3], cy = map.centres[m * 3 + 1], cz = map.centres[m * 3 + 2];
    int e2;
    const double inv_res = (g.res > 0.0 && frexp(g.res, &e2) == 0.5 && e2 > -1000 && e2 < 1000) ? 1.0 / g.res : 0.0;
    const NdtCell *scells = scan.cells + (size_t)f * scan.grid.max_cells;
    const bool subsample = prm.subsample_level < 1.0;
    const unsigned long long sub_stream = ndt_mcl_stream(f, state[f].draws, NDT_MCL_DRAW_SUBSAMPLE);

    double sum = 0.0;
    unsigned cnt = 0;
    for (unsigned s0 = c0; s0 < c1; s0 += NDT_MCL_STAGE) {
        const unsigned ns = min((unsigned)NDT_MCL_STAGE, c1 - s0);
        __syncthreads();
        for (unsigned j = tid; j < ns; j += NDT_MCL_THREADS) {
            const NdtCell &c = scells[s0 + j];
            const bool keep = !subsample || ndt_hash_uniform(prm.seed, sub_stream, s0 + j) < prm.subsample_level;
            s_cell[0][j] = keep ? c.mean[0] : __builtin_nan("");
            s_cell[1][j] = c.mean[1];
            s_cell[2][j] = c.mean[2];
            for (int q = 0; q < 6; q++) s_cell[3 + q][j] = c.cov[q];
        }
        __syncthreads();
        if (!active) continue;
        for (unsigned j = 0; j < ns; j++) {
            const d3 mu = apply(P, d3{s_cell[0][j], s_cell[1][j], s_cell[2][j]});
            if (mu.z < prm.zfilt_min) continue;
            // map.getCellAtPoint(pcl::PointXYZ(m)): float coordinates
            const int ix = mcl_grid_index((double)(float)mu.x, cx, g.res, inv_res, g.half[0]);
            const int iy = mcl_grid_index((double)(float)mu.y, cy, g.res, inv_res, g.half[1]);
            const int iz = mcl_grid_index((double)(float)mu.z, cz, g.res, inv_res, g.half[2]);
            if ((unsigned)ix >= (unsigned)g.size[0] || (unsigned)iy >= (unsigned)g.size[1] || (unsigned)iz >= (unsigned)g.size[2]) continue;
            const int rk = ndt_rank_of(rankmap, (unsigned)((ix * g.size[1] + iy) * g.size[2] + iz));
            if (rk < 0) continue;
            const NdtCell &mc = mcells[rk];
            const sym3 sc{s_cell[3][j], s_cell[4][j], s_cell[5][j], s_cell[6][j], s_cell[7][j], s_cell[8][j]};
            const sym3 S = sym3{mc.cov[0], mc.cov[1], mc.cov[2], mc.cov[3], mc.cov[4], mc.cov[5]} + rotate_cov(P.r, sc);
            sym3 Si;
            if (!inverse_check(S, Si)) continue;
            const d3 dm{mc.mean[0] - mu.x, mc.mean[1] - mu.y, mc.mean[2] - mu.z};
            const double l = dot(dm, mul(Si, dm));
            if (!(l * 0.0 == 0.0)) continue;
            sum += 0.1 + 0.9 * exp(-0.05 * l / 2.0);
            cnt++;
        }
    }
    if (active) partial[((size_t)f * n_chunks + ck) * n_particles + i] = sum;
    int par = 0;
    const unsigned long long t = ndt_block_count(cnt, s_cnt, par);    // terms scored
    if (tid == 0 && t) atomicAdd(&state[f].terms, t);
}

// updateAndPredictEff steps 6 (the chunks' sum) - 8, one workgroup per filter: lik, pf.normalize(), varP, the SIR decision and
// systematic resampling -- cumulative weights as exact 64-bit fixed-point sums, then one binary search per output particle.
__global__ __launch_bounds__(NDT_MCL_NORM_THREADS) void ndt_mcl_normalise_kernel(unsigned first, unsigned n_particles, unsigned chunk,
                                                                                 unsigned n_chunks, NdtMclParamsDev prm,
                                                                                 const NdtMapCounters *__restrict__ scan_ctr,
                                                                                 unsigned scan_cap, NdtMclState *__restrict__ state,
                                                                                 rigid *__restrict__ T, rigid *__restrict__ T_tmp,
                                                                                 double *__restrict__ w, double *__restrict__ lik,
                                                                                 const double *__restrict__ partial,
                                                                                 long long *__restrict__ cum)
{
#pragma clang fp contract(off)
    constexpr int NT = NDT_MCL_NORM_THREADS;
    __shared__ NdtBlockSums<NT / 64, 2> s_red;
    __shared__ long long s_scan[NT];
    __shared__ int s_sir;
    __shared__ double s_u0;
    const unsigned f = first + blockIdx.x, tid = threadIdx.x;
    const unsigned N = n_particles;
    const size_t base = (size_t)f * N;
    unsigned n_cells = scan_ctr[f].n_cells;
    if (n_cells > scan_cap) n_cells = scan_cap;
    const unsigned nch = (n_cells + chunk - 1) / chunk;
    const double invN = 1.0 / (double)N;

    int par = 0;
    double wl[2] = {0.0, 0.0};                                    // the sums of the weights and of the likelihoods
    for (unsigned i = tid; i < N; i += NT) {
        double li = 0.0;
        for (unsigned k = 0; k < nch; k++) li += partial[((size_t)f * n_chunks + k) * N + i];
        lik[base + i] = li;
        const double p = w[base + i] * li;
        w[base + i] = p;
        wl[0] += p;
        wl[1] += li;
    }
    ndt_block_sum(wl, s_red, par);
    const double S = wl[0], lik_sum = wl[1];
    double vs = 0.0;
    for (unsigned i = tid; i < N; i += NT) {
        const double p = S > 0.0 ? w[base + i] / S : invN;
        w[base + i] = p;
        const double d = p - invN;
        vs += d * d;
    }
    const double var_p = sqrt(ndt_block_sum(vs, s_red, par) / (double)N);
    if (tid == 0) {
        NdtMclState st = state[f];
        int sir = 0;
        if (prm.force_sir) {
            sir = 1;
        } else if (var_p > prm.sir_varp_threshold || st.since_sir > prm.sir_max_iters_wo_resampling) {
            sir = 1;
            st.since_sir = 0;
        } else {
            st.since_sir++;
        }
        s_sir = sir;
        s_u0 = ndt_hash_uniform(prm.seed, ndt_mcl_stream(f, st.draws, NDT_MCL_DRAW_SIR), 0);
        st.draws += 1ull;
        st.var_p = var_p;
        st.lik_sum = lik_sum;
        st.resampled = sir;
        st.n_scan_cells = (int)n_cells;
        st.overflow = scan_ctr[f].overflow ? 1 : 0;
        state[f] = st;              // (terms: written by the likelihood kernel, carried through unchanged)
    }
    __syncthreads();
    if (!s_sir) return;

    // SIRUpdate: thread t owns particles [t * seg, (t + 1) * seg)
    const unsigned seg = (N + NT - 1) / NT;
    const unsigned i0 = min(tid * seg, N), i1 = min(i0 + seg, N);
    long long run = 0;
    for (unsigned i = i0; i < i1; i++) {
        run += (long long)rint(ldexp(w[base + i], NDT_MCL_FX_SHIFT));
        cum[base + i] = run;
    }
    s_scan[tid] = run;
    __syncthreads();
    for (unsigned o = 1; o < (unsigned)NT; o <<= 1) {          // inclusive scan of the thread totals (exact integers)
        const long long v = tid >= o ? s_scan[tid - o] : 0ll;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const long long before = tid ? s_scan[tid - 1] : 0ll;
    for (unsigned i = i0; i < i1; i++) cum[base + i] += before;
    __syncthreads();
    const double u0 = s_u0;
    for (unsigned k = i0; k < i1; k++) {
        // the first particle whose cumulative weight exceeds (u0 + k) / N (none: the last one)
        const double thr = ldexp((u0 + (double)k) / (double)N, NDT_MCL_FX_SHIFT);
        unsigned lo = 0, hi = N - 1;
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if ((double)cum[base + mid] > thr) hi = mid;
            else lo = mid + 1;
        }
        T_tmp[base + k] = T[base + lo];
    }
    __syncthreads();
    for (unsigned k = i0; k < i1; k++) {
        T[base + k] = T_tmp[base + k];
        w[base + k] = invN;
    }
}

// pf.getMean(), one workgroup per filter: the weighted mean translation, and per Euler angle atan2(sum p sin, sum p cos) with
// each particle's eulerAngles(0, 1, 2)
__global__ __launch_bounds__(NDT_MCL_THREADS) void ndt_mcl_mean_kernel(unsigned first, unsigned n_particles,
                                                                            const rigid *__restrict__ T, const double *__restrict__ w,
                                                                            double *__restrict__ mean16)
{
#pragma clang fp contract(off)
    constexpr int NT = NDT_MCL_THREADS;
    __shared__ NdtBlockSums<NT / 64, 9> s_red;
    const unsigned fl = blockIdx.x, f = first + fl, tid = threadIdx.x;
    const size_t base = (size_t)f * n_particles;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned i = tid; i < n_particles; i += NT) {
        const rigid P = T[base + i];
        const double p = w[base + i];
        double P16[16], e[3];
        ndt_rigid_to16(P, P16);
        ndt_euler012(P16, e);
        for (int q = 0; q < 3; q++) {
            s[q] += p * P.t[q];
            s[3 + q] += p * cos(e[q]);
            s[6 + q] += p * sin(e[q]);
        }
    }
    int par = 0;
    ndt_block_sum(s, s_red, par);
    if (tid == 0) {
        rigid M;
        ndt_mcl_xyz_rigid(s[0], s[1], s[2], atan2(s[6], s[3]), atan2(s[7], s[4]), atan2(s[8], s[5]), M);
        ndt_rigid_to16(M, mean16 + (size_t)fl * 16);
    }
}

static unsigned mcl_tiles(unsigned n_particles) { return (n_particles + NDT_MCL_THREADS - 1) / NDT_MCL_THREADS; }

hipError_t ndt_mcl_launch_init(size_t first, size_t count, unsigned n_particles, const double *pose12_dev, unsigned long long seed,
                               NdtMclState *state, rigid *T, double *w, hipStream_t st)
{
    if (!count) return hipSuccess;
    const unsigned tiles = mcl_tiles(n_particles);
    hipLaunchKernelGGL(ndt_mcl_init_kernel, dim3((unsigned)(count * tiles)), dim3(NDT_MCL_THREADS), 0, st, (unsigned)first, n_particles,
                       tiles, pose12_dev, seed, state, T, w);
    hipLaunchKernelGGL(ndt_mcl_bump_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (unsigned)first, (unsigned)count,
                       state);
    return hipGetLastError();
}

hipError_t ndt_mcl_launch_predict(size_t first, size_t count, unsigned n_particles, const NdtMclMotion *motion_dev,
                                  unsigned long long seed, NdtMclState *state, rigid *T, hipStream_t st)
{
    if (!count) return hipSuccess;
    const unsigned tiles = mcl_tiles(n_particles);
    hipLaunchKernelGGL(ndt_mcl_predict_kernel, dim3((unsigned)(count * tiles)), dim3(NDT_MCL_THREADS), 0, st, (unsigned)first,
                       n_particles, tiles, motion_dev, seed, state, T);
    return hipGetLastError();
}

hipError_t ndt_mcl_launch_likelihood(const NdtSetView &map, const uint32_t *map_idx_dev, const NdtSetView &scan, size_t first,
                                     size_t count, unsigned n_particles, unsigned chunk, unsigned n_chunks, const NdtMclParamsDev &prm,
                                     NdtMclState *state, const rigid *T, double *partial, hipStream_t st)
{
    if (!count) return hipSuccess;
    const unsigned tiles = mcl_tiles(n_particles);
    hipLaunchKernelGGL(ndt_mcl_likelihood_kernel, dim3((unsigned)(count * tiles * n_chunks)), dim3(NDT_MCL_THREADS), 0, st, map,
                       map_idx_dev, scan, (unsigned)first, n_particles, tiles, chunk, n_chunks, prm, state, T, partial);
    return hipGetLastError();
}

hipError_t ndt_mcl_launch_normalise(size_t first, size_t count, unsigned n_particles, unsigned chunk, unsigned n_chunks,
                                    const NdtMclParamsDev &prm, const NdtSetView &scan, NdtMclState *state, rigid *T, rigid *T_tmp,
                                    double *w, double *lik, const double *partial, long long *cum, hipStream_t st)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(ndt_mcl_normalise_kernel, dim3((unsigned)count), dim3(NDT_MCL_NORM_THREADS), 0, st, (unsigned)first, n_particles,
                       chunk, n_chunks, prm, (const NdtMapCounters *)scan.counters, scan.grid.max_cells, state, T, T_tmp, w, lik,
                       partial, cum);
    return hipGetLastError();
}

hipError_t ndt_mcl_launch_mean(size_t first, size_t count, unsigned n_particles, const rigid *T, const double *w, double *mean16_dev,
                               hipStream_t st)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(ndt_mcl_mean_kernel, dim3((unsigned)count), dim3(NDT_MCL_THREADS), 0, st, (unsigned)first, n_particles, T, w,
                       mean16_dev);
    return hipGetLastError();
}
