// ndt_fuserfeat.hip -- the device side of the fuser bank's feature path (include/ndtgpu.h "the fuser bank's feature path"): what
// sits between ndt_featmatch_kernel (the RANSAC of ndt_feature_fuser_hmt.cpp:251) and ndt_match_kernel (matchFusion, :353-357), and
// behind ndt_fuser_post_kernel (the pose update), when NDTFeatureFuserHMT::update runs with useFeat for a batch of fusers.
//
// Replaces, per fuser slot (ndt_feature/src/ndt_feature_src/ndt_feature_fuser_hmt.cpp):
//   :252-289   Tfeat and the consistency gate                                              -> ndt_fuserfeat_cells_kernel
//   :294-334   convertCorrespondencesToCellvectorsFixedCovWithCorr, pseudoTransformNDTMap (sensor_pose, then Tnow / Tinit),
//              the 40 odometry cells behind them                                           -> ndt_fuserfeat_cells_kernel
//   :497-502   ptsPrev = pts, moveInterestPointVec, featuremap.update                      -> ndt_fuserfeat_commit_kernel
//
// The matcher reads the cells of registration k at feat_off[k] .. feat_off[k + 1], so a call's records are contiguous: one
// workgroup scans the slots' counts in slot order first (ndt_fuserfeat_offsets_kernel; integer sums, the same on every run).  No
// workgroup waits for another, no atomics, fp64 with contraction off (ndt_fuserfeat.h): a slot's outputs depend on its own
// inputs only.  All three are latency-sized: a few hundred bytes per slot, except the commit's descriptor copy (desc_len x n
// doubles per slot, read and written coalesced along the points).
#include "ndt_fuserfeat.h"
#include "ndt_block.h"

namespace {

// the gate of slot k (uniform over the lanes that call it)
NDT_D void ff_gate(const NdtFuserFeatArgs &a, unsigned k, ndtgpu_fuser_feat_result &rec)
{
    ndt_fuserfeat_gate(a.pol, a.ransac ? a.ransac + k : nullptr, a.T16 + 16 * (size_t)k, a.sensor_pose16, a.state[k].Tnow,
                       a.Tmotion16 + 16 * (size_t)k, rec);
}

}  // namespace

// foff[k] = the number of cells of the slots below k, foff[count] = all of them: ONE workgroup, 256 slots per pass
__global__ __launch_bounds__(256) void ndt_fuserfeat_offsets_kernel(NdtFuserFeatArgs a)
{
    __shared__ NdtBlockCounts<4> cnt;
    int par = 0;
    unsigned running = 0;
    for (unsigned base = 0; base < a.count; base += 256) {
        const unsigned k = base + threadIdx.x;
        unsigned c = 0;
        if (k < a.count) {
            ndtgpu_fuser_feat_result rec;
            ff_gate(a, k, rec);
            c = (unsigned)(rec.n_feat_cells + rec.n_odom_cells);
        }
        unsigned total;
        const unsigned below = ndt_block_scan(c, cnt, par, total);
        if (k < a.count) a.foff[k] = running + below;
        running += total;
    }
    if (threadIdx.x == 0) a.foff[a.count] = running;
}

// One wave per slot, one lane per cell pair: the slot's record and its cells at foff[slot]
__global__ __launch_bounds__(64) void ndt_fuserfeat_cells_kernel(NdtFuserFeatArgs a)
{
    const unsigned k = blockIdx.x, lane = threadIdx.x;
    if (k >= a.count) return;
    ndtgpu_fuser_feat_result rec;
    ff_gate(a, k, rec);
    const unsigned nf = (unsigned)rec.n_feat_cells, no = (unsigned)rec.n_odom_cells, MP = a.max_points;
    double cell[18];
    bool have = false;
    if (lane < nf) {
        const uint32_t *cr = a.corr + ((size_t)k * MP + lane) * 2;
        // (the matcher's indices are below the sets' counts; an index into the set's own storage all the same)
        const unsigned i = min(cr[0], MP - 1u), j = min(cr[1], MP - 1u);
        const unsigned cs = min(a.cur_idx[k], a.n_sets - 1u), ps = min(a.prev_idx[k], a.n_sets - 1u);
        const double *cp = a.bank_pos + ((size_t)cs * MP + i) * 3, *pp = a.bank_pos + ((size_t)ps * MP + j) * 3;
        const double cur3[3] = {cp[0], cp[1], cp[2]}, prev3[3] = {pp[0], pp[1], pp[2]};
        const bool as_is = a.pol.prev_in_map_frame && (a.slot_flags[k] & NDT_FUSERFEAT_PREV_MOVED);
        ndt_fuserfeat_cell_pair(a.pol, a.sensor_pose16, a.state[k].Tnow, cur3, prev3, as_is, cell);
        have = true;
    } else if (lane < nf + no) {
        ndt_fuserfeat_odom_cell(a.odom18 + 18 * (size_t)k, lane - nf == no - 1u, cell);
        have = true;
    }
    if (have) {                                                // (nf + no <= 64: the gate's room)
        double *out = a.cells + ((size_t)a.foff[k] + lane) * 18;
#pragma unroll
        for (int q = 0; q < 18; q++) out[q] = cell[q];
    }
    if (lane == 0) a.rec[k] = rec;
}

// One workgroup per slot, behind the pose update: prev <- cur (moved by Tmove where the call moves them), the append to map, the
// counts last.  cur is read only; cur, prev and map are three different sets (checked by the host).
__global__ __launch_bounds__(NDT_FUSERFEAT_COMMIT_THREADS) void ndt_fuserfeat_commit_kernel(NdtFuserFeatArgs a)
{
    const unsigned k = blockIdx.x, tid = threadIdx.x;
    if (k >= a.count) return;
    const unsigned MP = a.max_points, D = a.desc_len;
    const unsigned cs = a.cur_idx[k], ps = a.prev_idx[k], ms = a.map_idx[k], flags = a.slot_flags[k];
    if (cs >= a.n_sets || ps >= a.n_sets || ms >= a.n_sets) return;       // (never: the host refused such a call)
    const unsigned n = min(a.bank_count[cs], MP);
    const unsigned n_prev_old = min(a.bank_count[ps], MP);
    const unsigned nm = (flags & NDT_FUSERFEAT_RESET_MAP) ? 0u : min(a.bank_count[ms], MP);
    const bool append = (flags & NDT_FUSERFEAT_APPEND) != 0;
    const unsigned na = append ? min(n, MP - nm) : 0u;          // the first points that fit
    const double *T = a.Tmove16 + 16 * (size_t)k;
    const double *cpos = a.bank_pos + (size_t)cs * MP * 3;
    double *ppos = a.bank_pos + (size_t)ps * MP * 3, *mpos = a.bank_pos + (size_t)ms * MP * 3;
    for (unsigned i = tid; i < n; i += NDT_FUSERFEAT_COMMIT_THREADS) {
        const double p[3] = {cpos[3 * i], cpos[3 * i + 1], cpos[3 * i + 2]};
        double q[3] = {p[0], p[1], p[2]};
        if (flags & NDT_FUSERFEAT_MOVE) ndt_fuserfeat_move_point(T, p, q);
        ppos[3 * i] = q[0]; ppos[3 * i + 1] = q[1]; ppos[3 * i + 2] = q[2];
        if (i < na) { mpos[3 * (nm + i)] = q[0]; mpos[3 * (nm + i) + 1] = q[1]; mpos[3 * (nm + i) + 2] = q[2]; }
    }
    // descriptors: [bin][point], consecutive threads on consecutive points; prev's columns beyond n stay zero as
    // ndt_featmatch_pack_desc leaves them
    const double *cdesc = a.bank_desc + (size_t)cs * D * MP;
    double *pdesc = a.bank_desc + (size_t)ps * D * MP, *mdesc = a.bank_desc + (size_t)ms * D * MP;
    const unsigned lim = max(n, n_prev_old);
    for (unsigned e = tid; e < D * lim; e += NDT_FUSERFEAT_COMMIT_THREADS) {
        const unsigned bin = e / lim, i = e - bin * lim;
        const double v = i < n ? cdesc[(size_t)bin * MP + i] : 0.0;
        pdesc[(size_t)bin * MP + i] = v;
        if (i < na) mdesc[(size_t)bin * MP + nm + i] = v;
    }
    __syncthreads();
    if (tid == 0) {
        a.bank_count[ps] = n;
        if (na || (flags & NDT_FUSERFEAT_RESET_MAP)) a.bank_count[ms] = nm + na;
        ndtgpu_fuser_feat_result &r = a.rec[k];
        r.n_prev = (int32_t)n;
        r.n_map = (int32_t)(nm + na);
        r.map_appended = (int32_t)na;
        r.map_overflow = (append && n > MP - nm) ? 1 : 0;
    }
}

hipError_t ndt_launch_fuserfeat_cells(const NdtFuserFeatArgs &a, hipStream_t st)
{
    if (!a.count) return hipSuccess;
    hipLaunchKernelGGL(ndt_fuserfeat_offsets_kernel, dim3(1), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ndt_fuserfeat_cells_kernel, dim3(a.count), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t ndt_launch_fuserfeat_commit(const NdtFuserFeatArgs &a, hipStream_t st)
{
    if (!a.count) return hipSuccess;
    hipLaunchKernelGGL(ndt_fuserfeat_commit_kernel, dim3(a.count), dim3(NDT_FUSERFEAT_COMMIT_THREADS), 0, st, a);
    return hipGetLastError();
}
