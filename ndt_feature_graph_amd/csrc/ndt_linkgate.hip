// ndt_linkgate.hip -- link gating on CDNA4 (gfx950): which loop-closure links exist (include/ndtgpu.h "link gating").
//
// Replaces (reference call sites):
//   NDTFeatureGraph::computeAllPossibleLinks' enumeration   ndt_feature/src/ndt_feature_src/ndt_feature_graph.cpp:395-405
//   NDTFeatureGraph::getValidLinks                          ndt_feature_graph.cpp:527-556 (the loop ndt_feature_graph_opt.cpp:152-173)
//
// Design: an ordered selection without any workgroup waiting on another -- no look-back spin, no grid barrier,
// no atomics.  Three plain launches in stream order:
//   1. ndt_linkgate_flag_kernel<MODE>: a workgroup of 256 threads takes a TILE of 1024 consecutive items (pairs in
//      computeAllPossibleLinks' order, or links), evaluates the gate of four items per thread and leaves the tile's count;
//   2. ndt_linkgate_scan_kernel: ONE workgroup turns the tile counts into the number kept before each tile, and the total;
//   3. ndt_linkgate_emit_kernel<MODE>: the tile's workgroup evaluates the gates AGAIN (a flag array would cost a write and a read
//      of every item; the gate is 30 flops on 12 doubles that are still in the cache), ranks the kept items of each run of 256 by
//      ndt_block_rank and writes them at (kept before the tile) + (kept in the tile's earlier runs) + rank, up to the capacity.
// An item's position depends on the flags of the items before it only, and a flag on the item and the thresholds only: the
// output is in input order and the same bits on any run and in any batch.
// The gather (ndt_linkgate_gather_kernel) moves 4-byte words, one lane per word, consecutive lanes on consecutive words of a row:
// reads and writes of a row are contiguous.  It reads the count on the device and runs a grid-stride loop up to it.
#include "ndt_linkgate.h"
#include "ndt_block.h"
#include <algorithm>

enum { NDT_LINKGATE_PAIRS = 0, NDT_LINKGATE_LINKS = 1 };

struct NdtLinkGateItems {
    unsigned long long n_items;                   // pairs or links
    const uint32_t *ref, *mov;                    // LINKS: the links' node indices
    const double *T16, *score;                    // LINKS: the links' poses and scores (score may be NULL)
};

// the gate of item `it`; PAIRS: also the pair
template <int MODE>
NDT_D bool ndt_linkgate_flag(const NdtLinkGateView &v, const NdtLinkGateParamsDev &prm, const NdtLinkGateItems &in, unsigned long long it,
                             uint32_t &i, uint32_t &j)
{
    if (it >= in.n_items) return false;
    if (MODE == NDT_LINKGATE_PAIRS) {
        ndt_linkgate_decode_pair(it, v.n_nodes, i, j);
        return ndt_linkgate_candidate(v.nodes, i, j, prm);
    }
    i = in.ref[it];
    j = in.mov[it];
    return ndt_linkgate_link_valid(v.nodes, v.n_nodes, i, j, in.T16 + 16 * it, in.score ? in.score + it : nullptr, prm);
}

template <int MODE>
__global__ __launch_bounds__(NDT_LINKGATE_THREADS) void ndt_linkgate_flag_kernel(NdtLinkGateView v, NdtLinkGateParamsDev prm,
                                                                                  NdtLinkGateItems in)
{
    __shared__ NdtBlockCounts<NDT_LINKGATE_WAVES> cnt;
    int par = 0;
    const unsigned long long base = (unsigned long long)blockIdx.x * NDT_LINKGATE_TILE + threadIdx.x;
    unsigned kept = 0;
#pragma unroll
    for (int s = 0; s < NDT_LINKGATE_SUBTILES; s++) {
        uint32_t i, j;
        kept += ndt_linkgate_flag<MODE>(v, prm, in, base + (unsigned long long)s * NDT_LINKGATE_THREADS, i, j) ? 1u : 0u;
    }
    const unsigned n = ndt_block_count(kept, cnt, par);
    if (threadIdx.x == 0) v.tile[blockIdx.x] = n;
}

// tile[t] <- the sum of tile[0 .. t), *total <- the sum of all: one workgroup, chunks of 1024 tiles with a running carry
extern "C" __global__ __launch_bounds__(NDT_LINKGATE_SCAN_THREADS) void ndt_linkgate_scan_kernel(uint32_t *__restrict__ tile,
                                                                                                  unsigned n_tiles,
                                                                                                  uint32_t *__restrict__ total)
{
    __shared__ unsigned wsum[NDT_LINKGATE_SCAN_THREADS / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0;
    for (unsigned at = 0; at < n_tiles; at += NDT_LINKGATE_SCAN_THREADS) {
        const unsigned t = at + threadIdx.x;
        const unsigned c = t < n_tiles ? tile[t] : 0u;
        const unsigned incl = ndt_wave_incl_scan(c);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned below = 0, all = 0;
        for (unsigned w = 0; w < NDT_LINKGATE_SCAN_THREADS / 64; w++) {
            const unsigned s = wsum[w];
            below += w < wave ? s : 0u;
            all += s;
        }
        if (t < n_tiles) tile[t] = carry + below + (incl - c);
        carry += all;
        __syncthreads();                          // (wsum is rewritten by the next chunk)
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int MODE>
__global__ __launch_bounds__(NDT_LINKGATE_THREADS) void ndt_linkgate_emit_kernel(NdtLinkGateView v, NdtLinkGateParamsDev prm,
                                                                                  NdtLinkGateItems in, uint32_t *__restrict__ out_a,
                                                                                  uint32_t *__restrict__ out_b, double *__restrict__ out_T,
                                                                                  unsigned long long capacity)
{
    __shared__ NdtBlockCounts<NDT_LINKGATE_WAVES> cnt;
    int par = 0;
    const unsigned long long base = (unsigned long long)blockIdx.x * NDT_LINKGATE_TILE + threadIdx.x;
    unsigned long long at = v.tile[blockIdx.x];
    for (int s = 0; s < NDT_LINKGATE_SUBTILES; s++) {
        const unsigned long long it = base + (unsigned long long)s * NDT_LINKGATE_THREADS;
        uint32_t i = 0, j = 0;
        const bool keep = ndt_linkgate_flag<MODE>(v, prm, in, it, i, j);
        unsigned run;
        const unsigned long long pos = at + ndt_block_rank(keep, cnt, par, run);
        at += run;
        if (!keep) continue;
        if (MODE == NDT_LINKGATE_PAIRS) {
            if (pos >= capacity) continue;
            out_a[pos] = i;
            out_b[pos] = j;
            if (out_T) {
                double T[16];
                ndt_linkgate_relative(v.nodes + 16 * (size_t)i, v.nodes + 16 * (size_t)j, T);
#pragma unroll
                for (int k = 0; k < 16; k++) out_T[16 * pos + k] = T[k];
            }
        } else {
            out_a[pos] = (uint32_t)it;            // the handle's keep list: room for every link
            if (out_b && pos < capacity) out_b[pos] = (uint32_t)it;
        }
    }
}

extern "C" __global__ __launch_bounds__(NDT_LINKGATE_THREADS) void ndt_linkgate_gather_kernel(const uint32_t *__restrict__ keep,
                                                                                               const uint32_t *__restrict__ count,
                                                                                               unsigned long long max_rows,
                                                                                               const uint32_t *__restrict__ src,
                                                                                               unsigned row_words, uint32_t *__restrict__ dst,
                                                                                               unsigned long long dst_first_row)
{
    const unsigned long long rows = min((unsigned long long)*count, max_rows);
    const unsigned long long words = rows * row_words, step = (unsigned long long)gridDim.x * NDT_LINKGATE_THREADS;
    for (unsigned long long w = (unsigned long long)blockIdx.x * NDT_LINKGATE_THREADS + threadIdx.x; w < words; w += step) {
        const unsigned long long k = w / row_words;
        const unsigned c = (unsigned)(w - k * row_words);
        dst[(dst_first_row + k) * row_words + c] = src[(unsigned long long)keep[k] * row_words + c];
    }
}

static unsigned tiles_of(unsigned long long n_items) { return (unsigned)((n_items + NDT_LINKGATE_TILE - 1) / NDT_LINKGATE_TILE); }

template <int MODE>
static hipError_t launch_select(const NdtLinkGateView &v, const NdtLinkGateParamsDev &prm, const NdtLinkGateItems &in, uint32_t *total,
                                uint32_t *out_a, uint32_t *out_b, double *out_T, size_t capacity, hipStream_t st)
{
    const unsigned n_tiles = tiles_of(in.n_items);
    if (n_tiles)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ndt_linkgate_flag_kernel<MODE>), dim3(n_tiles), dim3(NDT_LINKGATE_THREADS), 0, st, v, prm, in);
    hipLaunchKernelGGL(ndt_linkgate_scan_kernel, dim3(1), dim3(NDT_LINKGATE_SCAN_THREADS), 0, st, v.tile, n_tiles, total);
    if (n_tiles)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ndt_linkgate_emit_kernel<MODE>), dim3(n_tiles), dim3(NDT_LINKGATE_THREADS), 0, st, v, prm, in,
                           out_a, out_b, out_T, (unsigned long long)capacity);
    return hipGetLastError();
}

hipError_t ndt_linkgate_launch_candidates(const NdtLinkGateView &v, const NdtLinkGateParamsDev &prm, uint32_t *ref_dev, uint32_t *mov_dev,
                                          double *T16_dev, size_t capacity, hipStream_t st)
{
    NdtLinkGateItems in{};
    in.n_items = ndt_linkgate_pairs_before(v.n_nodes ? v.n_nodes - 1u : 0u, v.n_nodes ? v.n_nodes : 1u);     // n (n - 1) / 2
    return launch_select<NDT_LINKGATE_PAIRS>(v, prm, in, v.total, ref_dev, mov_dev, T16_dev, capacity, st);
}

hipError_t ndt_linkgate_launch_valid(const NdtLinkGateView &v, const NdtLinkGateParamsDev &prm, size_t n_links, const uint32_t *ref_dev,
                                     const uint32_t *mov_dev, const double *T16_dev, const double *score_dev, uint32_t *keep_dev,
                                     size_t capacity, hipStream_t st)
{
    NdtLinkGateItems in{};
    in.n_items = n_links;
    in.ref = ref_dev;
    in.mov = mov_dev;
    in.T16 = T16_dev;
    in.score = score_dev;
    return launch_select<NDT_LINKGATE_LINKS>(v, prm, in, v.total + 1, v.keep, keep_dev, nullptr, capacity, st);
}

hipError_t ndt_linkgate_launch_gather(const NdtLinkGateView &v, size_t max_rows, const uint32_t *src_dev, size_t row_words, uint32_t *dst_dev,
                                      size_t dst_first_row, hipStream_t st)
{
    if (max_rows == 0 || row_words == 0) return hipSuccess;
    const unsigned long long words = (unsigned long long)max_rows * row_words;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((words + NDT_LINKGATE_THREADS - 1) / NDT_LINKGATE_THREADS, 1u << 16);
    hipLaunchKernelGGL(ndt_linkgate_gather_kernel, dim3(blocks), dim3(NDT_LINKGATE_THREADS), 0, st, v.keep, v.total + 1,
                       (unsigned long long)max_rows, src_dev, (unsigned)row_words, dst_dev, (unsigned long long)dst_first_row);
    return hipGetLastError();
}
