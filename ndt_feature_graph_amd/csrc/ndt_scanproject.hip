// ndt_scanproject.hip -- laser-scan projection on CDNA4 (gfx950): ranges to fuser-ready clouds (include/ndtgpu.h "laser-scan
// projection").
//
// Replaces (reference call sites): projector_.projectLaser(*msg_in, cloud), the loop that drops the points outside the range gate
// and the z jitter of every kept point --
//   ndt_feature2d_fuser.cpp:747-765, :875-888       publish_graph_message.cpp:1356-1381, :1523-1535
//   ndt_feature_fuser.cpp:325-336, :378-390         ndt_feature2d_reg_node.cpp:75-86        ndt_feature2d_view.cpp:119-129
//
// Design: an ordered compaction per scan, tiled over the grid -- a fuser scan has up to 100 k beams, and one
// workgroup per scan would walk 100 tiles one after the other.  No workgroup waits on another: no atomics, no spin on memory, no
// grid barrier.  Two plain launches in stream order, (scans) x (tiles of a scan) workgroups of 256 threads each, a tile being
// T = 1024 consecutive beams of one scan:
//   1. ndt_scanproject_count_kernel: loads and the gate only, four beams a thread; the tile's count of kept beams goes to the
//      handle's scratch (one uint32 per tile).
//   2. ndt_scanproject_emit_kernel: the tile's workgroup sums the counts of its scan's tiles -- those in front of it give its first
//      row, all of them n_kept --, an integer sum through ndt_block_count; then per run of 256 beams it evaluates the gate again
//      (the ranges are 8 KiB a tile and still in the cache), ranks the kept beams with ndt_block_rank and writes their rows at
//      (kept before the tile) + (kept in the tile's earlier runs) + rank: the kept rows of a run are one contiguous block of
//      memory, written with dword stores by consecutive lanes.  The NaN pads of the rows of its own beam range at or beyond
//      n_kept follow; the scan's last tile writes n_kept.
// A beam's point depends on (i, angle_min, angle_increment, r, seed, scan_id, varz) alone and its row on the gates of the beams in
// front of it: the same bits in any batch, at any position and for any launch geometry.  fp64 with contraction off; the sine and
// cosine are the device library's, one each per kept beam (a table of them per call would be read once per scan and was not
// measured).
#include "ndt_scanproject.h"
#include "ndt_block.h"

struct NdtScanProjectArgs {
    const double *ranges;                         // [n_scans][n_beams]
    const unsigned long long *scan_id;            // [n_scans] or NULL: scan b has id b
    uint32_t *tile;                               // [n_scans][n_tiles] kept beams per tile
    uint32_t *xyz;                                // the destination as 4-byte words
    uint32_t *n_kept;                             // [n_scans] or NULL
    unsigned long long stride_words, map_stride_words;
    double angle_min, angle_increment;
    uint32_t n_beams, n_tiles;
    unsigned long long scan0;                     // the first scan of this launch
};

extern "C" __global__ __launch_bounds__(NDT_SCANPROJECT_THREADS) void ndt_scanproject_count_kernel(NdtScanProjectArgs a,
                                                                                                    NdtScanProjectParamsDev prm)
{
    __shared__ NdtBlockCounts<NDT_SCANPROJECT_WAVES> cnt;
    int par = 0;
    const unsigned long long b = a.scan0 + blockIdx.x / a.n_tiles;
    const uint32_t t = blockIdx.x % a.n_tiles;
    const double *r = a.ranges + b * a.n_beams;
    unsigned kept = 0;
#pragma unroll
    for (int s = 0; s < NDT_SCANPROJECT_SUBTILES; s++) {
        const uint32_t i = t * NDT_SCANPROJECT_TILE + s * NDT_SCANPROJECT_THREADS + threadIdx.x;
        kept += i < a.n_beams && ndt_scanproject_kept(r[i], prm.r_min, prm.r_max) ? 1u : 0u;
    }
    const unsigned n = ndt_block_count(kept, cnt, par);
    if (threadIdx.x == 0) a.tile[b * a.n_tiles + t] = n;
}

extern "C" __global__ __launch_bounds__(NDT_SCANPROJECT_THREADS) void ndt_scanproject_emit_kernel(NdtScanProjectArgs a,
                                                                                                   NdtScanProjectParamsDev prm)
{
    __shared__ NdtBlockCounts<NDT_SCANPROJECT_WAVES> cnt;
    int par = 0;
    const unsigned long long b = a.scan0 + blockIdx.x / a.n_tiles;
    const uint32_t t = blockIdx.x % a.n_tiles;
    const double *r = a.ranges + b * a.n_beams;
    uint32_t *out = a.xyz + b * a.map_stride_words;
    const unsigned long long id = a.scan_id ? a.scan_id[b] : b;
    const bool pad_word = a.stride_words >= 4;    // pcl::PointXYZ's fourth float
    const uint32_t one = __float_as_uint(1.0f), nan = 0x7FC00000u;

    // the kept beams in front of this tile and in the whole scan
    unsigned before = 0, all = 0;
    const uint32_t *tc = a.tile + b * a.n_tiles;
    for (uint32_t k = threadIdx.x; k < a.n_tiles; k += NDT_SCANPROJECT_THREADS) {
        const unsigned c = tc[k];
        before += k < t ? c : 0u;
        all += c;
    }
    unsigned at = ndt_block_count(before, cnt, par);
    const unsigned n_kept = ndt_block_count(all, cnt, par);

    for (int s = 0; s < NDT_SCANPROJECT_SUBTILES; s++) {
        const uint32_t i = t * NDT_SCANPROJECT_TILE + s * NDT_SCANPROJECT_THREADS + threadIdx.x;
        float p[3] = {0.f, 0.f, 0.f};
        const bool keep = i < a.n_beams && ndt_scanproject_beam(prm, a.angle_min, a.angle_increment, id, i, r[i], p);
        unsigned run;
        const unsigned row = at + ndt_block_rank(keep, cnt, par, run);
        at += run;
        if (!keep) continue;
        uint32_t *o = out + row * a.stride_words;             // row < n_kept <= n_beams: inside the scan's block
        o[0] = __float_as_uint(p[0]);
        o[1] = __float_as_uint(p[1]);
        o[2] = __float_as_uint(p[2]);
        if (pad_word) o[3] = one;
    }

    // the NaN pads of this tile's share of the rows n_kept .. n_beams - 1
    uint32_t pb, pe;
    ndt_scanproject_pad_range(t, a.n_beams, n_kept, pb, pe);
    const unsigned row_words = pad_word ? 4u : 3u;
    for (unsigned long long w = threadIdx.x; w < (unsigned long long)(pe - pb) * row_words; w += NDT_SCANPROJECT_THREADS) {
        const unsigned long long k = w / row_words;
        const unsigned c = (unsigned)(w - k * row_words);
        out[(pb + k) * a.stride_words + c] = c == 3 ? one : nan;
    }
    if (a.n_kept && t == a.n_tiles - 1 && threadIdx.x == 0) a.n_kept[b] = n_kept;
}

hipError_t ndt_scanproject_launch(const double *ranges_dev, const unsigned long long *scan_id_dev, size_t n_scans, size_t n_beams,
                                  double angle_min, double angle_increment, const NdtScanProjectParamsDev &prm, uint32_t *tile_dev,
                                  uint32_t *xyz_dev, size_t stride_words, size_t map_stride_words, uint32_t *n_kept_dev, hipStream_t st)
{
    NdtScanProjectArgs a{};
    a.ranges = ranges_dev;
    a.scan_id = scan_id_dev;
    a.tile = tile_dev;
    a.xyz = xyz_dev;
    a.n_kept = n_kept_dev;
    a.stride_words = stride_words;
    a.map_stride_words = map_stride_words;
    a.angle_min = angle_min;
    a.angle_increment = angle_increment;
    a.n_beams = (uint32_t)n_beams;
    a.n_tiles = ndt_scanproject_tiles(n_beams);
    const size_t per_launch = ndt_scanproject_scans_per_launch(n_beams);
    for (size_t first = 0; first < n_scans; first += per_launch) {
        const size_t n = n_scans - first < per_launch ? n_scans - first : per_launch;
        const dim3 grid((unsigned)(n * a.n_tiles));
        a.scan0 = first;
        hipLaunchKernelGGL(ndt_scanproject_count_kernel, grid, dim3(NDT_SCANPROJECT_THREADS), 0, st, a, prm);
        hipLaunchKernelGGL(ndt_scanproject_emit_kernel, grid, dim3(NDT_SCANPROJECT_THREADS), 0, st, a, prm);
    }
    return hipGetLastError();
}
