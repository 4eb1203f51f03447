// ndt_evalgroup.h -- the stage of the matcher (csrc/ndt_match.hip) that decides WHICH pairs are summed: one group of up to 64
// source cells is transformed, every mean finds its target cell (LazyGrid's index formula), the (2n+1)^3 neighbourhood is read
// as bit windows of the rank bitmap, a wave scan places the hits in the share's hit list, and the pair terms (ndt_pairterm.h)
// are taken from the list 64 at a time; the hit cache lets an evaluation use the list of the one before it.  Device only;
// depends on ndt_common.h, ndt_math.h, ndt_wave.h and ndt_pairterm.h alone, so that tests/native/evalgroup_checks.hip can run
// every function here by itself.  ndt_match.hip includes it inside its anonymous namespace.
#pragma once
#include "ndt_common.h"
#include "ndt_math.h"
#include "ndt_wave.h"
#include "ndt_pairterm.h"

// (section clocks and the launch timeline of the matcher's experiment builds: ndt_match.hip defines them before it includes this)
#ifndef NDT_PROF_T
#define NDT_PROF_T(k)
#endif
#ifndef NDT_TL
#define NDT_TL(pair, k)
#endif

// cell records and rank bitmaps live in device (global) memory: said in the pointer types, so that pointers that went
// through an LDS copy of a MapView are still dereferenced with global_load, not flat_load
typedef const NdtCell __attribute__((address_space(1))) *gcell_ptr;
typedef const unsigned long long __attribute__((address_space(1))) *grank_ptr;   // uint2 {bits, first rank} as one 8-byte word

struct MapView {
    grank_ptr rankmap;
    gcell_ptr cells;
    int n_cells;
    int sx, sy, sz;
    double cx, cy, cz, res;
    double hx, hy, hz;          // size / 2.0 per axis (the addend of LazyGrid's index formula)
    double inv_res;             // 1 / res when res is a power of two (the quotient of the index formula is then a product, bit for
                                // bit: 3 instructions instead of the 42 of three IEEE divisions per source cell and evaluation), else 0
};

// lazygrid_index with size / 2.0 handed in (a value the large-map kernels keep in scalar registers)
NDT_D int lazygrid_index_h(double p, double centre, double res, double half)
{
#pragma clang fp contract(off)
    double v = floor((p - centre) / res + 0.5) + half;
    if (!(v > -2.0e9 && v < 2.0e9)) return -1;
    return (int)v;
}
// the same for a cell size that is a power of two: x / 2^k == x * 2^-k in every case (both are the correctly rounded value of
// the same real number; no fused multiply-add: the product is rounded before 0.5 is added, like the quotient)
NDT_D int lazygrid_index_p2(double p, double centre, double inv_res, double half)
{
#pragma clang fp contract(off)
    double q = (p - centre) * inv_res;
    double v = floor(q + 0.5) + half;
    if (!(v > -2.0e9 && v < 2.0e9)) return -1;
    return (int)v;
}
NDT_D double pow2_reciprocal(double res)
{
    int e;
    return (res > 0.0 && frexp(res, &e) == 0.5 && e > -1000 && e < 1000) ? 1.0 / res : 0.0;
}

NDT_D double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (pl_swap_add, xor_lane, wave_sum_step: csrc/ndt_wave.h)
template <int N>
NDT_D double wave_sum_all(double (&v)[N])
{
    static_assert(N == 8 || N == 32, "padded value count");
    const unsigned lane = threadIdx.x & 63u;
    wave_sum_step<N, N / 2, 32>(v, lane);
    double t = v[0];
    if constexpr (N == 8) {          // 8 values: the lane bits 2, 1, 0 are left
        t += xor_lane<4>(t);
        t += xor_lane<2>(t);
        t += xor_lane<1>(t);
    } else {                         // 32 values: lane bit 0 is left
        t += xor_lane<1>(t);
    }
    return t;
}

NDT_D unsigned long long lanemask_lt()
{
    unsigned lane = threadIdx.x & 63u;
    return (lane == 0) ? 0ull : (~0ull >> (64u - lane));
}

struct HitCache {                   // what a wave remembers of its last evaluation (one group of source cells per wave)
    unsigned key;                   // the caller's key of the registration (0: nothing cached)
    int base;                       // first source cell of the group
    unsigned count;                 // hits in the list
    unsigned pad;
};

// What a wave carries through an evaluation: its accumulators, its hit queue, its share of the LDS.
template <bool WITH_H>
struct WaveEval {
    static constexpr int NACC = WITH_H ? 28 : 7;
#ifdef NDT_MATCH_PROF
    long long prof[6], pt, pt0;
#endif
    double acc[NACC];
    double *mysrc;
    uint32_t *myq;
    uint2 *mywin;
    int *mycell;
    HitCache *cache;
    unsigned terms;                  // wave-uniform
};

// inclusive scan over the 64 lanes in the vector ALU: DPP row shifts within the rows of 16, then the two row broadcasts
// hand the row totals on (no LDS round trips)
NDT_D unsigned wave_incl_scan_u32(unsigned v)
{
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, true);   // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, true);   // row_bcast:31 into rows 2 and 3
    return (unsigned)x;
}

template <bool WITH_H>
NDT_D double wave_totals(const WaveEval<WITH_H> &w);      // (defined below, used by eval_group's segment rows)

// TERM stage: the n (source lane, target cell) pairs at the head of the wave's list, 64 at a time; every lane does one
// dense pair term.  Without a Hessian the target cells of the next batch are fetched while this one is computed.
template <bool WITH_H, bool PLANAR = false>
NDT_D void term_list(WaveEval<WITH_H> &w, const MapView &tg, double lfd1, double lfd2, unsigned n)
{
    const unsigned lane = threadIdx.x & 63u;
    auto tile_m = [&](unsigned sl) { return d3{w.mysrc[0 * 64 + sl], w.mysrc[1 * 64 + sl], w.mysrc[2 * 64 + sl]}; };
    auto tile_C = [&](unsigned sl) {
        return sym3{w.mysrc[3 * 64 + sl], w.mysrc[4 * 64 + sl], w.mysrc[5 * 64 + sl],
                    w.mysrc[6 * 64 + sl], w.mysrc[7 * 64 + sl], w.mysrc[8 * 64 + sl]};
    };
    // The list entries and target cells of the NEXT batch are fetched while this one is computed.  Every lane fetches
    // (lanes past the end of the list fetch its last entry again): a fetch under a lane mask is a branch the wave may
    // skip, and the wait counts the compiler then has to use (the smaller of the two paths) would make every batch wait
    // for the prefetch it has just issued.
    auto fetch = [&](unsigned e, uint32_t &en, d3 &mu, sym3 &Cj) {
        en = w.myq[min(e + lane, n - 1u)];
#ifdef NDT_EXP_FIXED_TARGET
        gcell_ptr tc = tg.cells + (en & 0x1u);
#else
        gcell_ptr tc = tg.cells + (en & 0xFFFFFFu);
#endif
        mu = d3{tc->mean[0], tc->mean[1], tc->mean[2]};
        Cj = sym3{tc->cov[0], tc->cov[1], tc->cov[2], tc->cov[3], tc->cov[4], tc->cov[5]};
    };
    if (n == 0u) return;
    if constexpr (WITH_H) {
        uint32_t en0, en1;
        d3 mu0, mu1;
        sym3 Cj0, Cj1;
        fetch(0u, en0, mu0, Cj0);
#pragma unroll 1
        for (unsigned e0 = 0; e0 < n; e0 += 64u) {
            fetch(e0 + 64u, en1, mu1, Cj1);
            __builtin_amdgcn_sched_barrier(0);       // (the loads stay above the arithmetic)
            if (e0 + lane < n) pair_term<true, PLANAR>(tile_m(en0 >> 24), tile_C(en0 >> 24), mu0, Cj0, lfd1, lfd2, w.acc);
            en0 = en1; mu0 = mu1; Cj0 = Cj1;
        }
    } else {
        // two register sets that take turns (no rotation moves: they would be a tenth of the gradient-only term)
        uint32_t enA, enB;
        d3 muA, muB;
        sym3 CjA, CjB;
        fetch(0u, enA, muA, CjA);
#pragma unroll 1
        for (unsigned e0 = 0; e0 < n; e0 += 128u) {
            fetch(e0 + 64u, enB, muB, CjB);
            __builtin_amdgcn_sched_barrier(0);
            if (e0 + lane < n) pair_term<false, PLANAR>(tile_m(enA >> 24), tile_C(enA >> 24), muA, CjA, lfd1, lfd2, w.acc);
            fetch(e0 + 128u, enA, muA, CjA);
            __builtin_amdgcn_sched_barrier(0);
            if (e0 + 64u + lane < n) pair_term<false, PLANAR>(tile_m(enB >> 24), tile_C(enB >> 24), muB, CjB, lfd1, lfd2, w.acc);
        }
    }
    w.terms += n;
}

// One group of up to 64 source cells base + k stride < end: transform (pseudoTransformNDT), PROBE, TERM.
//   PROBE reads the (2n+1)^3 slots around every lane's cell as bit windows of the map's rank bitmap (1 bit per slot +
//   the rank of every 32-slot word's first Gaussian cell): slots are z-fastest, so the neighbours along z are one run
//   of <= W bits, and in a flat map (sz <= n+1: every z-layer is a neighbour) the whole (y, z) block of one x is a
//   single run of <= W*sz bits.  Cells are ranked in slot order, so the k-th set bit of a run is cell `first + k`: no
//   per-slot lookups.  Every lane counts its hits, a scan over the wave gives it its place in the wave's hit list, and
//   the lanes fill the list without talking to each other.
//   The list only depends on the target-grid cells the transformed means fall into.  `cache_key` != 0 names the
//   registration this evaluation belongs to: when the wave's last evaluation had the same key and group and no mean
//   has left its cell since (the small steps of a line search), PROBE is skipped and the list is used again.
// On return every hit of the group has been summed into w.acc.
// SEG: the 64 lanes (cells) of the group are cut into segments of `seg_lanes` lanes -- the chunks of the grid-barrier
// matcher -- and every segment gets its own hit list, its own pass over the pair terms and its own row of wave totals
// (seg_rows + segment * seg_stride; the accumulators are zero again afterwards): TRANSFORM and PROBE run once for all 64
// cells, while the sums of a segment are bit for bit those of a group that holds that segment's cells alone.
template <int NN, bool WITH_H, int QL, bool SEG = false, bool KEEP_RUNS = false, bool PLANAR = false>
NDT_D void eval_group(WaveEval<WITH_H> &w, const MapView &tg, gcell_ptr src, int base, int stride, int end,
                      const rigid &T, double lfd1, double lfd2, unsigned cache_key, unsigned seg_lanes = 64u,
                      double *seg_rows = nullptr, unsigned seg_stride = 0u)
{
    constexpr int W = 2 * NN + 1;
    constexpr int NDT_QL = QL;
    const unsigned lane = threadIdx.x & 63u;
    const int i = base + (int)lane * stride;
    const bool vi = i < end;
    int ix = 0, iy = 0, iz = 0;
    NDT_PROF_T(4)
    // (wave-uniform: a branch, not a select.  Only in the persistent matcher of the 2D batches, whose map views live in LDS: the
    //  large-map kernels -- KEEP_RUNS -- hold theirs in scalar registers and have none to spare for the reciprocal)
    const bool res_pow2 = !KEEP_RUNS && __builtin_amdgcn_readfirstlane(tg.inv_res != 0.0 ? 1 : 0) != 0;
    if (vi) {
        gcell_ptr sc = src + i;
        d3 m0 = {sc->mean[0], sc->mean[1], sc->mean[2]};
        sym3 C0 = {sc->cov[0], sc->cov[1], sc->cov[2], sc->cov[3], sc->cov[4], sc->cov[5]};
        d3 m = apply(T, m0);                    // pseudoTransformNDT: mean' = T mean
        sym3 C = rotate_cov(T.r, C0);           //                      cov'  = R cov R^T
        w.mysrc[0 * 64 + lane] = m.x; w.mysrc[1 * 64 + lane] = m.y; w.mysrc[2 * 64 + lane] = m.z;
        w.mysrc[3 * 64 + lane] = C.xx; w.mysrc[4 * 64 + lane] = C.xy; w.mysrc[5 * 64 + lane] = C.xz;
        w.mysrc[6 * 64 + lane] = C.yy; w.mysrc[7 * 64 + lane] = C.yz; w.mysrc[8 * 64 + lane] = C.zz;
        if (res_pow2) {                                     // getCellsForPoint(mean, n_neighbours)
            ix = lazygrid_index_p2(m.x, tg.cx, tg.inv_res, tg.hx);
            iy = lazygrid_index_p2(m.y, tg.cy, tg.inv_res, tg.hy);
            iz = lazygrid_index_p2(m.z, tg.cz, tg.inv_res, tg.hz);
        } else {
            ix = lazygrid_index_h(m.x, tg.cx, tg.res, tg.hx);
            iy = lazygrid_index_h(m.y, tg.cy, tg.res, tg.hy);
            iz = lazygrid_index_h(m.z, tg.cz, tg.res, tg.hz);
        }
    }
    NDT_PROF_T(0)
    const HitCache hc = *w.cache;
    const bool moved = vi && (w.mycell[lane] != ix || w.mycell[64 + lane] != iy || w.mycell[128 + lane] != iz);
    const bool reuse = cache_key != 0u && hc.key == cache_key && hc.base == base && !ndt_ballot(moved);
    if (vi && !reuse) { w.mycell[lane] = ix; w.mycell[64 + lane] = iy; w.mycell[128 + lane] = iz; }
    // flat form only when every lane's z-neighbourhood is the whole column (a source cell that lies two or
    // more cells above / below a thin map sees only part of it, or nothing): wave-uniform
    const bool flat = tg.sz <= NN + 1 && !ndt_ballot(vi && !(iz - NN <= 0 && iz + NN >= tg.sz - 1));
    const int zlo = flat ? 0 : max(iz - NN, 0), zhi = flat ? tg.sz - 1 : min(iz + NN, tg.sz - 1);
    grank_ptr rmw = tg.rankmap;
    // The runs are fetched W at a time (flat map: the W runs of the W x-neighbours; otherwise, per x, the W runs of the
    // y-neighbours): all 2 W loads are in flight together.
    auto windows = [&](int outer, unsigned (&bits)[W], unsigned (&id0)[W]) {
        uint2 wa[W], wb[W];
        unsigned sh[W];
        int len[W];
#pragma unroll
        for (int q = 0; q < W; q++) {
            const int dx = flat ? q - NN : outer - NN;
            const int xx = ix + dx;
            const bool xok = vi && xx >= 0 && xx < tg.sx && zlo <= zhi;
            const int ylo = flat ? max(iy - NN, 0) : iy - NN + q;
            const int yhi = flat ? min(iy + NN, tg.sy - 1) : ylo;
            const bool ok = xok && ylo <= yhi && ylo >= 0 && yhi < tg.sy;
            const unsigned s0 = ok ? (unsigned)((xx * tg.sy + ylo) * tg.sz + zlo) : 0u;
            len[q] = ok ? (flat ? (yhi - ylo + 1) * tg.sz : zhi - zlo + 1) : 0;   // <= 28 bits
            sh[q] = s0 & 31u;
            const unsigned long long ra = rmw[s0 >> 5], rb = rmw[(s0 >> 5) + 1u];
            wa[q] = make_uint2((unsigned)ra, (unsigned)(ra >> 32));
            wb[q] = make_uint2((unsigned)rb, (unsigned)(rb >> 32));
        }
#pragma unroll
        for (int q = 0; q < W; q++) {
            bits[q] = __builtin_amdgcn_alignbit(wb[q].x, wa[q].x, sh[q]) & ((1u << len[q]) - 1u);
            const unsigned lowa = wa[q].x >> sh[q];          // the window's part of the first word
            id0[q] = lowa ? wa[q].y + (unsigned)__popc(wa[q].x & ((1u << sh[q]) - 1u)) : wb[q].y;
        }
    };
    uint2 *win = w.mywin + lane;
    unsigned cnt = 0;
    // thick maps (W x W runs of <= W bits per lane): the decoded runs stay in REGISTERS, (bits << 24 | first cell rank), for
    // the pass that fills the hit list -- fetching and decoding them a second time there was a third of a 3D evaluation
    // (16 k of 48 k clocks per 512 cells, tools/evalloop3d.py).  The largest neighbourhood (7 x 7 runs) fetches twice.
    // (KEEP_RUNS: the kernels that serve large maps; the persistent matcher of the 2D batches has no registers to spare)
    constexpr bool KEEP = KEEP_RUNS && W <= 5;
    unsigned pk[KEEP ? W * W : 1];
#pragma unroll
    for (int i = 0; i < (KEEP ? W * W : 1); i++) pk[i] = 0u;
    if (!reuse) {
        if (flat) {
            unsigned bits[W], id0[W];
            windows(0, bits, id0);
#pragma unroll
            for (int q = 0; q < W; q++) {
                win[q * 64] = make_uint2(bits[q], id0[q]);
                cnt += (unsigned)__popc(bits[q]);
            }
        } else if constexpr (KEEP) {
            // two rounds of 2 W loads in flight: round k + 1 is issued before round k is decoded (all W rounds at once would
            // need 100 registers; one at a time pays W dependent round trips)
            uint2 wa[2][W], wb[2][W];
            unsigned shf[2][W];
            int len[2][W];
            auto issue = [&](int outer, int slot) __attribute__((always_inline)) {
                const int xx = ix + outer - NN;
                const bool xok = vi && xx >= 0 && xx < tg.sx && zlo <= zhi;
#pragma unroll
                for (int q = 0; q < W; q++) {
                    const int yy = iy - NN + q;
                    const bool ok = xok && yy >= 0 && yy < tg.sy;
                    const unsigned s0 = ok ? (unsigned)((xx * tg.sy + yy) * tg.sz + zlo) : 0u;
                    len[slot][q] = ok ? zhi - zlo + 1 : 0;
                    shf[slot][q] = s0 & 31u;
                    const unsigned long long ra = rmw[s0 >> 5], rb = rmw[(s0 >> 5) + 1u];
                    wa[slot][q] = make_uint2((unsigned)ra, (unsigned)(ra >> 32));
                    wb[slot][q] = make_uint2((unsigned)rb, (unsigned)(rb >> 32));
                }
            };
            issue(0, 0);
#pragma unroll
            for (int outer = 0; outer < W; outer++) {
                const int cur = outer & 1;
                if (outer + 1 < W) issue(outer + 1, cur ^ 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < W; q++) {
                    const unsigned bits = __builtin_amdgcn_alignbit(wb[cur][q].x, wa[cur][q].x, shf[cur][q]) & ((1u << len[cur][q]) - 1u);
                    const unsigned lowa = wa[cur][q].x >> shf[cur][q];          // the window's part of the first word
                    const unsigned id0 = lowa ? wa[cur][q].y + (unsigned)__popc(wa[cur][q].x & ((1u << shf[cur][q]) - 1u)) : wb[cur][q].y;
                    pk[outer * W + q] = (bits << 24) | (id0 & 0xFFFFFFu);
                    cnt += (unsigned)__popc(bits);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll 1
            for (int outer = 0; outer < W; outer++) {
                unsigned bits[W], id0[W];
                windows(outer, bits, id0);
#pragma unroll
                for (int q = 0; q < W; q++) cnt += (unsigned)__popc(bits[q]);
            }
        }
    }
    // entries [p0, p1) of a hit list in which this lane's `cnt_l` hits start at `off_l` go to the queue.  FROM_REGS: the
    // runs of a thick map come from the registers the count pass left them in (only the FIRST fill of a group may: the
    // registers must not live across the pair terms); otherwise they are fetched and decoded again.
    auto put_run = [&](unsigned b_, unsigned id, unsigned &gi, unsigned p0, unsigned p1) __attribute__((always_inline)) {
        while (b_) {
            if (gi >= p0 && gi < p1) w.myq[gi - p0] = (lane << 24) | id;
            gi += 1u; id += 1u; b_ &= b_ - 1u;
        }
    };
    auto fill_flat = [&](unsigned &gi, unsigned p0, unsigned p1) __attribute__((always_inline)) {
#pragma unroll 1
        for (int q = 0; q < W; q++) {
            const uint2 v = win[q * 64];
            put_run(v.x, v.y, gi, p0, p1);
        }
    };
    auto fill_regs = [&](unsigned off_l, unsigned cnt_l, unsigned p0, unsigned p1) __attribute__((always_inline)) {
        if (!reuse && cnt_l != 0u && off_l < p1 && off_l + cnt_l > p0) {
            unsigned gi = off_l;
            if (flat) {
                fill_flat(gi, p0, p1);
            } else if constexpr (KEEP) {
                // branch-free: every bit of every run stores -- a set bit into the list, a clear one into a word of the
                // (idle, on thick maps) window buffer -- and advances the list by its value.  The loops over the set bits of
                // a run cost a wave the longest run of its 64 lanes per run plus a branch per step: 10 k clocks per 512 cells.
                // (only for the one-pass fill: p0 = 0 and the whole list fits)
                uint32_t *const dummy = reinterpret_cast<uint32_t *>(w.mywin) + lane;
                uint32_t *q = w.myq + gi;
#pragma unroll
                for (int i = 0; i < W * W; i++) {
                    const unsigned b_ = pk[i] >> 24;
                    unsigned id = (lane << 24) | (pk[i] & 0xFFFFFFu);
#pragma unroll
                    for (int b = 0; b < W; b++) {
                        const unsigned on = (b_ >> b) & 1u;
                        *(on ? q : dummy) = id;
                        q += on; id += on;
                    }
                }
            } else {                                      // (no registers kept: fetch and decode again)
#pragma unroll 1
                for (int outer = 0; outer < W; outer++) {
                    unsigned bits[W], id0[W];
                    windows(outer, bits, id0);
#pragma unroll
                    for (int q = 0; q < W; q++) put_run(bits[q], id0[q], gi, p0, p1);
                }
            }
        }
    };
    auto fill = [&](unsigned off_l, unsigned cnt_l, unsigned p0, unsigned p1) __attribute__((always_inline)) {
        if (!reuse && cnt_l != 0u && off_l < p1 && off_l + cnt_l > p0) {
            unsigned gi = off_l;
            if (flat) {
                fill_flat(gi, p0, p1);
            } else {
#pragma unroll 1
                for (int outer = 0; outer < W; outer++) {
                    unsigned bits[W], id0[W];
                    windows(outer, bits, id0);
#pragma unroll
                    for (int q = 0; q < W; q++) put_run(bits[q], id0[q], gi, p0, p1);
                }
            }
        }
    };
    // the list is materialised NDT_QL hits at a time (one pass unless the neighbourhoods are dense 3D ones), each
    // pass followed by its pair terms
    // (`filled`: the list already holds its first -- then only -- pass)
    auto run_list = [&](unsigned off_l, unsigned cnt_l, unsigned total_l, bool filled) __attribute__((always_inline)) {
#pragma unroll 1
        for (unsigned p0 = 0; p0 < total_l; p0 += (unsigned)NDT_QL) {
            const unsigned p1 = min(total_l, p0 + (unsigned)NDT_QL);
            if (!(filled && p0 == 0u)) fill(off_l, cnt_l, p0, p1);
            ndt_wave_sync();                             // list entries and tile columns were written by other lanes
            NDT_PROF_T(2)
            term_list<WITH_H, PLANAR>(w, tg, lfd1, lfd2, p1 - p0);
            NDT_PROF_T(3)
            ndt_wave_sync();                             // the next pass (or group) overwrites the list and the tile
        }
    };
    unsigned total = hc.count, my_off = 0u;
    if constexpr (SEG) {
        constexpr int NACC = WaveEval<WITH_H>::NACC, SH = WITH_H ? 1 : 3;
        NDT_PROF_T(1)
        const unsigned incl = wave_incl_scan_u32(cnt);
        const unsigned total_all = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
        const unsigned off_all = incl - cnt;
        const unsigned long long have = ndt_ballot(vi);
        const unsigned n_seg = have ? (63u - (unsigned)__builtin_clzll(have)) / seg_lanes + 1u : 0u;   // segments that hold cells
        // list offset at which segment x starts (x == n_seg: the end of the list)
        auto seg_off = [&](unsigned x) -> unsigned {
            return x * seg_lanes < 64u && x < n_seg ? (unsigned)__builtin_amdgcn_readlane((int)off_all, (int)(x * seg_lanes)) : total_all;
        };
        auto emit_row = [&](unsigned sg) __attribute__((always_inline)) {
            const double tot = wave_totals<WITH_H>(w);
            double *row = seg_rows + sg * seg_stride;
            if ((lane & ((1u << SH) - 1u)) == 0u && (lane >> SH) < (unsigned)NACC) row[lane >> SH] = tot;
            if (lane == 0) row[28] = (double)w.terms;
            w.terms = 0;
#pragma unroll
            for (int k = 0; k < NACC; k++) w.acc[k] = 0.0;
        };
        // the terms of segments [sg, e), whose hits are in the list from offset o0 on: every segment on its own
        auto seg_terms = [&](unsigned sg, unsigned e, unsigned o0) __attribute__((always_inline)) {
            uint32_t *const q0 = w.myq;
#pragma unroll 1
            for (unsigned x = sg; x < e; x++) {
                const unsigned a = seg_off(x), b = seg_off(x + 1u);
                w.myq = q0 + (a - o0);
                term_list<WITH_H>(w, tg, lfd1, lfd2, b - a);
                emit_row(x);
            }
            w.myq = q0;
        };
        // the usual case: ONE fill, from the registers, for all segments -- before the loop, so that the registers are dead
        // when the pair terms start
        const bool all_in = total_all <= (unsigned)NDT_QL;
        if (all_in) fill_regs(off_all, cnt, 0u, total_all);
#pragma unroll 1
        for (unsigned sg = 0; sg < n_seg;) {
            const unsigned o0 = seg_off(sg);
            unsigned e = sg + 1u;
            if (all_in) e = n_seg;
            else while (e < n_seg && seg_off(e + 1u) - o0 <= (unsigned)NDT_QL) e++;   // whole segments that fit into the list together
            const unsigned o1 = seg_off(e);
            const bool in = lane >= sg * seg_lanes && lane < e * seg_lanes;
            const unsigned cnt_s = in ? cnt : 0u, off_s = in ? off_all - o0 : 0u;
            if (o1 - o0 > (unsigned)NDT_QL) {             // one segment with more hits than the list holds: its own passes
                run_list(off_s, cnt_s, o1 - o0, false);
                emit_row(sg);
            } else {                                      // one pass of window fetches for all of them, then their terms in turn
                if (!all_in) fill(off_s, cnt_s, 0u, o1 - o0);
                ndt_wave_sync();
                seg_terms(sg, e, o0);
                ndt_wave_sync();
            }
            sg = e;
        }
        return;
    }
    if (!reuse) {
        const unsigned incl = wave_incl_scan_u32(cnt);
        total = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
        my_off = incl - cnt;
    }
    NDT_PROF_T(1)
    const bool one_pass = total <= (unsigned)NDT_QL;      // the usual case: one fill, from the registers (dead after it)
    if (one_pass) fill_regs(my_off, cnt, 0u, total);
    run_list(my_off, cnt, total, one_pass);
    if (lane == 0 && !reuse) {
        HitCache nc;
        nc.key = total <= (unsigned)NDT_QL ? cache_key : 0u;
        nc.base = base; nc.count = total; nc.pad = 0u;
        *w.cache = nc;
    }
}

// wave-wide totals of the accumulators: on return lane l holds value (l >> SH) in `tot` when (l & ((1 << SH) - 1)) == 0
template <bool WITH_H>
NDT_D double wave_totals(const WaveEval<WITH_H> &w)
{
    constexpr int NACC = WaveEval<WITH_H>::NACC, NP = WITH_H ? 32 : 8;
    double vv[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) vv[k] = k < NACC ? w.acc[k] : 0.0;
    return wave_sum_all<NP>(vv);
}
