// ndt_block.h -- reductions and ordered compaction over ONE workgroup (product code, device only), for the kernels that give a
// workgroup an item of their batch and separate their phases by __syncthreads: ndt_pgo.hip, ndt_mcl.hip, ndt_featmatch.hip,
// ndt_featextract.hip.
//
// THE ORDER of a floating-point sum, part of those kernels' contract (a result is the same bits whichever batch its item runs
// in): per wave v += lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 in that order, then the waves' sums added in ascending wave order
// starting from 0.0.  tests/featmatch_model.py and tests/flirt_model.py restate it operation for operation, and
// tests/native/block_checks.hip restates it on the host.  Integer sums are exact: their order is free.
//
// LDS: a kernel embeds an NdtBlockSums / NdtBlockCounts in its own shared struct (or declares one __shared__) and holds a
// parity, initially 0, for each.  Every call is made by all threads of the workgroup, writes the half of the block its parity
// names, has exactly ONE __syncthreads, reads that half and flips the parity: the next call writes the other half, and the one
// after it starts behind that call's barrier, which no thread passes before all have read this one's half.
#pragma once
#include "ndt_wave.h"

template <int WAVES, int N>
struct NdtBlockSums {
    double v[2][WAVES][N];
};

template <int WAVES>
struct NdtBlockCounts {
    unsigned v[2][WAVES];
};

// the sum of v over the 64 lanes, in every lane, in the vector ALU
NDT_D double ndt_wave_sum(double v)
{
    v = pl_swap_add(v, v, false);
    v = pl_swap_add(v, v, true);
    v += xor_lane<8>(v);
    v += xor_lane<4>(v);
    v += xor_lane<2>(v);
    v += xor_lane<1>(v);
    return v;
}

// sums of v[0..N) over the workgroup, in every thread
template <int N, int WAVES, int NB>
NDT_D void ndt_block_sum(double (&v)[N], NdtBlockSums<WAVES, NB> &red, int &par)
{
    static_assert(N <= NB, "NdtBlockSums::v");
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = ndt_wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) red.v[par][threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        double s = 0.0;
        for (int w = 0; w < WAVES; w++) s += red.v[par][w][k];
        v[k] = s;
    }
    par ^= 1;
}

template <int WAVES, int NB>
NDT_D double ndt_block_sum(double v, NdtBlockSums<WAVES, NB> &red, int &par)
{
    double a[1] = {v};
    ndt_block_sum(a, red, par);
    return a[0];
}

// The largest v over the workgroup, in every thread, OF NON-NEGATIVE VALUES: an fmax xor tree per wave, then the waves folded
// from a seed of 0.0.  fmax drops a NaN operand, so a NaN contributes nothing and all NaN gives 0.0.
template <int WAVES, int NB>
NDT_D double ndt_block_max(double v, NdtBlockSums<WAVES, NB> &red, int &par)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red.v[par][threadIdx.x >> 6][0] = v;
    __syncthreads();
    double m = 0.0;
    for (int w = 0; w < WAVES; w++) m = fmax(m, red.v[par][w][0]);
    par ^= 1;
    return m;
}

// the sum of c over the workgroup, in every thread
template <int WAVES>
NDT_D unsigned ndt_block_count(unsigned c, NdtBlockCounts<WAVES> &cnt, int &par)
{
    const unsigned incl = ndt_wave_incl_scan(c);
    if ((threadIdx.x & 63) == 63) cnt.v[par][threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned n = 0;
    for (int w = 0; w < WAVES; w++) n += cnt.v[par][w];
    par ^= 1;
    return n;
}

// Ordered exclusive scan of c in thread order: the sum of c over the threads below this one; total: over all of them.  The wave
// scan of ndt_block_count, the waves' totals through LDS.  Integer sums: the same result on every run.
template <int WAVES>
NDT_D unsigned ndt_block_scan(unsigned c, NdtBlockCounts<WAVES> &cnt, int &par, unsigned &total)
{
    const unsigned wave = threadIdx.x >> 6;
    const unsigned incl = ndt_wave_incl_scan(c);
    if ((threadIdx.x & 63) == 63) cnt.v[par][wave] = incl;
    __syncthreads();
    unsigned below = 0;
    total = 0;
    for (unsigned w = 0; w < (unsigned)WAVES; w++) {
        const unsigned t = cnt.v[par][w];
        below += w < wave ? t : 0u;
        total += t;
    }
    par ^= 1;
    return below + incl - c;
}

// Ordered compaction: where `keep`, the number of kept threads below this one (the kept threads get 0 .. total - 1 in thread
// order); total: all of them.  A ballot and a population count per wave, the waves' counts through LDS.
template <int WAVES>
NDT_D unsigned ndt_block_rank(bool keep, NdtBlockCounts<WAVES> &cnt, int &par, unsigned &total)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = ndt_ballot(keep);
    if (lane == 0) cnt.v[par][wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned below = 0;
    total = 0;
    for (unsigned w = 0; w < (unsigned)WAVES; w++) {
        const unsigned c = cnt.v[par][w];
        below += w < wave ? c : 0u;
        total += c;
    }
    par ^= 1;
    return below + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}
