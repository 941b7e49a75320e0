// What the order-preserving compactions of pointcloud.hip, tsdf.hip and tsdf_mesh.hip share.  A compaction is three steps over tiles of
// ITERS * WAVES * 64 items, one workgroup a tile: the count of every tile (wave_count, tile_count_store), the one-workgroup exclusive scan of
// the counts (exclusive_scan_kernel), and the rank of every item inside its tile (tile_ranks), so that item g = tile offset + rank.
// THE ORDER: item `it * (WAVES * 64) + threadIdx.x` of a tile belongs to iteration `it` of thread threadIdx.x, so the items of a tile are ordered
// by iteration, then wave, then lane.  Counting is by wave ballot and popcount over the bit planes of the per-lane counts; there are no
// atomics and no workgroup waits for another.  Everything here is internal to the translation unit that includes it.
#pragma once
#include "ops.hpp"

namespace edv {
namespace {

using u64 = unsigned long long;

constexpr int SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / WAVE, SCAN_ITEMS = 4;

// the sum over the wave of per-lane counts below 2^PLANES; every lane of the wave calls it
template <int PLANES>
__device__ __forceinline__ unsigned wave_count(unsigned c) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < PLANES; ++k) s += (unsigned)__popcll(__ballot((c >> k) & 1u)) << k;
    return s;
}

// The count epilogue.  c[q] is this wave's sum of count q, the same in every lane (sums of wave_count): per-wave sums in LDS, one barrier, and
// thread q adds them in wave order into dst[q][tile].  Every thread of the workgroup calls it.
template <int WAVES, int N>
__device__ __forceinline__ void tile_count_store(const unsigned (&c)[N], u64 *const (&dst)[N], long long tile) {
    __shared__ unsigned red[N][WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) red[q][wave] = c[q];
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += red[threadIdx.x][w];
        dst[threadIdx.x][tile] = t;
    }
}

// rank[it]: the sum of the counts (below 2^PLANES each) of the items of the tile before this thread's item of iteration `it`, in THE ORDER.
// Returns the tile's sum.  Every thread of the workgroup calls it.
template <int ITERS, int WAVES, int PLANES>
__device__ __forceinline__ unsigned tile_ranks(const unsigned (&c)[ITERS], unsigned (&rank)[ITERS]) {
    __shared__ unsigned cnt[ITERS][WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        unsigned in_wave = 0;
        rank[it] = 0;
#pragma unroll
        for (int k = 0; k < PLANES; ++k) {
            const u64 ballot = __ballot((c[it] >> k) & 1u);
            in_wave += (unsigned)__popcll(ballot) << k;
            rank[it] += (unsigned)__popcll(ballot & below) << k;
        }
        if (lane == 0) cnt[it][wave] = in_wave;
    }
    __syncthreads();
    unsigned run = 0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w == wave) rank[it] += run;
            run += cnt[it][w];
        }
    }
    return run;
}

// one workgroup: ws[i] = sum of ws[0 .. i) for the `tiles` counts, offsets[n] = the total; with tiles_per_frame > 0 also
// offsets[f] = ws[f * tiles_per_frame] after the scan (tiles_per_frame == 0, n == 0: the total alone, in offsets[0]).
// A round takes SCAN_THREADS * SCAN_ITEMS counts; the total of the rounds before is carried into the next.
__global__ __launch_bounds__(SCAN_THREADS) void exclusive_scan_kernel(u64 *__restrict__ ws, long long tiles, long long tiles_per_frame, long long *__restrict__ offsets,
                                                                      long long n) {
    __shared__ u64 wave_sum_s[SCAN_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    u64 carry = 0;
    for (long long base = 0; base < tiles; base += (long long)SCAN_THREADS * SCAN_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * SCAN_ITEMS;
        u64 v[SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            v[j] = i0 + j < tiles ? ws[i0 + j] : 0;
            mine += v[j];
        }
        u64 inc = mine;  // inclusive over the lanes of the wave
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const u64 up = __shfl_up(inc, o, WAVE);
            if (lane >= o) inc += up;
        }
        if (lane == WAVE - 1) wave_sum_s[wave] = inc;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < SCAN_WAVES; ++k) {
            const u64 t = wave_sum_s[k];
            before += k < wave ? t : 0;
            total += t;
        }
        u64 ex = carry + before + (inc - mine);
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            const long long i = i0 + j;
            if (i < tiles) {
                ws[i] = ex;
                if (tiles_per_frame > 0 && i % tiles_per_frame == 0) offsets[i / tiles_per_frame] = (long long)ex;
                ex += v[j];
            }
        }
        carry += total;
        __syncthreads();  // wave_sum_s is rewritten by the next round
    }
    if (threadIdx.x == 0) offsets[n] = (long long)carry;
}

}  // namespace
}  // namespace edv
