// Point clouds on the device: a clip of depth [n, h, w] fp32 lifted to world-space points with the frames' colours, masked, subsampled and
// compacted in order (get_point_cloud of the loaders in tools/viser-rgbd/utils and visualize_reconstruction.py in the reference, float64 numpy there).
// An order-preserving stream compaction with the geometry fused in, three launches in two calls:
//   cloud_count    one workgroup per tile of CLOUD_TILE output pixels of one frame (the frame is blockIdx.y): the kept pixels of the tile, counted
//                  by wave ballot and popcount, one 64-bit count per tile in the workspace
//                  one workgroup: exclusive 64-bit scan of the counts over all tiles in frame-major order, in place; offsets[f] = the points of
//                  the frames before f, offsets[n] = the total
//   cloud_scatter  the same tiles: the predicate again, the rank of every kept pixel inside its tile (compact_common.hpp's tile_ranks), the
//                  point in fp64, and element stores of point g = tile offset + rank when g < capacity
// No workgroup waits for another inside a launch and there are no atomics at all: the same input gives the same bits on every call.  The output
// of a tile starts at an arbitrary 12-byte (points) or 1-byte (colours) boundary; every store is one float or one byte of exactly one point, so
// no two workgroups ever write the same dword.
// Contraction is off for the whole file and the division is IEEE's: every fp32 and fp64 operation is numpy's, in the order written here.
#include <algorithm>

#include "ops.hpp"

#pragma clang fp contract(off)

#include "cloud_common.hpp"    // depth_value, kept, check_selection: shared with tsdf.hip
#include "compact_common.hpp"  // wave_count, tile_count_store, exclusive_scan_kernel, tile_ranks: shared with tsdf.hip and tsdf_mesh.hip

namespace edv {
namespace {

constexpr int CLOUD_THREADS = 256, CLOUD_WAVES = CLOUD_THREADS / WAVE;
constexpr int CLOUD_ITERS = 8;
constexpr int CLOUD_TILE = CLOUD_THREADS * CLOUD_ITERS;  // output pixels per workgroup: the one constant behind cloud_tile_pixels()

// grid (tiles per frame, frames).  UNIT: step == 1, where the source pixel is the output pixel
template <bool UNIT>
__global__ __launch_bounds__(CLOUD_THREADS) void cloud_count_kernel(CloudSel s, int ow, unsigned grid_pixels, u64 *__restrict__ counts) {
    const long long f = blockIdx.y;
    const float *xf = s.x + f * s.h * s.w;
    const uint8_t *mf = s.mask ? s.mask + f * s.mask_stride : nullptr;
    // all loads of the tile first, so that they are in flight together
    float x[CLOUD_ITERS];
    unsigned m[CLOUD_ITERS];
#pragma unroll
    for (int it = 0; it < CLOUD_ITERS; ++it) {
        const unsigned q = blockIdx.x * (unsigned)CLOUD_TILE + it * CLOUD_THREADS + threadIdx.x;
        x[it] = 0.0f, m[it] = 0;
        if (q < grid_pixels) {
            int ox, oy;
            const int p = UNIT ? (int)q : source_pixel(s, ow, q, ox, oy);
            x[it] = xf[p], m[it] = mf ? mf[p] : 1u;
        }
    }
    unsigned c = 0;
#pragma unroll
    for (int it = 0; it < CLOUD_ITERS; ++it) {
        float z;
        c += wave_count<1>(kept(s, x[it], m[it], z));
    }
    tile_count_store<CLOUD_WAVES, 1>({c}, {counts}, f * gridDim.x + blockIdx.x);
}

// grid (tiles per frame, frames)
__global__ __launch_bounds__(CLOUD_THREADS) void cloud_scatter_kernel(CloudSel s, int ow, unsigned grid_pixels, const double *__restrict__ cams, int cam_stride,
                                                                      const uint8_t *__restrict__ frames, const long long *__restrict__ offsets,
                                                                      const u64 *__restrict__ tile_offsets, float *__restrict__ points,
                                                                      uint8_t *__restrict__ colors, u64 capacity) {
    const long long f = blockIdx.y;
    const u64 tile_base = tile_offsets[f * gridDim.x + blockIdx.x];
    // uniform over the workgroup: a frame without points, or a tile that starts behind the capacity, has nothing to write
    if (offsets[f + 1] == offsets[f] || tile_base >= capacity) return;
    const float *xf = s.x + f * s.h * s.w;
    const uint8_t *mf = s.mask ? s.mask + f * s.mask_stride : nullptr;
    float z[CLOUD_ITERS];
    unsigned m[CLOUD_ITERS], keep[CLOUD_ITERS], rank[CLOUD_ITERS];
    int p[CLOUD_ITERS], ox[CLOUD_ITERS], oy[CLOUD_ITERS];
#pragma unroll
    for (int it = 0; it < CLOUD_ITERS; ++it) {  // all loads of the tile first, so that they are in flight together
        const unsigned q = blockIdx.x * (unsigned)CLOUD_TILE + it * CLOUD_THREADS + threadIdx.x;
        z[it] = 0.0f, m[it] = 0, p[it] = 0, ox[it] = 0, oy[it] = 0;
        if (q < grid_pixels) {
            p[it] = source_pixel(s, ow, q, ox[it], oy[it]);
            z[it] = xf[p[it]], m[it] = mf ? mf[p[it]] : 1u;
        }
    }
#pragma unroll
    for (int it = 0; it < CLOUD_ITERS; ++it) keep[it] = kept(s, z[it], m[it], z[it]);
    if (tile_ranks<CLOUD_ITERS, CLOUD_WAVES, 1>(keep, rank) == 0) return;
    const double *cam = cams + f * cam_stride;
    double Kinv[9], R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Kinv[i] = cam[i], R[i] = cam[9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = cam[18 + i];
    const bool colour = frames && colors;
    const uint8_t *ff = colour ? frames + f * s.h * s.w * 3 : nullptr;
#pragma unroll
    for (int it = 0; it < CLOUD_ITERS; ++it) {
        if (!keep[it]) continue;
        const u64 g = tile_base + rank[it];
        if (g >= capacity) continue;
        const double u = ((double)ox[it] + 0.5) * (double)s.step, v = ((double)oy[it] + 0.5) * (double)s.step;
        double l[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) l[i] = (Kinv[3 * i] * u + Kinv[3 * i + 1] * v) + Kinv[3 * i + 2];
        const double zd = (double)z[it];
        float *o = points + g * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double r = (R[3 * i] * l[0] + R[3 * i + 1] * l[1]) + R[3 * i + 2] * l[2];
            o[i] = (float)(t[i] + r * zd);
        }
        if (colour) {
            const uint8_t *c = ff + (long long)p[it] * 3;
            uint8_t *oc = colors + g * 3;
            oc[0] = c[0], oc[1] = c[1], oc[2] = c[2];
        }
    }
}

struct CloudGrid {
    int ow;
    unsigned pixels;  // oh * ow <= h * w < 2^31
    long long tiles_per_frame;
};

inline CloudGrid cloud_grid(int h, int w, int step) {
    const long long oh = ((long long)h + step - 1) / step, ow = ((long long)w + step - 1) / step;
    return {(int)ow, (unsigned)(oh * ow), (oh * ow + CLOUD_TILE - 1) / CLOUD_TILE};
}

inline int check_workspace(const CloudSel &s, const void *ws, size_t ws_bytes) {
    EDV_CHECK(ws && aligned_to(ws, 8) && ws_bytes >= cloud_workspace(s.n, s.h, s.w, s.step), "workspace missing, too small or not 8-byte aligned (edv_cloud_workspace)");
    return 0;
}

}  // namespace

int cloud_tile_pixels() { return CLOUD_TILE; }

size_t cloud_workspace(long long n, int h, int w, int step) {
    if (n < 1 || n > 65535 || h < 1 || w < 1 || step < 1 || (long long)h * w >= (1ll << 31)) return 0;
    return (size_t)(n * cloud_grid(h, w, step).tiles_per_frame) * sizeof(u64);
}

int cloud_count(const CloudSel &s, long long *offsets, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_TRY(check_selection(s));
    EDV_CHECK(offsets && aligned_to(offsets, 8), "offsets missing or not 8-byte aligned");
    EDV_TRY(check_workspace(s, ws, ws_bytes));
    const CloudGrid g = cloud_grid(s.h, s.w, s.step);
    const dim3 grid((unsigned)g.tiles_per_frame, (unsigned)s.n);
    u64 *counts = static_cast<u64 *>(ws);
    if (s.step == 1)
        EDV_LAUNCH(cloud_count_kernel<true>, grid, dim3(CLOUD_THREADS), 0, stream, s, g.ow, g.pixels, counts);
    else
        EDV_LAUNCH(cloud_count_kernel<false>, grid, dim3(CLOUD_THREADS), 0, stream, s, g.ow, g.pixels, counts);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, counts, s.n * g.tiles_per_frame, g.tiles_per_frame, offsets, s.n);
    EDV_LAUNCH_OK();
    return 0;
}

int cloud_scatter(const CloudSel &s, const double *cams, int cam_stride, const uint8_t *frames, const long long *offsets, const void *ws, size_t ws_bytes,
                  float *points, uint8_t *colors, long long capacity, hipStream_t stream) {
    EDV_TRY(check_selection(s));
    EDV_CHECK(cams && aligned_to(cams, 8), "cameras missing or not 8-byte aligned");
    EDV_CHECK(cam_stride == 0 || cam_stride == 21, "cam_stride: 0 (one camera for all frames) or 21 (a camera per frame)");
    EDV_CHECK(offsets && aligned_to(offsets, 8), "offsets missing or not 8-byte aligned");
    EDV_TRY(check_workspace(s, ws, ws_bytes));
    EDV_CHECK(capacity >= 0, "negative capacity");
    EDV_CHECK(points && aligned_to(points, 4), "points missing or not 4-byte aligned");
    if (capacity == 0) return 0;
    const CloudGrid g = cloud_grid(s.h, s.w, s.step);
    EDV_LAUNCH(cloud_scatter_kernel, dim3((unsigned)g.tiles_per_frame, (unsigned)s.n), dim3(CLOUD_THREADS), 0, stream, s, g.ow, g.pixels, cams, cam_stride, frames,
               offsets, static_cast<const u64 *>(ws), points, colors, (u64)capacity);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace edv
