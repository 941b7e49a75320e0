#pragma clang fp contract(off)
// Surface fusion on the device: a clip of depth [n, h, w] fp32 with its cameras folded into one truncated signed distance (TSDF) volume
// [nz, ny, nx], x fastest, and the zero crossings of that volume written as an ordered, compacted point list.
//   tsdf_integrate  one launch for the whole clip.  One thread owns one voxel (x along the lanes, so the volume accesses coalesce), loads it once,
//                   takes the n frames in order with the voxel in registers, and stores it once, only if some frame updated it.  The depth, mask
//                   and colour gathers are the scattered side: neighbouring voxels in x project to neighbouring pixels.
//   tsdf_count      one workgroup per tile of TSDF_TILE voxels in linear order: the crossings of the tile (up to three a voxel, towards its +x, +y
//                   and +z neighbour), counted by wave ballot and popcount, one 64-bit count per tile in the workspace; then the one-workgroup
//                   exclusive scan of compact_common.hpp, which leaves the total in total[0]
//   tsdf_extract    the same tiles: the predicates again, the rank of every crossing inside its tile (voxel-major, axis-minor), the point in fp64,
//                   and element stores of point g = tile offset + rank when g < capacity
// One thread per voxel and a fixed frame order: no atomics anywhere, no workgroup waits for another, the same input gives the same bits on every
// call.  Every store of the extract is one float or one byte of exactly one point, so no two workgroups ever write the same dword.
// Contraction is off for the whole file and the divisions are IEEE's: every fp32 and fp64 operation is numpy's, in the order written here
// (fusion.TsdfHost is the mirror the kernels are held to, bit for bit).
#include <cmath>

#include "ops.hpp"

#include "cloud_common.hpp"    // depth_value, kept, check_selection: shared with pointcloud.hip
#include "compact_common.hpp"  // wave_count, tile_count_store, exclusive_scan_kernel, tile_ranks: shared with pointcloud.hip and tsdf_mesh.hip
#include "tsdf_common.hpp"     // TSDF_TILE, voxel_index, tiles_of, check_volume: shared with tsdf_mesh.hip

namespace edv {
namespace {

// grid: ceil(voxels / TSDF_THREADS).  cam = W[3][4] (rows 0..2 of inv(T_world_camera)), then K00 K01 K02 K10 K11 K12
template <bool COLOUR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(TsdfVol v, CloudSel s, const double *__restrict__ cams, int cam_stride,
                                                                      const uint8_t *__restrict__ frames, unsigned voxels) {
    const unsigned a = blockIdx.x * (unsigned)TSDF_THREADS + threadIdx.x;
    if (a >= voxels) return;
    unsigned ix, iy, iz;
    voxel_index(v, a, ix, iy, iz);
    const double cx = v.origin[0] + ((double)ix + 0.5) * v.voxel;
    const double cy = v.origin[1] + ((double)iy + 0.5) * v.voxel;
    const double cz = v.origin[2] + ((double)iz + 0.5) * v.voxel;
    float t = v.tsdf[a], wt = v.weight[a], c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (COLOUR) {
        const float *c = v.color + (size_t)a * 3;
        c0 = c[0], c1 = c[1], c2 = c[2];
    }
    const long long hw = (long long)s.h * s.w;
    const double wd = (double)s.w, hd = (double)s.h, behind = -v.trunc;
    bool touched = false;
    for (long long f = 0; f < s.n; ++f) {
        const double *cam = cams + f * cam_stride;
        const double q2 = ((cam[8] * cx + cam[9] * cy) + cam[10] * cz) + cam[11];
        if (!(q2 > 0.0)) continue;  // behind the camera, or NaN
        const double q0 = ((cam[0] * cx + cam[1] * cy) + cam[2] * cz) + cam[3];
        const double q1 = ((cam[4] * cx + cam[5] * cy) + cam[6] * cz) + cam[7];
        const double pu = ((cam[12] * q0 + cam[13] * q1) + cam[14] * q2) / q2;
        const double pv = ((cam[15] * q0 + cam[16] * q1) + cam[17] * q2) / q2;
        if (!(pu >= 0.0 && pu < wd && pv >= 0.0 && pv < hd)) continue;  // in fp64, before any conversion: 0 <= px < w and 0 <= py < h below
        const int px = (int)pu, py = (int)pv;
        const long long p = (long long)py * s.w + px;
        const float x = s.x[f * hw + p];
        const unsigned m = s.mask ? s.mask[f * s.mask_stride + p] : 1u;
        float z;
        if (!kept(s, x, m, z)) continue;
        const double sdf = (double)z - q2;
        if (sdf < behind) continue;  // more than trunc behind the surface: unseen
        const double ratio = sdf / v.trunc;
        const float d = (float)(ratio < 1.0 ? ratio : 1.0);
        const float wn = wt + 1.0f;
        t = (t * wt + d) / wn;
        if (COLOUR) {
            const uint8_t *c = frames + (f * hw + p) * 3;
            c0 = (c0 * wt + (float)c[0]) / wn;
            c1 = (c1 * wt + (float)c[1]) / wn;
            c2 = (c2 * wt + (float)c[2]) / wn;
        }
        wt = wn < v.max_weight ? wn : v.max_weight;
        touched = true;
    }
    if (!touched) return;
    v.tsdf[a] = t, v.weight[a] = wt;
    if (COLOUR) {
        float *c = v.color + (size_t)a * 3;
        c[0] = c0, c[1] = c1, c[2] = c2;
    }
}

// the crossings of voxel a towards its +x, +y, +z neighbour as bits 0..2; ta and tb[k] are the two distances of a pair that crosses.
// A voxel beyond the volume has none, so every lane of a wave reaches the ballots that follow.
__device__ __forceinline__ unsigned crossings(const TsdfVol &v, unsigned a, unsigned voxels, float min_weight, unsigned &ix, unsigned &iy, unsigned &iz,
                                              float &ta, float (&tb)[3]) {
    ix = iy = iz = 0, ta = 0.0f, tb[0] = tb[1] = tb[2] = 0.0f;
    if (a >= voxels) return 0;
    voxel_index(v, a, ix, iy, iz);
    if (!(v.weight[a] >= min_weight)) return 0;
    ta = v.tsdf[a];
    const bool neg = ta < 0.0f;  // 0 and -0 count as outside
    const bool inside[3] = {ix + 1 < (unsigned)v.nx, iy + 1 < (unsigned)v.ny, iz + 1 < (unsigned)v.nz};
    const unsigned hop[3] = {1u, (unsigned)v.nx, (unsigned)v.nx * (unsigned)v.ny};
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!inside[k]) continue;
        const unsigned b = a + hop[k];  // inside the grid, so below voxels
        if (!(v.weight[b] >= min_weight)) continue;
        tb[k] = v.tsdf[b];
        if (neg != (tb[k] < 0.0f)) bits |= 1u << k;
    }
    return bits;
}

// grid: tiles
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_count_kernel(TsdfVol v, float min_weight, unsigned voxels, u64 *__restrict__ counts) {
    unsigned c = 0;
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        unsigned ix, iy, iz;
        float ta, tb[3];
        const unsigned bits = crossings(v, a, voxels, min_weight, ix, iy, iz, ta, tb);
        c += wave_count<2>((unsigned)__popc(bits));
    }
    tile_count_store<TSDF_WAVES, 1>({c}, {counts}, blockIdx.x);
}

// grid: tiles
template <bool COLOUR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_extract_kernel(TsdfVol v, float min_weight, unsigned voxels, const u64 *__restrict__ tile_offsets,
                                                                    float *__restrict__ points, uint8_t *__restrict__ colors, u64 capacity) {
    const u64 tile_base = tile_offsets[blockIdx.x];
    if (tile_base >= capacity) return;  // uniform over the workgroup: a tile that starts behind the capacity has nothing to write
    unsigned ix[TSDF_ITERS], iy[TSDF_ITERS], iz[TSDF_ITERS], bits[TSDF_ITERS], c[TSDF_ITERS], rank[TSDF_ITERS];
    float ta[TSDF_ITERS], tb[TSDF_ITERS][3];
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        bits[it] = crossings(v, a, voxels, min_weight, ix[it], iy[it], iz[it], ta[it], tb[it]);
        c[it] = (unsigned)__popc(bits[it]);
    }
    // the rank of the voxel's first crossing: all three axes of an earlier voxel come first
    if (tile_ranks<TSDF_ITERS, TSDF_WAVES, 2>(c, rank) == 0) return;
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        if (!bits[it]) continue;
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        u64 g = tile_base + rank[it];
        const double ctr[3] = {(double)ix[it] + 0.5, (double)iy[it] + 0.5, (double)iz[it] + 0.5};
        const unsigned hop[3] = {1u, (unsigned)v.nx, (unsigned)v.nx * (unsigned)v.ny};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!((bits[it] >> k) & 1u)) continue;
            if (g < capacity) {
                const float t = ta[it] / (ta[it] - tb[it][k]);  // the signs differ, so the divisor is never zero
                float *o = points + g * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = (float)(v.origin[j] + (j == k ? ctr[j] + (double)t : ctr[j]) * v.voxel);
                if (COLOUR) {
                    const float *ca = v.color + (size_t)a * 3, *cb = v.color + (size_t)(a + hop[k]) * 3;
                    uint8_t *oc = colors + g * 3;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float c = ca[j] + t * (cb[j] - ca[j]);
                        oc[j] = (uint8_t)fminf(255.0f, fmaxf(0.0f, floorf(c + 0.5f)));
                    }
                }
            }
            ++g;
        }
    }
}

inline int check_workspace(const TsdfVol &v, const void *ws, size_t ws_bytes) {
    EDV_CHECK(ws && aligned_to(ws, 8) && ws_bytes >= tsdf_workspace(v.nx, v.ny, v.nz), "workspace missing, too small or not 8-byte aligned (edv_tsdf_workspace)");
    return 0;
}

}  // namespace

int tsdf_tile_voxels() { return TSDF_TILE; }

size_t tsdf_workspace(int nx, int ny, int nz) {
    if (!volume_dims_ok(nx, ny, nz)) return 0;
    return (size_t)tiles_of((long long)nx * ny * nz) * sizeof(u64);
}

int tsdf_integrate(const TsdfVol &v, const CloudSel &s, const double *cams, int cam_stride, const uint8_t *frames, hipStream_t stream) {
    long long voxels = 0;
    EDV_TRY(check_volume(v, voxels));
    EDV_TRY(check_selection(s));
    EDV_CHECK(s.step == 1, "step must be 1: every voxel samples the full-resolution clip");
    EDV_CHECK(cams && aligned_to(cams, 8), "cameras missing or not 8-byte aligned");
    EDV_CHECK(cam_stride == 0 || cam_stride == 18, "cam_stride: 0 (one camera for all frames) or 18 (a camera per frame)");
    EDV_CHECK((v.color != nullptr) == (frames != nullptr), "a coloured volume takes frames and an uncoloured one takes none");
    const dim3 grid((unsigned)((voxels + TSDF_THREADS - 1) / TSDF_THREADS));
    if (v.color)
        EDV_LAUNCH(tsdf_integrate_kernel<true>, grid, dim3(TSDF_THREADS), 0, stream, v, s, cams, cam_stride, frames, (unsigned)voxels);
    else
        EDV_LAUNCH(tsdf_integrate_kernel<false>, grid, dim3(TSDF_THREADS), 0, stream, v, s, cams, cam_stride, frames, (unsigned)voxels);
    EDV_LAUNCH_OK();
    return 0;
}

int tsdf_count(const TsdfVol &v, float min_weight, long long *total, void *ws, size_t ws_bytes, hipStream_t stream) {
    long long voxels = 0;
    EDV_TRY(check_volume(v, voxels));
    EDV_CHECK(total && aligned_to(total, 8), "total missing or not 8-byte aligned");
    EDV_TRY(check_workspace(v, ws, ws_bytes));
    const long long tiles = tiles_of(voxels);
    u64 *counts = static_cast<u64 *>(ws);
    EDV_LAUNCH(tsdf_count_kernel, dim3((unsigned)tiles), dim3(TSDF_THREADS), 0, stream, v, min_weight, (unsigned)voxels, counts);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, counts, tiles, 0ll, total, 0ll);
    EDV_LAUNCH_OK();
    return 0;
}

int tsdf_extract(const TsdfVol &v, float min_weight, const void *ws, size_t ws_bytes, float *points, uint8_t *colors, long long capacity, hipStream_t stream) {
    long long voxels = 0;
    EDV_TRY(check_volume(v, voxels));
    EDV_TRY(check_workspace(v, ws, ws_bytes));
    EDV_CHECK(capacity >= 0, "negative capacity");
    EDV_CHECK(points && aligned_to(points, 4), "points missing or not 4-byte aligned");
    EDV_CHECK(!colors || v.color, "colours asked of a volume that has none");
    if (capacity == 0) return 0;
    const dim3 grid((unsigned)tiles_of(voxels));
    const u64 *tile_offsets = static_cast<const u64 *>(ws);
    if (v.color && colors)
        EDV_LAUNCH(tsdf_extract_kernel<true>, grid, dim3(TSDF_THREADS), 0, stream, v, min_weight, (unsigned)voxels, tile_offsets, points, colors, (u64)capacity);
    else
        EDV_LAUNCH(tsdf_extract_kernel<false>, grid, dim3(TSDF_THREADS), 0, stream, v, min_weight, (unsigned)voxels, tile_offsets, points, colors, (u64)capacity);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace edv
