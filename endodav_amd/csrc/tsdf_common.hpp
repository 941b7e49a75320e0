// What tsdf.hip, tsdf_mesh.hip and tsdf_raycast.hip share: the tile of the extraction kernels, the index of a voxel, the hop of a cell corner, the
// gradient of a voxel and the checks of an edv_tsdf_volume.
// Everything here is internal to the translation unit that includes it.
#pragma once
#include <cmath>

#include "ops.hpp"

namespace edv {
namespace {

constexpr int TSDF_THREADS = 256, TSDF_WAVES = TSDF_THREADS / WAVE;
constexpr int TSDF_ITERS = 4;
constexpr int TSDF_TILE = TSDF_THREADS * TSDF_ITERS;  // voxels per workgroup of count and extract: the one constant behind tsdf_tile_voxels()

__device__ __forceinline__ void voxel_index(const TsdfVol &v, unsigned a, unsigned &ix, unsigned &iy, unsigned &iz) {
    const unsigned r = a / (unsigned)v.nx;
    ix = a - r * (unsigned)v.nx, iz = r / (unsigned)v.ny, iy = r - iz * (unsigned)v.ny;
}

// the linear hop of offset d = (d & 1, d >> 1 & 1, d >> 2 & 1)
__device__ __forceinline__ unsigned hop_of(const TsdfVol &v, unsigned d) {
    return (d & 1u) + ((d >> 1) & 1u) * (unsigned)v.nx + ((d >> 2) & 1u) * (unsigned)v.nx * (unsigned)v.ny;
}

// g_k = tsdf[i_k -> min(i_k + 1, n_k - 1)] - tsdf[i_k -> max(i_k - 1, 0)]: every index stays in the grid
__device__ __forceinline__ void gradient(const TsdfVol &v, unsigned a, unsigned ix, unsigned iy, unsigned iz, float (&g)[3]) {
    const unsigned hx = 1u, hy = (unsigned)v.nx, hz = (unsigned)v.nx * (unsigned)v.ny;
    g[0] = v.tsdf[ix + 1 < (unsigned)v.nx ? a + hx : a] - v.tsdf[ix > 0 ? a - hx : a];
    g[1] = v.tsdf[iy + 1 < (unsigned)v.ny ? a + hy : a] - v.tsdf[iy > 0 ? a - hy : a];
    g[2] = v.tsdf[iz + 1 < (unsigned)v.nz ? a + hz : a] - v.tsdf[iz > 0 ? a - hz : a];
}

inline long long tiles_of(long long voxels) { return (voxels + TSDF_TILE - 1) / TSDF_TILE; }

inline bool positive(double x) { return std::isfinite(x) && x > 0.0; }

// the dimensions alone: what the workspace sizes refuse with 0
inline bool volume_dims_ok(int nx, int ny, int nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny < (1ll << 31) && (long long)nx * ny * nz < (1ll << 31);
}

// the volume's own fields; `voxels` = nx * ny * nz < 2^31
inline int check_volume(const TsdfVol &v, long long &voxels) {
    EDV_CHECK(v.tsdf && v.weight, "null tsdf or weight");
    EDV_CHECK(aligned_to(v.tsdf, 4) && aligned_to(v.weight, 4) && aligned_to(v.color, 4), "volume arrays not 4-byte aligned");
    EDV_CHECK(v.nx >= 1 && v.ny >= 1 && v.nz >= 1, "nx, ny and nz must be at least 1");
    EDV_CHECK((long long)v.nx * v.ny < (1ll << 31) && (long long)v.nx * v.ny * v.nz < (1ll << 31), "a volume of 2^31 voxels or more");
    EDV_CHECK(positive(v.voxel) && positive(v.trunc) && positive((double)v.max_weight), "voxel, trunc and max_weight must be finite and positive");
    voxels = (long long)v.nx * v.ny * v.nz;
    return 0;
}

}  // namespace
}  // namespace edv
