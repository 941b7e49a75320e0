#pragma clang fp contract(off)
// Triangle meshes from the TSDF volume of tsdf.hip: marching tetrahedra on the Kuhn split of every cell (six tetrahedra around the body
// diagonal, the same in every cell, so neighbouring cells agree on the diagonals of their shared faces: no ambiguous case, a watertight and
// consistently oriented mesh).  The rule is stated once, in include/endodav_hip.h; fusion.TsdfHost.mesh is the mirror, bit for bit.
//   mesh_flags     one thread per voxel: one byte with OBSERVED (weight >= min_weight), INSIDE (tsdf < 0) and VALID (the cell of the voxel exists
//                  and its eight corners are observed)
//   mesh_count     one workgroup per tile of TSDF_TILE voxels, from the flags alone: the 7-bit mask of the edges a -> a + off(d) that carry a
//                  vertex (one byte per voxel) and the triangles of the voxel's cell; two 64-bit counts per tile, summed by wave ballot and
//                  popcount over the bit planes of the per-voxel counts.  Then the one-workgroup scan of compact_common.hpp, once per count array
//   mesh_base      the same tiles: the rank of every voxel's first vertex inside its tile, and base[a] = tile offset + rank (u32 per voxel)
//   mesh_vertex    one thread per voxel that owns vertices: position (fp64), normal and colour (fp32) of vertex base[a] + its rank in the mask
//   mesh_triangle  the same tiles: the corner pattern of every valid cell again, the rank of its first triangle inside the tile, and per
//                  triangle three indices base[u] + popcount(mask[u] & bits below d) looked up through the 6 x 16 table
// The first four launches are edv_tsdf_mesh_count and fill the workspace; the last two are edv_tsdf_mesh_extract and only read it.
// One thread per voxel with x along the lanes, no atomics, no workgroup waits for another: the passes are launches on one stream.  Every store
// to an output is one float, one byte or one int of exactly one vertex or triangle, guarded by its capacity.  Contraction is off for the whole
// file, the divisions and the square root are IEEE's (hipcc's default lowering of fp32 / and sqrtf is correctly rounded; no fast-math flag).
#include <cmath>

#include "ops.hpp"

#include "compact_common.hpp"  // wave_count, tile_count_store, exclusive_scan_kernel, tile_ranks: shared with pointcloud.hip and tsdf.hip
#include "tsdf_common.hpp"     // TSDF_TILE, voxel_index, hop_of, gradient, tiles_of, check_volume

namespace edv {
namespace {

constexpr unsigned OBSERVED = 1u, INSIDE = 2u, VALID = 4u;

// corner i of tetrahedron ti: (0, 1 << p, (1 << p) | (1 << q), 7) for the ti-th permutation (p, q, r) of (0, 1, 2) in lexicographic order
__host__ __device__ constexpr int tet_corner(int ti, int i) {
    const int p = ti / 2, q = (ti % 2 == 0) ? (p == 0 ? 1 : 0) : (p == 2 ? 1 : 2);
    return i == 0 ? 0 : i == 1 ? (1 << p) : i == 2 ? ((1 << p) | (1 << q)) : 7;
}

// edge[ti][m]: the triangles of tetrahedron ti under case mask m (bit i: corner i inside), three edges each, an edge as (d << 3) | u with u
// the cube corner that owns it and d = v - u its direction.  popcount(m) = 1, 2, 3 gives 1, 2, 1 triangles.
struct MeshTable {
    uint8_t edge[6][16][6];
};

// derived from the rule, in integers: the polygon's points are twice the edge midpoints of the unit cube, and the direction from the inside
// to the outside corners is scaled by both counts
constexpr MeshTable make_mesh_table() {
    MeshTable t{};
    for (int ti = 0; ti < 6; ++ti) {
        for (int m = 1; m < 15; ++m) {
            int ins[4] = {}, outs[4] = {}, ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) {
                if ((m >> i) & 1) ins[ni++] = i;
                else outs[no++] = i;
            }
            int poly[4][2] = {}, np = 0;
            if (ni == 1) {
                for (int o = 0; o < 3; ++o) poly[np][0] = ins[0], poly[np][1] = outs[o], ++np;
            } else if (ni == 3) {
                for (int i = 0; i < 3; ++i) poly[np][0] = ins[i], poly[np][1] = outs[0], ++np;
            } else {
                const int quad[4][2] = {{ins[0], outs[0]}, {ins[0], outs[1]}, {ins[1], outs[1]}, {ins[1], outs[0]}};
                for (int k = 0; k < 4; ++k) poly[np][0] = quad[k][0], poly[np][1] = quad[k][1], ++np;
            }
            int P[3][3] = {}, dir[3] = {};
            for (int j = 0; j < 3; ++j) {
                for (int k = 0; k < 3; ++k) P[k][j] = ((tet_corner(ti, poly[k][0]) >> j) & 1) + ((tet_corner(ti, poly[k][1]) >> j) & 1);
                for (int o = 0; o < no; ++o) dir[j] += ni * ((tet_corner(ti, outs[o]) >> j) & 1);
                for (int i = 0; i < ni; ++i) dir[j] -= no * ((tet_corner(ti, ins[i]) >> j) & 1);
            }
            const int e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
            const int dot = (e1[1] * e2[2] - e1[2] * e2[1]) * dir[0] + (e1[2] * e2[0] - e1[0] * e2[2]) * dir[1] + (e1[0] * e2[1] - e1[1] * e2[0]) * dir[2];
            if (dot < 0) {
                for (int k = 0; k < np / 2; ++k) {
                    for (int e = 0; e < 2; ++e) {
                        const int s = poly[k][e];
                        poly[k][e] = poly[np - 1 - k][e], poly[np - 1 - k][e] = s;
                    }
                }
            }
            const int order[6] = {0, 1, 2, 0, 2, 3};
            for (int k = 0; k < (np == 4 ? 6 : 3); ++k) {
                const int ci = tet_corner(ti, poly[order[k]][0]), cj = tet_corner(ti, poly[order[k]][1]);
                const int u = ci < cj ? ci : cj, w = ci < cj ? cj : ci;
                t.edge[ti][m][k] = (uint8_t)(((w - u) << 3) | u);
            }
        }
    }
    return t;
}

__constant__ MeshTable MESH_TABLE = make_mesh_table();

// the case mask of tetrahedron ti under the cell's corner pattern (bit c: corner c inside)
__device__ __forceinline__ unsigned tet_case(unsigned pattern, int ti) {
    return (pattern & 1u) | (((pattern >> tet_corner(ti, 1)) & 1u) << 1) | (((pattern >> tet_corner(ti, 2)) & 1u) << 2) | (((pattern >> 7) & 1u) << 3);
}

__device__ __forceinline__ unsigned triangles_of_case(unsigned m) {
    const unsigned inside = (unsigned)__popc(m);
    return inside <= 2 ? inside : 4 - inside;
}

// grid: ceil(voxels / TSDF_THREADS)
__global__ __launch_bounds__(TSDF_THREADS) void mesh_flags_kernel(TsdfVol v, float min_weight, unsigned voxels, uint8_t *__restrict__ flags) {
    const unsigned a = blockIdx.x * (unsigned)TSDF_THREADS + threadIdx.x;
    if (a >= voxels) return;
    unsigned ix, iy, iz;
    voxel_index(v, a, ix, iy, iz);
    unsigned f = (v.weight[a] >= min_weight ? OBSERVED : 0u) | (v.tsdf[a] < 0.0f ? INSIDE : 0u);  // 0 and -0 count as outside
    if ((f & OBSERVED) && ix + 1 < (unsigned)v.nx && iy + 1 < (unsigned)v.ny && iz + 1 < (unsigned)v.nz) {
        bool all = true;
#pragma unroll
        for (unsigned c = 1; c < 8; ++c) all = all && v.weight[a + hop_of(v, c)] >= min_weight;  // the cell exists: all eight corners are in the grid
        if (all) f |= VALID;
    }
    flags[a] = (uint8_t)f;
}

// bit d - 1: the edge a -> a + off(d) carries a vertex.  A valid cell a - off(s) with s & d == 0 contains the edge, so b = a + off(d) is its
// corner s | d: inside the grid and observed, and only such b are read.
__device__ __forceinline__ unsigned vertex_mask(const TsdfVol &v, const uint8_t *__restrict__ flags, unsigned a, unsigned ix, unsigned iy, unsigned iz) {
    const unsigned fa = flags[a];
    if (!(fa & OBSERVED)) return 0;
    unsigned cells = 0;  // bit s: the cell of voxel a - off(s) lies in the grid and is valid
#pragma unroll
    for (unsigned s = 0; s < 8; ++s) {
        if (ix >= (s & 1u) && iy >= ((s >> 1) & 1u) && iz >= ((s >> 2) & 1u) && (flags[a - hop_of(v, s)] & VALID)) cells |= 1u << s;
    }
    if (!cells) return 0;
    unsigned mask = 0;
#pragma unroll
    for (unsigned d = 1; d < 8; ++d) {
        unsigned with = 0;  // the cells s with s & d == 0
#pragma unroll
        for (unsigned s = 0; s < 8; ++s) with |= (s & d) ? 0u : 1u << s;
        if ((cells & with) && ((fa ^ flags[a + hop_of(v, d)]) & INSIDE)) mask |= 1u << (d - 1);
    }
    return mask;
}

// the corner pattern of the valid cell of voxel a: bit c set when corner c is inside
__device__ __forceinline__ unsigned cell_pattern(const TsdfVol &v, const uint8_t *__restrict__ flags, unsigned a) {
    unsigned pattern = 0;
#pragma unroll
    for (unsigned c = 0; c < 8; ++c) pattern |= (flags[a + hop_of(v, c)] & INSIDE) ? 1u << c : 0u;
    return pattern;
}

__device__ __forceinline__ unsigned triangles_of_cell(unsigned pattern) {
    unsigned n = 0;
#pragma unroll
    for (int ti = 0; ti < 6; ++ti) n += triangles_of_case(tet_case(pattern, ti));
    return n;  // at most 12
}

// grid: tiles
__global__ __launch_bounds__(TSDF_THREADS) void mesh_count_kernel(TsdfVol v, unsigned voxels, const uint8_t *__restrict__ flags, uint8_t *__restrict__ mask,
                                                                  u64 *__restrict__ vertex_counts, u64 *__restrict__ triangle_counts) {
    unsigned nv = 0, nt = 0;
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        unsigned vm = 0, tc = 0;
        if (a < voxels) {
            unsigned ix, iy, iz;
            voxel_index(v, a, ix, iy, iz);
            vm = vertex_mask(v, flags, a, ix, iy, iz);
            mask[a] = (uint8_t)vm;
            if (flags[a] & VALID) tc = triangles_of_cell(cell_pattern(v, flags, a));
        }
        nv += wave_count<4>((unsigned)__popc(vm));  // at most 7
        nt += wave_count<4>(tc);                    // at most 12
    }
    tile_count_store<TSDF_WAVES, 2>({nv, nt}, {vertex_counts, triangle_counts}, blockIdx.x);
}

// grid: tiles
__global__ __launch_bounds__(TSDF_THREADS) void mesh_base_kernel(unsigned voxels, const uint8_t *__restrict__ mask, const u64 *__restrict__ vertex_offsets,
                                                                 unsigned *__restrict__ base) {
    unsigned c[TSDF_ITERS], rank[TSDF_ITERS];
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        c[it] = a < voxels ? (unsigned)__popc((unsigned)mask[a]) : 0u;
    }
    tile_ranks<TSDF_ITERS, TSDF_WAVES, 4>(c, rank);
    const u64 tile_base = vertex_offsets[blockIdx.x];
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        if (a < voxels) base[a] = (unsigned)(tile_base + rank[it]);
    }
}

// grid: ceil(voxels / TSDF_THREADS).  normals and colors may be null
__global__ __launch_bounds__(TSDF_THREADS) void mesh_vertex_kernel(TsdfVol v, unsigned voxels, const uint8_t *__restrict__ mask, const unsigned *__restrict__ base,
                                                                   float *__restrict__ vertices, float *__restrict__ normals, uint8_t *__restrict__ colors,
                                                                   u64 capacity) {
    const unsigned a = blockIdx.x * (unsigned)TSDF_THREADS + threadIdx.x;
    if (a >= voxels) return;
    const unsigned m = mask[a];
    if (!m) return;
    u64 g = base[a];
    if (g >= capacity) return;
    unsigned ix, iy, iz;
    voxel_index(v, a, ix, iy, iz);
    const float ta = v.tsdf[a];
    const double ctr[3] = {(double)ix + 0.5, (double)iy + 0.5, (double)iz + 0.5};
    float ga[3] = {};
    if (normals) gradient(v, a, ix, iy, iz, ga);
    for (unsigned d = 1; d < 8; ++d) {
        if (!((m >> (d - 1)) & 1u)) continue;
        if (g < capacity) {
            const unsigned b = a + hop_of(v, d);  // the mask bit says that b is inside the grid
            const float t = ta / (ta - v.tsdf[b]);  // the signs differ, so the divisor is never zero
            float *o = vertices + g * 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = (float)(v.origin[j] + (((d >> j) & 1u) ? ctr[j] + (double)t : ctr[j]) * v.voxel);
            if (normals) {
                float gb[3], n[3];
                gradient(v, b, ix + (d & 1u), iy + ((d >> 1) & 1u), iz + ((d >> 2) & 1u), gb);
#pragma unroll
                for (int j = 0; j < 3; ++j) n[j] = ga[j] + t * (gb[j] - ga[j]);
                const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                float *on = normals + g * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) on[j] = len > 0.0f ? n[j] / len : 0.0f;
            }
            if (colors) {
                const float *ca = v.color + (size_t)a * 3, *cb = v.color + (size_t)b * 3;
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

// grid: tiles
__global__ __launch_bounds__(TSDF_THREADS) void mesh_triangle_kernel(TsdfVol v, unsigned voxels, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ mask,
                                                                     const unsigned *__restrict__ base, const u64 *__restrict__ triangle_offsets,
                                                                     int *__restrict__ triangles, u64 capacity) {
    const u64 tile_base = triangle_offsets[blockIdx.x];
    if (tile_base >= capacity) return;  // uniform over the workgroup: a tile that starts behind the capacity has nothing to write
    unsigned pattern[TSDF_ITERS], c[TSDF_ITERS], rank[TSDF_ITERS];
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        pattern[it] = c[it] = 0;
        if (a < voxels && (flags[a] & VALID)) {
            pattern[it] = cell_pattern(v, flags, a);
            c[it] = triangles_of_cell(pattern[it]);
        }
    }
    if (tile_ranks<TSDF_ITERS, TSDF_WAVES, 4>(c, rank) == 0) return;
#pragma unroll
    for (int it = 0; it < TSDF_ITERS; ++it) {
        if (!c[it]) continue;
        const unsigned a = blockIdx.x * (unsigned)TSDF_TILE + it * TSDF_THREADS + threadIdx.x;
        u64 g = tile_base + rank[it];
#pragma unroll
        for (int ti = 0; ti < 6; ++ti) {
            const unsigned m = tet_case(pattern[it], ti), n = triangles_of_case(m);
            for (unsigned j = 0; j < n; ++j) {
                if (g < capacity) {
                    int *o = triangles + g * 3;
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const unsigned code = MESH_TABLE.edge[ti][m][3 * j + e], u = code & 7u, d = code >> 3;
                        const unsigned w = a + hop_of(v, u);  // a corner of a cell that exists
                        o[e] = (int)(base[w] + (unsigned)__popc((unsigned)mask[w] & ((1u << (d - 1)) - 1u)));
                    }
                }
                ++g;
            }
        }
    }
}

// the workspace: two 64-bit counts per tile (offsets after the scans), then per voxel the u32 base, the flags byte and the mask byte
struct MeshWorkspace {
    u64 *vertex_tiles, *triangle_tiles;
    unsigned *base;
    uint8_t *flags, *mask;
};

inline MeshWorkspace mesh_workspace_of(const void *ws, long long voxels) {
    const long long tiles = tiles_of(voxels);
    MeshWorkspace m;
    m.vertex_tiles = static_cast<u64 *>(const_cast<void *>(ws));
    m.triangle_tiles = m.vertex_tiles + tiles;
    m.base = reinterpret_cast<unsigned *>(m.triangle_tiles + tiles);
    m.flags = reinterpret_cast<uint8_t *>(m.base + voxels);
    m.mask = m.flags + voxels;
    return m;
}

inline int check_mesh_workspace(const TsdfVol &v, const void *ws, size_t ws_bytes) {
    EDV_CHECK(ws && aligned_to(ws, 8) && ws_bytes >= tsdf_mesh_workspace(v.nx, v.ny, v.nz),
              "workspace missing, too small or not 8-byte aligned (edv_tsdf_mesh_workspace)");
    return 0;
}

}  // namespace

size_t tsdf_mesh_workspace(int nx, int ny, int nz) {
    if (!volume_dims_ok(nx, ny, nz)) return 0;
    const long long voxels = (long long)nx * ny * nz;
    return (size_t)tiles_of(voxels) * 2 * sizeof(u64) + (size_t)voxels * 6;
}

int tsdf_mesh_count(const TsdfVol &v, float min_weight, long long *totals, void *ws, size_t ws_bytes, hipStream_t stream) {
    long long voxels = 0;
    EDV_TRY(check_volume(v, voxels));
    EDV_CHECK(totals && aligned_to(totals, 8), "totals missing or not 8-byte aligned");
    EDV_TRY(check_mesh_workspace(v, ws, ws_bytes));
    const long long tiles = tiles_of(voxels);
    const MeshWorkspace m = mesh_workspace_of(ws, voxels);
    const dim3 per_voxel((unsigned)((voxels + TSDF_THREADS - 1) / TSDF_THREADS)), per_tile((unsigned)tiles), block(TSDF_THREADS);
    EDV_LAUNCH(mesh_flags_kernel, per_voxel, block, 0, stream, v, min_weight, (unsigned)voxels, m.flags);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(mesh_count_kernel, per_tile, block, 0, stream, v, (unsigned)voxels, m.flags, m.mask, m.vertex_tiles, m.triangle_tiles);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, m.vertex_tiles, tiles, 0ll, totals, 0ll);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, m.triangle_tiles, tiles, 0ll, totals + 1, 0ll);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(mesh_base_kernel, per_tile, block, 0, stream, (unsigned)voxels, m.mask, m.vertex_tiles, m.base);
    EDV_LAUNCH_OK();
    return 0;
}

int tsdf_mesh_extract(const TsdfVol &v, const void *ws, size_t ws_bytes, float *vertices, float *normals, uint8_t *colors, long long vertex_capacity,
                      int *triangles, long long triangle_capacity, hipStream_t stream) {
    long long voxels = 0;
    EDV_TRY(check_volume(v, voxels));
    EDV_TRY(check_mesh_workspace(v, ws, ws_bytes));
    EDV_CHECK(vertex_capacity >= 0 && triangle_capacity >= 0, "negative capacity");
    EDV_CHECK(vertex_capacity < (1ll << 31), "2^31 vertices or more: the triangle indices are int32");
    EDV_CHECK(vertices && aligned_to(vertices, 4) && aligned_to(normals, 4), "vertices missing, or vertices or normals not 4-byte aligned");
    EDV_CHECK(triangles && aligned_to(triangles, 4), "triangles missing or not 4-byte aligned");
    EDV_CHECK(!colors || v.color, "colours asked of a volume that has none");
    const MeshWorkspace m = mesh_workspace_of(ws, voxels);
    const dim3 block(TSDF_THREADS);
    if (vertex_capacity > 0) {
        EDV_LAUNCH(mesh_vertex_kernel, dim3((unsigned)((voxels + TSDF_THREADS - 1) / TSDF_THREADS)), block, 0, stream, v, (unsigned)voxels, m.mask, m.base, vertices,
                   normals, colors, (u64)vertex_capacity);
        EDV_LAUNCH_OK();
    }
    if (triangle_capacity > 0) {
        EDV_LAUNCH(mesh_triangle_kernel, dim3((unsigned)tiles_of(voxels)), block, 0, stream, v, (unsigned)voxels, m.flags, m.mask, m.base, m.triangle_tiles, triangles,
                   (u64)triangle_capacity);
        EDV_LAUNCH_OK();
    }
    return 0;
}

}  // namespace edv
