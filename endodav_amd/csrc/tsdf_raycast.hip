#pragma clang fp contract(off)
// Views of the TSDF volume of tsdf.hip: every pixel of every camera marches its ray through the volume in equal steps of depth, samples the
// distance by trilinear interpolation, and stops at the first change from outside (s >= 0) to inside (s < 0) between two neighbouring valid
// samples.  Depth, and optionally the normal and the colour at the hit, are written for every pixel; a miss writes zeros.  The rule is stated
// once, in include/endodav_hip.h; fusion.TsdfHost.raycast is the mirror, bit for bit.
//   tsdf_raycast   one launch for all views, one thread per pixel.  A workgroup is a 16 x 16 pixel tile and a wave an 8 x 8 block of it, so the rays
//                  of a wave stay within a few voxels of each other and its sixteen gathers per sample (eight weights, eight distances) fall
//                  into the same few cache lines; a row segment of 64 pixels would spread them over 64 voxels' worth of lines.
// Per sample the loop holds four fp64 multiply-adds (z_k and the three g_i), the box test, three conversions and differences, and fp32 after
// that.  The eight weights are read first and the eight distances only where all of them pass.  No division in the loop: the rule multiplies by
// 1 / voxel (integrate is bound by its fp64 divisions).
// Each ray's k range is cut to where it can be inside the box of voxel centres: a slab test in fp64, widened in g by 2^-40 (|o_i| + n_i), in
// z by 2^-40 |z| and then by one step on either side, all far more than the roundings of g_i (2^-52 of its terms).  The test inside the loop
// stays authoritative, so the cut only skips samples the rule calls not valid: before the first of them nothing is remembered, which is the
// state the march starts in, and after the last no hit can follow.  A doubt (NaN) keeps the full range.
// No atomics, no LDS, no workgroup waits for another; every pixel of every output is written exactly once by plain stores, so the same input
// gives the same bytes on every call.  Contraction is off for the whole file, the division and the square root are IEEE's.
#include <cmath>

#include "ops.hpp"

#include "tsdf_common.hpp"  // hop_of, gradient, check_volume

namespace edv {
namespace {

constexpr int RAY_TILE = 16, RAY_THREADS = RAY_TILE * RAY_TILE;
constexpr int RAY_MAX_STEPS = 65536;

// 0 <= g_i <= n_i - 1 on every axis; NaN fails
__device__ __forceinline__ bool in_box(const TsdfVol &v, const double (&g)[3]) {
    return g[0] >= 0.0 && g[0] <= (double)(v.nx - 1) && g[1] >= 0.0 && g[1] <= (double)(v.ny - 1) && g[2] >= 0.0 && g[2] <= (double)(v.nz - 1);
}

// the cell c_i = min(max((int)g_i, 0), n_i - 2) that holds g and the position f_i = (float)(g_i - c_i) inside it.  Every n_i >= 2 here.
__device__ __forceinline__ void cell_of(const TsdfVol &v, const double (&g)[3], unsigned (&c)[3], float (&f)[3]) {
    const int n[3] = {v.nx, v.ny, v.nz};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int ci = (int)g[i];
        ci = ci < 0 ? 0 : ci;
        ci = ci > n[i] - 2 ? n[i] - 2 : ci;
        c[i] = (unsigned)ci;
        f[i] = (float)(g[i] - (double)ci);
    }
}

// corner c = x | y << 1 | z << 2: along x, then y, then z, every operation rounded on its own
__device__ __forceinline__ float trilinear(const float (&q)[8], const float (&f)[3]) {
    const float a00 = q[0] + f[0] * (q[1] - q[0]), a10 = q[2] + f[0] * (q[3] - q[2]);
    const float a01 = q[4] + f[0] * (q[5] - q[4]), a11 = q[6] + f[0] * (q[7] - q[6]);
    const float b0 = a00 + f[1] * (a10 - a00), b1 = a01 + f[1] * (a11 - a01);
    return b0 + f[2] * (b1 - b0);
}

// the range of z in which o + d * z can lie in [0, n - 1], widened; `lo > hi` is an empty range.  NaN leaves lo and hi as they are.
__device__ __forceinline__ void slab(double o, double d, int n, double &lo, double &hi) {
    const double e = 0x1p-40 * (fabs(o) + (double)n);
    const double g0 = -e, g1 = (double)(n - 1) + e;
    if (d == 0.0) {
        if (o < g0 || o > g1) lo = 1.0, hi = 0.0;
        return;
    }
    const double z0 = (g0 - o) / d, z1 = (g1 - o) / d;
    const double a = z0 < z1 ? z0 : z1, b = z0 < z1 ? z1 : z0;
    if (a > lo) lo = a;
    if (b < hi) hi = b;
}

// grid: views * tiles_y * tiles_x.  cam = Kinv[3][3], R[3][3], t[3]; normals and colors may be null
__global__ __launch_bounds__(RAY_THREADS) void tsdf_raycast_kernel(TsdfVol v, const double *__restrict__ cams, int h, int w, unsigned tiles_x, unsigned tiles_y, double inv,
                                                                   double near, double step, int steps, float min_weight, float *__restrict__ depth,
                                                                   float *__restrict__ normals, uint8_t *__restrict__ colors) {
    const unsigned tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x, ty = rest % tiles_y, view = rest / tiles_y;
    // wave i of the four is the 8 x 8 block (i & 1, i >> 1) of the tile; inside it x runs along the lanes first
    const unsigned t = threadIdx.x, lx = (t & 7u) | (((t >> 6) & 1u) << 3), ly = ((t >> 3) & 7u) | ((t >> 7) << 3);
    const unsigned x = tx * RAY_TILE + lx, y = ty * RAY_TILE + ly;
    if (x >= (unsigned)w || y >= (unsigned)h) return;
    const size_t p = ((size_t)view * (unsigned)h + y) * (unsigned)w + x;
    const double *cam = cams + (size_t)view * 21;
    const double pu = (double)x + 0.5, pv = (double)y + 0.5;
    double l[3], o[3], d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) l[i] = (cam[3 * i] * pu + cam[3 * i + 1] * pv) + cam[3 * i + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double r = (cam[9 + 3 * i] * l[0] + cam[10 + 3 * i] * l[1]) + cam[11 + 3 * i] * l[2];
        o[i] = (cam[18 + i] - v.origin[i]) * inv - 0.5;
        d[i] = r * inv;
    }
    int k0 = 0, k1 = steps - 1;
    if (v.nx < 2 || v.ny < 2 || v.nz < 2) {
        k1 = -1;  // a volume without a cell: every pixel is a miss
    } else {
        double lo = -INFINITY, hi = INFINITY;
        slab(o[0], d[0], v.nx, lo, hi);
        slab(o[1], d[1], v.ny, lo, hi);
        slab(o[2], d[2], v.nz, lo, hi);
        if (lo > hi) {
            k1 = -1;
        } else {
            const double first = floor(((lo - 0x1p-40 * fabs(lo)) - near) / step) - 1.0, last = ceil(((hi + 0x1p-40 * fabs(hi)) - near) / step) + 1.0;
            if (first > (double)(steps - 1) || last < 0.0) {
                k1 = -1;
            } else {
                if (first > 0.0) k0 = (int)first;  // below steps, from the test above
                if (last < (double)(steps - 1)) k1 = (int)last;
            }
        }
    }
    const unsigned hop[8] = {0u, hop_of(v, 1), hop_of(v, 2), hop_of(v, 3), hop_of(v, 4), hop_of(v, 5), hop_of(v, 6), hop_of(v, 7)};
    bool have = false, hit = false;
    float sp = 0.0f, frac = 0.0f;
    int kh = 0;
    for (int k = k0; k <= k1; ++k) {
        const double z = near + (double)k * step;
        const double g[3] = {o[0] + d[0] * z, o[1] + d[1] * z, o[2] + d[2] * z};
        if (!in_box(v, g)) {
            have = false;
            continue;
        }
        unsigned c[3];
        float f[3];
        cell_of(v, g, c, f);
        const unsigned a = c[0] + (unsigned)v.nx * (c[1] + (unsigned)v.ny * c[2]);
        bool valid = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) valid = valid && v.weight[a + hop[j]] >= min_weight;
        if (!valid) {
            have = false;
            continue;
        }
        float q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = v.tsdf[a + hop[j]];
        const float s = trilinear(q, f);
        if (!(s < 0.0f)) {  // 0 and -0 count as outside
            have = true, sp = s;
            continue;
        }
        if (have) hit = true, frac = sp / (sp - s), kh = k - 1;  // the divisor is positive
        break;  // a hit, or the ray entered the surface from unobserved space or started inside: a miss
    }
    float out_z = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f};
    uint8_t out_c[3] = {0, 0, 0};
    if (hit) {
        const double zs = (near + (double)kh * step) + (double)frac * step;
        out_z = (float)zs;
        if (normals || colors) {
            const double g[3] = {o[0] + d[0] * zs, o[1] + d[1] * zs, o[2] + d[2] * zs};
            unsigned c[3];
            float f[3];
            cell_of(v, g, c, f);  // the clamp keeps the cell in the grid whatever the rounding
            const unsigned a = c[0] + (unsigned)v.nx * (c[1] + (unsigned)v.ny * c[2]);
            if (normals) {
                float gx[8], gy[8], gz[8];
#pragma unroll
                for (unsigned j = 0; j < 8; ++j) {
                    float gr[3];
                    gradient(v, a + hop[j], c[0] + (j & 1u), c[1] + ((j >> 1) & 1u), c[2] + ((j >> 2) & 1u), gr);
                    gx[j] = gr[0], gy[j] = gr[1], gz[j] = gr[2];
                }
                const float n[3] = {trilinear(gx, f), trilinear(gy, f), trilinear(gz, f)};
                const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
                for (int j = 0; j < 3; ++j) out_n[j] = len > 0.0f ? n[j] / len : 0.0f;
            }
            if (colors) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float q[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) q[j] = v.color[(size_t)(a + hop[j]) * 3 + ch];
                    out_c[ch] = (uint8_t)fminf(255.0f, fmaxf(0.0f, floorf(trilinear(q, f) + 0.5f)));
                }
            }
        }
    }
    depth[p] = out_z;
    if (normals) {
        float *on = normals + p * 3;
        on[0] = out_n[0], on[1] = out_n[1], on[2] = out_n[2];
    }
    if (colors) {
        uint8_t *oc = colors + p * 3;
        oc[0] = out_c[0], oc[1] = out_c[1], oc[2] = out_c[2];
    }
}

}  // namespace

int tsdf_raycast(const TsdfVol &v, const double *cams, int views, int h, int w, double near, double step, int steps, float min_weight, float *depth,
                 float *normals, uint8_t *colors, hipStream_t stream) {
    long long voxels = 0;
    EDV_TRY(check_volume(v, voxels));
    EDV_CHECK(cams && aligned_to(cams, 8), "cameras missing or not 8-byte aligned");
    EDV_CHECK(views >= 1 && h >= 1 && w >= 1, "views, h and w must be at least 1");
    EDV_CHECK((long long)views * h * w < (1ll << 31), "2^31 pixels or more");
    EDV_CHECK(positive(step) && std::isfinite(near), "step must be finite and positive and near finite");
    EDV_CHECK(steps >= 1 && steps <= RAY_MAX_STEPS, "steps must be 1 to 65536");
    EDV_CHECK(depth && aligned_to(depth, 4) && aligned_to(normals, 4), "depth missing, or depth or normals not 4-byte aligned");
    EDV_CHECK(!colors || v.color, "colours asked of a volume that has none");
    const unsigned tiles_x = (unsigned)((w + RAY_TILE - 1) / RAY_TILE), tiles_y = (unsigned)((h + RAY_TILE - 1) / RAY_TILE);
    const long long blocks = (long long)views * tiles_x * tiles_y;  // at most one per pixel: below 2^31
    EDV_LAUNCH(tsdf_raycast_kernel, dim3((unsigned)blocks), dim3(RAY_THREADS), 0, stream, v, cams, h, w, tiles_x, tiles_y, 1.0 / v.voxel, near, step, steps, min_weight,
               depth, normals, colors);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace edv
