#pragma clang fp contract(off)
// Coarse-to-fine camera tracking: the image pyramids of one live frame.  The tracker (fusion._track) runs its first ICP steps on coarse copies of
// the frame against the volume ray-cast at the same coarse size; the sums, the normals and the ray-cast take any grid size and intrinsics, so
// what is new on the device is what makes the levels.  The rule is stated once, in include/endodav_hip.h; fusion.depth_pyramid_host and
// fusion.rgb_pyramid_host are the mirrors, bit for bit.
//   depth  level 0 is the frame read through the cloud's selection (step 1): the raw depth d_0 (the depth rule without its last multiply by
//          the gain), valid where the cloud keeps the pixel.  Level l + 1 takes the 2 x 2 block of level l: the smallest valid value m, the
//          valid values d <= m * (1 + jump) summed in block order and divided by their count; +0 where nothing is valid.  A stored +0 is the
//          mark of "not valid" from level 1 on.
//   rgb    per channel (a + b + c + d + 2) >> 2 over the same block
// Level l + 1 depends only on its own 2 x 2 block, so a tile of level 0 aligned to PYRAMID_TILE = 2^(PYRAMID_MAX_LEVELS - 1) holds everything
// its pixels of every level need.  One launch makes all levels of one frame:
//   pyramid_kernel  a workgroup of 256 per 32 x 32 tile of level 0, one thread per pixel of level 1: it reads its four pixels of level 0 from
//                   global memory (two pairs a row apart, neighbouring lanes neighbouring pairs), reduces, stores level 1 and leaves the value
//                   in LDS; then 64, 16, 4 and 1 threads reduce LDS to LDS for levels 2..5 and store them.  A pixel beyond a level's ragged
//                   edge (an odd last row or column is dropped) is neither read nor written; its LDS slot holds "nothing" and no pixel inside
//                   the level reads it, since a pixel inside level l + 1 has its whole block inside level l.
// No atomics, no workgroup waits for another, every pixel of every level written exactly once (zeros included) and nothing outside the levels.
// Contraction is off for the whole file and the division is IEEE's.
#include <cmath>

#include "ops.hpp"

#include "cloud_common.hpp"  // depth_value's rule, check_selection

namespace edv {
namespace {

constexpr int PYRAMID_MAX_LEVELS = 6;                  // level 0 and up to five coarser ones: the one constant behind pyramid_max_levels()
constexpr int PYRAMID_TILE = 1 << (PYRAMID_MAX_LEVELS - 1);  // 32 pixels of level 0 a side
constexpr int PYRAMID_HALF = PYRAMID_TILE / 2;         // 16 pixels of level 1 a side
constexpr int PYRAMID_THREADS = PYRAMID_HALF * PYRAMID_HALF;
static_assert(PYRAMID_THREADS == 256 && PYRAMID_MAX_LEVELS >= 4);

struct PyramidLevels {
    int count;                          // coarser levels, 1 .. PYRAMID_MAX_LEVELS - 1
    int h[PYRAMID_MAX_LEVELS], w[PYRAMID_MAX_LEVELS];  // [0]: the frame
    long long offset[PYRAMID_MAX_LEVELS];              // pixels in front of level l in the output; [0] unused
};

// the sizes and offsets of `levels` coarser levels of an h x w frame; false where a level would be empty or the arguments are out of range
inline bool pyramid_levels(int h, int w, int levels, PyramidLevels &p) {
    if (h < 1 || w < 1 || levels < 1 || levels > PYRAMID_MAX_LEVELS - 1 || (long long)h * w >= (1ll << 31)) return false;
    p.count = levels, p.h[0] = h, p.w[0] = w, p.offset[0] = 0;
    long long at = 0;
    for (int l = 1; l <= levels; ++l) {
        p.h[l] = p.h[l - 1] / 2, p.w[l] = p.w[l - 1] / 2, p.offset[l] = at;
        if (p.h[l] < 1 || p.w[l] < 1) return false;
        at += (long long)p.h[l] * p.w[l];
    }
    for (int l = levels + 1; l < PYRAMID_MAX_LEVELS; ++l) p.h[l] = p.w[l] = 0, p.offset[l] = at;
    return true;
}

// the depth levels: a float a pixel, +0 for "not valid"
struct DepthPyramid {
    using Value = float;
    CloudSel s;
    const float *xf;      // the frame
    const uint8_t *mf;    // its mask or null
    float one_plus_jump;
    float *out;

    // pixel p of level 0: the raw depth where the cloud keeps the pixel, +0 elsewhere.  near_z >= 0 and gain > 0 (checked on the host side of
    // the launch), so a kept pixel has d > 0
    __device__ __forceinline__ float load(int p) const {
        const float x = xf[p];
        float d = x;
        if (s.mode != 0) {
            const float scaled = s.lo + s.span * x;
            d = 1.0f / scaled;
        }
        const float z = d * s.gain;
        const bool keep = (mf ? mf[p] : 1u) != 0 && z > s.near_z && z < s.far_z;  // the cloud's kept: NaN and Inf fail
        return keep ? d : 0.0f;
    }
    // a block in the order (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1); level 0 marks "not valid" by +0 too (load above).  Valid values are
    // finite and positive
    __device__ __forceinline__ float reduce(const float (&d)[4]) const {
        float m = INFINITY;
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (d[k] != 0.0f) m = fminf(m, d[k]), any = true;
        }
        if (!any) return 0.0f;
        const float limit = m * one_plus_jump;
        float sum = 0.0f;  // +0 + d == d for the first used value
        int count = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (d[k] != 0.0f && d[k] <= limit) sum = sum + d[k], ++count;
        }
        return sum / (float)count;
    }
    __device__ __forceinline__ static float nothing() { return 0.0f; }
    __device__ __forceinline__ void store(long long at, float v) const { out[at] = v; }
};

// the colour levels: a pixel packed as r | g << 8 | b << 16
struct RgbPyramid {
    using Value = unsigned;
    const uint8_t *rgb;  // the frame [h][w][3]
    uint8_t *out;

    __device__ __forceinline__ unsigned load(int p) const {
        const uint8_t *c = rgb + (size_t)p * 3;
        return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
    }
    __device__ __forceinline__ unsigned reduce(const unsigned (&d)[4]) const {
        unsigned v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int sh = 8 * ch;
            const unsigned sum = (d[0] >> sh & 255u) + (d[1] >> sh & 255u) + (d[2] >> sh & 255u) + (d[3] >> sh & 255u) + 2u;
            v |= (sum >> 2) << sh;
        }
        return v;
    }
    __device__ __forceinline__ static unsigned nothing() { return 0u; }
    __device__ __forceinline__ void store(long long at, unsigned v) const {
        uint8_t *c = out + (size_t)at * 3;
        c[0] = (uint8_t)(v & 255u), c[1] = (uint8_t)(v >> 8 & 255u), c[2] = (uint8_t)(v >> 16 & 255u);
    }
};

// grid: ceil(w_1 / 16) * ceil(h_1 / 16), row-major in x alone (a tall frame has more rows of tiles than a grid's y holds): the tiles of level 0
// that hold a pixel of level 1, tiles_x of them a row.  Every level's pixels of the tile are written here
template <typename P>
__global__ __launch_bounds__(PYRAMID_THREADS) void pyramid_kernel(P q, PyramidLevels lv, unsigned tiles_x) {
    using V = typename P::Value;
    // level l of the tile at tile[l - 1]: 16 x 16, 8 x 8, 4 x 4, 2 x 2, 1 x 1, each with its own row length
    __shared__ V tile[PYRAMID_MAX_LEVELS - 1][PYRAMID_THREADS];
    const int t = threadIdx.x;
    const int tile_y = (int)(blockIdx.x / tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * tiles_x);
    {
        const int ly = t / PYRAMID_HALF, lx = t % PYRAMID_HALF;
        const int y = tile_y * PYRAMID_HALF + ly, x = tile_x * PYRAMID_HALF + lx;  // of level 1
        V v = P::nothing();
        if (y < lv.h[1] && x < lv.w[1]) {  // then rows 2y, 2y+1 and columns 2x, 2x+1 lie in the frame
            const int p = 2 * y * lv.w[0] + 2 * x;  // h * w < 2^31
            const V d[4] = {q.load(p), q.load(p + 1), q.load(p + lv.w[0]), q.load(p + lv.w[0] + 1)};
            v = q.reduce(d);
            q.store(lv.offset[1] + (long long)y * lv.w[1] + x, v);
        }
        tile[0][t] = v;
    }
    __syncthreads();
    int side = PYRAMID_HALF;  // of the level below, inside the tile
    for (int l = 2; l <= lv.count; ++l) {  // uniform over the workgroup; every level's LDS writes are followed by the barrier in straight-line code
        const int below = side;
        side >>= 1;
        if (t < side * side) {
            const int ly = t / side, lx = t % side;
            const int y = tile_y * side + ly, x = tile_x * side + lx;  // of level l
            V v = P::nothing();
            if (y < lv.h[l] && x < lv.w[l]) {
                const V *src = tile[l - 2] + 2 * ly * below + 2 * lx;
                const V d[4] = {src[0], src[1], src[below], src[below + 1]};
                v = q.reduce(d);
                q.store(lv.offset[l] + (long long)y * lv.w[l] + x, v);
            }
            tile[l - 1][t] = v;
        }
        __syncthreads();
    }
}

inline unsigned pyramid_tiles(int n1) { return (unsigned)((n1 + PYRAMID_HALF - 1) / PYRAMID_HALF); }  // tiles along an axis of n1 pixels of level 1

}  // namespace

int pyramid_max_levels() { return PYRAMID_MAX_LEVELS; }

size_t pyramid_pixels(int h, int w, int levels, long long *offsets) {
    PyramidLevels lv;
    if (!pyramid_levels(h, w, levels, lv)) return 0;
    if (offsets) {
        for (int l = 1; l <= levels; ++l) offsets[l - 1] = lv.offset[l];
    }
    return (size_t)(lv.offset[levels] + (long long)lv.h[levels] * lv.w[levels]);
}

int depth_pyramid(const CloudSel &s, long long frame, int levels, float one_plus_jump, float *out, hipStream_t stream) {
    EDV_TRY(check_selection(s));
    EDV_CHECK(s.step == 1, "the pyramid's level 0 is the full-resolution frame: step must be 1");
    EDV_CHECK(s.near_z >= 0.0f && s.gain > 0.0f, "near_z must be >= 0 and gain > 0: a stored +0 marks a pixel that is not valid");
    EDV_CHECK(frame >= 0 && frame < s.n, "frame outside the clip");
    EDV_CHECK(one_plus_jump >= 1.0f, "one_plus_jump must be >= 1 (+inf: every valid value is used), not NaN");
    EDV_CHECK(out && aligned_to(out, 4), "output missing or not 4-byte aligned");
    PyramidLevels lv;
    EDV_CHECK(pyramid_levels(s.h, s.w, levels, lv), "levels must be in 1 .. edv_pyramid_max_levels() - 1 and every level hold a pixel");
    const DepthPyramid q{s, s.x + frame * s.h * s.w, s.mask ? s.mask + frame * s.mask_stride : nullptr, one_plus_jump, out};
    const unsigned tiles_x = pyramid_tiles(lv.w[1]), tiles = tiles_x * pyramid_tiles(lv.h[1]);  // h_1 * w_1 < 2^29: fewer than 2^31 tiles
    EDV_LAUNCH(pyramid_kernel<DepthPyramid>, dim3(tiles), dim3(PYRAMID_THREADS), 0, stream, q, lv, tiles_x);
    EDV_LAUNCH_OK();
    return 0;
}

int rgb_pyramid(const uint8_t *frames, long long n, int h, int w, long long frame, int levels, uint8_t *out, hipStream_t stream) {
    EDV_CHECK(frames, "null frames");
    EDV_CHECK(n >= 1 && frame >= 0 && frame < n, "frame outside the clip");
    EDV_CHECK(out, "null output");
    PyramidLevels lv;
    EDV_CHECK(pyramid_levels(h, w, levels, lv), "h * w must be in 1 .. 2^31 - 1, levels in 1 .. edv_pyramid_max_levels() - 1 and every level hold a pixel");
    const RgbPyramid q{frames + (size_t)frame * 3 * h * w, out};
    const unsigned tiles_x = pyramid_tiles(lv.w[1]), tiles = tiles_x * pyramid_tiles(lv.h[1]);  // h_1 * w_1 < 2^29: fewer than 2^31 tiles
    EDV_LAUNCH(pyramid_kernel<RgbPyramid>, dim3(tiles), dim3(PYRAMID_THREADS), 0, stream, q, lv, tiles_x);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace edv
