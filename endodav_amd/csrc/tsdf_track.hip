#pragma clang fp contract(off)
// Camera tracking against the fused surface: the normal equations of one point-to-plane ICP step.  A live depth frame, lifted through the
// current estimate of its camera, is associated projectively with one view of tsdf_raycast.hip (the model's depth and normal maps seen from the
// previous pose), and the 6 x 6 system of the twist about the live camera centre is summed over the pairs.  The rule is stated once, in
// include/endodav_hip.h; fusion.icp_sums_host is the mirror, bit for bit.  With the frame's depth scale as a seventh unknown (icp_scaled_sums)
// the column J_6 = rho . N joins the six and the system is 7 x 7: 37 terms instead of 29, the same kernels instantiated on the column count,
// the same order of every sum, so the 29 values the two share come out with the same bits.
//   icp_tile   one workgroup per tile of ICP_TILE output pixels of the cloud's grid in row-major order, one thread per pixel: the pixel's 29
//              terms in fp64 (the upper triangle of J J^T, J e, e e and 1; 29 times +0 for a pixel without a pair), summed over the wave by a
//              butterfly and over the four waves in wave order (common.hpp's block_sum_store), one row of 29 doubles per tile in the workspace
//   icp_total  a workgroup of 64 per 64 values (one for 29 or 37): thread j adds value j of the tiles in index order, starting from tile 0's, and stores sums[j]
// The two cameras travel in the launch arguments, read from host memory before the call returns: the live pose changes with every iteration and
// nothing is staged.  The model is addressed only after its pixel passed the range test in fp64, and the live frame only inside the grid, so a
// guess that looks anywhere reads nothing outside the arrays.
// No atomics, no workgroup waits for another, a fixed order of every addition: the same input gives the same bits on every call.  Every slot of
// the workspace that is read and all 29 (37) outputs are written on every call.  Contraction is off for the whole file and the division is IEEE's.
// With colour (icp_colour_sums) every geometric pair also compares the live frame's intensity with the model view's colour image, sampled
// bilinearly where the point projects: a second block of 29 (37) terms with the intensity's gradient for N and the intensity difference for e.
//   icp_colour_tile   icp_tile with 2 * 29 (37) terms a pixel: the geometric block through the same icp_terms, so with the same bits, then the colour block
//   icp_total         as above, two workgroups for the 58 or 74 values
// The robust step (icp_robust_sums) tests a pair twice more: its orientation, the live frame's own normal against the model's, and the size
// of its residual, a Huber weight on its row.  The pair comes from the same icp_pair and icp_colour_pair as above, so up to the distance test the
// rule is shared code; the terms from the same icp_fill, with the weight on one factor of each product.
//   frame_normals     one thread per output pixel and frame: the unit normal in the camera's frame from central differences of the cloud's
//                     vertices, (0, 0, 0) where the pixel or one of its four neighbours is not kept or lies outside the grid
//   icp_robust_tile   icp_tile or icp_colour_tile (T or 2 T terms a pixel) with the normal test behind the distance test and the weights
//   icp_total         as above
#include <cmath>

#include "ops.hpp"

#include "cloud_common.hpp"  // depth_value, kept, source_pixel, check_selection: shared with pointcloud.hip and tsdf.hip

namespace edv {
namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_TILE = ICP_THREADS;  // output pixels per workgroup: the one constant behind icp_tile_pixels()
constexpr int icp_term_count(int cols) { return cols * (cols + 1) / 2 + cols + 2; }  // the upper triangle of J J^T, J e, e e and 1
static_assert(icp_term_count(6) == 29 && icp_term_count(7) == 37);
constexpr int ICP_TOTAL_THREADS = 64;

struct IcpCams {
    double live[21];   // Kinv[3][3], R[3][3], t[3] of the estimate
    double model[39];  // the model view's Kinv, R, t, then W[3][4] and K00 K01 K02 K10 K11 K12
};

// (M[0]*a + M[1]*b) + M[2]*c for the three rows of a row-major 3 x 3
__device__ __forceinline__ void rows3(const double *M, double a, double b, double c, double (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (M[3 * i] * a + M[3 * i + 1] * b) + M[3 * i + 2] * c;
}

// a geometric pair: the source pixel of the live frame, the lever arm, the point in the model camera's frame and where it projects (what the
// colour term takes over), the model's normal, and the residual with its row of the system (J[6] only with seven columns)
struct IcpPair {
    int p;
    double rho[3], q0, q1, q2, um, vm, N[3], e, J[7];
};

// the T terms of a row J with the residual e into a[0..T): the upper triangle of J J^T row-major, J e, e e and 1.  WEIGHTED: the robust rule,
// Jw_j = w * J_j in place of the first factor of the triangle and of J e; e e stays as it is.  With w = 1 both give the same bits.
template <int COLS, bool WEIGHTED>
__device__ __forceinline__ void icp_fill(const double *__restrict__ J, double e, double w, double *__restrict__ a) {
    constexpr int TRI = COLS * (COLS + 1) / 2;
    double Jw[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) Jw[j] = WEIGHTED ? w * J[j] : J[j];
    int t = 0;
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
#pragma unroll
        for (int k = j; k < COLS; ++k) a[t++] = Jw[j] * J[k];
    }
#pragma unroll
    for (int j = 0; j < COLS; ++j) a[TRI + j] = Jw[j] * e;
    a[TRI + COLS] = e * e;
    a[TRI + COLS + 1] = 1.0;
}

// the pair of output pixel q < grid_pixels of the live frame, through the distance test, e and J; false, with g untouched but for g.p, for a
// pixel without one
template <int COLS>
__device__ __forceinline__ bool icp_pair(const CloudSel &s, const IcpCams &c, const float *__restrict__ xf, const uint8_t *__restrict__ mf, int ow, unsigned q,
                                         const float *__restrict__ model_depth, const float *__restrict__ model_normals, int mh, int mw, double max_dist2, IcpPair &g) {
    int ox, oy;
    const int p = g.p = source_pixel(s, ow, q, ox, oy);
    float z;
    if (!kept(s, xf[p], mf ? mf[p] : 1u, z)) return false;
    const double u = ((double)ox + 0.5) * (double)s.step, v = ((double)oy + 0.5) * (double)s.step;
    double l[3], r[3], rho[3], P[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) l[i] = (c.live[3 * i] * u + c.live[3 * i + 1] * v) + c.live[3 * i + 2];
    rows3(c.live + 9, l[0], l[1], l[2], r);
#pragma unroll
    for (int i = 0; i < 3; ++i) rho[i] = r[i] * (double)z, P[i] = c.live[18 + i] + rho[i];
    // into the model view, as tsdf_integrate projects a voxel centre
    const double *W = c.model + 21, *K = c.model + 33;
    const double q2 = ((W[8] * P[0] + W[9] * P[1]) + W[10] * P[2]) + W[11];
    if (!(q2 > 0.0)) return false;  // behind the model camera, or NaN
    const double q0 = ((W[0] * P[0] + W[1] * P[1]) + W[2] * P[2]) + W[3];
    const double q1 = ((W[4] * P[0] + W[5] * P[1]) + W[6] * P[2]) + W[7];
    const double um = ((K[0] * q0 + K[1] * q1) + K[2] * q2) / q2;
    const double vm = ((K[3] * q0 + K[4] * q1) + K[5] * q2) / q2;
    if (!(um >= 0.0 && um < (double)mw && vm >= 0.0 && vm < (double)mh)) return false;  // in fp64, before any conversion: 0 <= px < mw and 0 <= py < mh below
    const int px = (int)um, py = (int)vm;
    const size_t at = (size_t)py * (unsigned)mw + (unsigned)px;
    const float dm = model_depth[at];
    if (!(dm > 0.0f)) return false;  // a miss is +0; NaN fails
    const double N[3] = {(double)model_normals[at * 3], (double)model_normals[at * 3 + 1], (double)model_normals[at * 3 + 2]};
    if (!((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2] > 0.0)) return false;
    // the model's vertex: the cloud's lift of its own pixel centre
    const double mu = (double)px + 0.5, mv = (double)py + 0.5;
    double lm[3], rm[3], D[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) lm[i] = (c.model[3 * i] * mu + c.model[3 * i + 1] * mv) + c.model[3 * i + 2];
    rows3(c.model + 9, lm[0], lm[1], lm[2], rm);
#pragma unroll
    for (int i = 0; i < 3; ++i) D[i] = (c.model[18 + i] + rm[i] * (double)dm) - P[i];
    if (!((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2] <= max_dist2)) return false;
    const double e = (N[0] * D[0] + N[1] * D[1]) + N[2] * D[2];
    const double J[6] = {rho[1] * N[2] - rho[2] * N[1], rho[2] * N[0] - rho[0] * N[2], rho[0] * N[1] - rho[1] * N[0], N[0], N[1], N[2]};
#pragma unroll
    for (int j = 0; j < 6; ++j) g.J[j] = J[j];
    if constexpr (COLS == 7) g.J[6] = (rho[0] * N[0] + rho[1] * N[1]) + rho[2] * N[2];  // the scale: P moves by delta * rho
#pragma unroll
    for (int i = 0; i < 3; ++i) g.rho[i] = rho[i], g.N[i] = N[i];
    g.q0 = q0, g.q1 = q1, g.q2 = q2, g.um = um, g.vm = vm, g.e = e;
    return true;
}

// the T = 29 (COLS = 6) or 37 (COLS = 7) terms of output pixel q into a[0..T); false, with `a` untouched, for a pixel without a pair.  `a` may
// be longer: the colour kernel keeps its second block behind the first.
template <int COLS, int LEN>
__device__ __forceinline__ bool icp_terms(const CloudSel &s, const IcpCams &c, const float *__restrict__ xf, const uint8_t *__restrict__ mf, int ow, unsigned q,
                                          const float *__restrict__ model_depth, const float *__restrict__ model_normals, int mh, int mw, double max_dist2,
                                          double (&a)[LEN], IcpPair &g) {
    static_assert(LEN >= icp_term_count(COLS));
    if (!icp_pair<COLS>(s, c, xf, mf, ow, q, model_depth, model_normals, mh, mw, max_dist2, g)) return false;
    icp_fill<COLS, false>(g.J, g.e, 1.0, a);
    return true;
}

// (0.299*R + 0.587*G) + 0.114*B of a uint8 triple
__device__ __forceinline__ double intensity(const uint8_t *__restrict__ rgb) { return (0.299 * (double)rgb[0] + 0.587 * (double)rgb[1]) + 0.114 * (double)rgb[2]; }

// the colour pair of a pixel that has the geometric pair g: its row J and residual r; false, with both untouched, where there is none
template <int COLS>
__device__ __forceinline__ bool icp_colour_pair(const IcpCams &c, const IcpPair &g, const uint8_t *__restrict__ live_rgb, const float *__restrict__ model_depth,
                                                const uint8_t *__restrict__ model_colors, int mh, int mw, double (&J)[COLS], double &r) {
    const double gu = g.um - 0.5, gv = g.vm - 0.5;
    if (!(mw >= 2 && mh >= 2 && gu >= 0.0 && gu <= (double)(mw - 1) && gv >= 0.0 && gv <= (double)(mh - 1))) return false;  // in fp64, before any conversion
    const int x0 = min((int)gu, mw - 2), y0 = min((int)gv, mh - 2);  // 0 <= x0 <= mw - 2 and 0 <= y0 <= mh - 2: the four pixels lie in the view
    const double fx = gu - (double)x0, fy = gv - (double)y0;
    const size_t at = (size_t)y0 * (unsigned)mw + (unsigned)x0;
    if (!(model_depth[at] > 0.0f && model_depth[at + 1] > 0.0f && model_depth[at + (unsigned)mw] > 0.0f && model_depth[at + (unsigned)mw + 1] > 0.0f)) return false;
    const double I00 = intensity(model_colors + at * 3), I10 = intensity(model_colors + (at + 1) * 3);
    const double I01 = intensity(model_colors + (at + (unsigned)mw) * 3), I11 = intensity(model_colors + (at + (unsigned)mw + 1) * 3);
    const double Yl = intensity(live_rgb + (size_t)g.p * 3);
    const double top = I00 + fx * (I10 - I00), bot = I01 + fx * (I11 - I01);
    const double Im = top + fy * (bot - top);
    const double Iu = (I10 - I00) + fy * ((I11 - I01) - (I10 - I00));
    const double Iv = (I01 - I00) + fx * ((I11 - I10) - (I01 - I00));
    // through the projection, into the model camera's frame, then into the world
    const double *W = c.model + 21, *K = c.model + 33;
    const double ka = K[0] * g.q0 + K[1] * g.q1, kb = K[3] * g.q0 + K[4] * g.q1;
    const double gq0 = (Iu * K[0] + Iv * K[3]) / g.q2, gq1 = (Iu * K[1] + Iv * K[4]) / g.q2, gq2 = -((Iu * ka + Iv * kb) / (g.q2 * g.q2));
    double G[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) G[j] = (W[j] * gq0 + W[4 + j] * gq1) + W[8 + j] * gq2;
    r = Yl - Im;
    const double *rho = g.rho;
    const double J6[6] = {rho[1] * G[2] - rho[2] * G[1], rho[2] * G[0] - rho[0] * G[2], rho[0] * G[1] - rho[1] * G[0], G[0], G[1], G[2]};
#pragma unroll
    for (int j = 0; j < 6; ++j) J[j] = J6[j];
    if constexpr (COLS == 7) J[6] = (rho[0] * G[0] + rho[1] * G[1]) + rho[2] * G[2];
    return true;
}

// the colour block of such a pixel: its T terms into a[0..T); false, with `a` untouched, where there is no colour pair
template <int COLS>
__device__ __forceinline__ bool icp_colour_terms(const IcpCams &c, const IcpPair &g, const uint8_t *__restrict__ live_rgb, const float *__restrict__ model_depth,
                                                 const uint8_t *__restrict__ model_colors, int mh, int mw, double *__restrict__ a) {
    double J[COLS], r;
    if (!icp_colour_pair<COLS>(c, g, live_rgb, model_depth, model_colors, mh, mw, J, r)) return false;
    icp_fill<COLS, false>(J, r, 1.0, a);
    return true;
}

// grid: tiles.  tile_sums [tiles][29] (COLS = 6) or [tiles][37] (COLS = 7)
template <int COLS>
__global__ __launch_bounds__(ICP_THREADS) void icp_tile_kernel(CloudSel s, long long frame, IcpCams c, int ow, unsigned grid_pixels, const float *__restrict__ model_depth,
                                                               const float *__restrict__ model_normals, int mh, int mw, double max_dist2,
                                                               double *__restrict__ tile_sums) {
    const unsigned q = blockIdx.x * (unsigned)ICP_TILE + threadIdx.x;
    constexpr int TERMS = icp_term_count(COLS);
    double a[TERMS];
    bool pair = false;
    if (q < grid_pixels) {
        const float *xf = s.x + frame * s.h * s.w;
        const uint8_t *mf = s.mask ? s.mask + frame * s.mask_stride : nullptr;
        IcpPair g;
        pair = icp_terms<COLS>(s, c, xf, mf, ow, q, model_depth, model_normals, mh, mw, max_dist2, a, g);
    }
    if (!pair) {
#pragma unroll
        for (int j = 0; j < TERMS; ++j) a[j] = 0.0;
    }
    // every thread of the workgroup: a butterfly over each wave, then ((w0 + w1) + w2) + w3
    block_sum_store<TERMS>(a, tile_sums + (size_t)blockIdx.x * TERMS);
}

// grid: tiles.  tile_sums [tiles][2 * 29] (COLS = 6) or [tiles][2 * 37] (COLS = 7): the geometric block, then the colour block
template <int COLS>
__global__ __launch_bounds__(ICP_THREADS) void icp_colour_tile_kernel(CloudSel s, long long frame, const uint8_t *__restrict__ frames, IcpCams c, int ow, unsigned grid_pixels,
                                                                      const float *__restrict__ model_depth, const float *__restrict__ model_normals,
                                                                      const uint8_t *__restrict__ model_colors, int mh, int mw, double max_dist2,
                                                                      double *__restrict__ tile_sums) {
    const unsigned q = blockIdx.x * (unsigned)ICP_TILE + threadIdx.x;
    constexpr int TERMS = icp_term_count(COLS);
    double a[2 * TERMS];
    bool pair = false, colour = false;
    if (q < grid_pixels) {
        const float *xf = s.x + frame * s.h * s.w;
        const uint8_t *mf = s.mask ? s.mask + frame * s.mask_stride : nullptr;
        IcpPair g;
        pair = icp_terms<COLS>(s, c, xf, mf, ow, q, model_depth, model_normals, mh, mw, max_dist2, a, g);
        if (pair) colour = icp_colour_terms<COLS>(c, g, frames + (size_t)frame * 3 * s.h * s.w, model_depth, model_colors, mh, mw, a + TERMS);
    }
    if (!pair) {
#pragma unroll
        for (int j = 0; j < TERMS; ++j) a[j] = 0.0;
    }
    if (!colour) {
#pragma unroll
        for (int j = TERMS; j < 2 * TERMS; ++j) a[j] = 0.0;
    }
    block_sum_store<2 * TERMS>(a, tile_sums + (size_t)blockIdx.x * (2 * TERMS));
}

struct IcpRobust {
    const float *live_normals;  // [oh][ow][3] of the frame, the camera's frame; null: no normal test
    double min_cos, huber, huber_colour;
};

// 1 inside the threshold, huber / |e| beyond it (IEEE division); +inf never weighs down
__device__ __forceinline__ double huber_weight(double e, double huber) {
    const double m = fabs(e);
    return m <= huber ? 1.0 : huber / m;
}

// whether the live normal of output pixel q, turned into the world by the estimate's R, lies within min_cos of the model's normal N
__device__ __forceinline__ bool normals_agree(const IcpCams &c, const IcpRobust &o, unsigned q, const double (&N)[3]) {
    const float *n = o.live_normals + (size_t)q * 3;
    const double nl[3] = {(double)n[0], (double)n[1], (double)n[2]};
    if (!((nl[0] * nl[0] + nl[1] * nl[1]) + nl[2] * nl[2] > 0.0)) return false;  // no live normal here; NaN fails
    double nw[3];
    rows3(c.live + 9, nl[0], nl[1], nl[2], nw);
    const double cs = (N[0] * nw[0] + N[1] * nw[1]) + N[2] * nw[2];
    return cs >= o.min_cos;
}

// grid: tiles.  tile_sums [tiles][T] or, with COLOUR, [tiles][2 * T]: icp_tile and icp_colour_tile with the normal test behind the distance
// test and Huber weights on the rows (the robust rule of include/endodav_hip.h); the pair itself comes from the same icp_pair
template <int COLS, bool COLOUR>
__global__ __launch_bounds__(ICP_THREADS) void icp_robust_tile_kernel(CloudSel s, long long frame, const uint8_t *__restrict__ frames, IcpCams c, int ow, unsigned grid_pixels,
                                                                      const float *__restrict__ model_depth, const float *__restrict__ model_normals,
                                                                      const uint8_t *__restrict__ model_colors, int mh, int mw, double max_dist2, IcpRobust o,
                                                                      double *__restrict__ tile_sums) {
    const unsigned q = blockIdx.x * (unsigned)ICP_TILE + threadIdx.x;
    constexpr int TERMS = icp_term_count(COLS), ALL = COLOUR ? 2 * TERMS : TERMS;
    double a[ALL];
    bool pair = false, colour = false;
    if (q < grid_pixels) {
        const float *xf = s.x + frame * s.h * s.w;
        const uint8_t *mf = s.mask ? s.mask + frame * s.mask_stride : nullptr;
        IcpPair g;
        pair = icp_pair<COLS>(s, c, xf, mf, ow, q, model_depth, model_normals, mh, mw, max_dist2, g);
        if (pair && o.live_normals) pair = normals_agree(c, o, q, g.N);  // q < grid_pixels: inside the map
        if (pair) {
            icp_fill<COLS, true>(g.J, g.e, huber_weight(g.e, o.huber), a);
            if constexpr (COLOUR) {
                double Jc[COLS], r;
                colour = icp_colour_pair<COLS>(c, g, frames + (size_t)frame * 3 * s.h * s.w, model_depth, model_colors, mh, mw, Jc, r);
                if (colour) icp_fill<COLS, true>(Jc, r, huber_weight(r, o.huber_colour), a + TERMS);
            }
        }
    }
    if (!pair) {
#pragma unroll
        for (int j = 0; j < TERMS; ++j) a[j] = 0.0;
    }
    if constexpr (COLOUR) {
        if (!colour) {
#pragma unroll
            for (int j = TERMS; j < 2 * TERMS; ++j) a[j] = 0.0;
        }
    }
    block_sum_store<ALL>(a, tile_sums + (size_t)blockIdx.x * ALL);
}

// grid: (tiles, count).  out [count][oh][ow][3]: the normal of every output pixel of frames first .. first + count - 1 in the camera's frame
// from central differences of the cloud's vertices; one thread a pixel, which writes its three floats whatever it finds
__global__ __launch_bounds__(ICP_THREADS) void frame_normals_kernel(CloudSel s, long long first, const double *__restrict__ cams, int cam_stride, int oh, int ow,
                                                                    unsigned grid_pixels, float *__restrict__ out) {
    const unsigned q = blockIdx.x * (unsigned)ICP_TILE + threadIdx.x;
    if (q >= grid_pixels) return;
    const long long frame = first + blockIdx.y;
    const float *xf = s.x + frame * s.h * s.w;
    const uint8_t *mf = s.mask ? s.mask + frame * s.mask_stride : nullptr;
    const double *kinv = cams + frame * cam_stride;
    int ox, oy;
    float z;
    const int p = source_pixel(s, ow, q, ox, oy);
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (ox >= 1 && ox <= ow - 2 && oy >= 1 && oy <= oh - 2 && kept(s, xf[p], mf ? mf[p] : 1u, z)) {
        // the four neighbours lie in the grid: left, right, up, down
        const unsigned nq[4] = {q - 1u, q + 1u, q - (unsigned)ow, q + (unsigned)ow};
        double V[4][3];
        bool valid = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int nx, ny;
            float nz;
            const int np = source_pixel(s, ow, nq[k], nx, ny);
            valid = kept(s, xf[np], mf ? mf[np] : 1u, nz) && valid;
            const double u = ((double)nx + 0.5) * (double)s.step, v = ((double)ny + 0.5) * (double)s.step;
#pragma unroll
            for (int i = 0; i < 3; ++i) V[k][i] = ((kinv[3 * i] * u + kinv[3 * i + 1] * v) + kinv[3 * i + 2]) * (double)nz;
        }
        if (valid) {
            double a[3], b[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) a[i] = V[1][i] - V[0][i], b[i] = V[3][i] - V[2][i];
            const double c[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};  // towards the camera
            const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
            if (len > 0.0) {  // NaN fails
#pragma unroll
                for (int i = 0; i < 3; ++i) n[i] = (float)(c[i] / len);
            }
        }
    }
    float *dst = out + ((size_t)blockIdx.y * grid_pixels + q) * 3;
    dst[0] = n[0], dst[1] = n[1], dst[2] = n[2];
}

// a workgroup per 64 values: sums[j] =(((t_0 + t_1) + t_2) + ...)[j], tile by tile.  The loads of eight tiles are issued together; the additions keep their order.
__global__ __launch_bounds__(ICP_TOTAL_THREADS) void icp_total_kernel(const double *__restrict__ tile_sums, unsigned tiles, unsigned terms, double *__restrict__ sums) {
    const unsigned j = blockIdx.x * (unsigned)ICP_TOTAL_THREADS + threadIdx.x;
    if (j >= terms) return;
    double t = tile_sums[j];
    unsigned i = 1;
    for (; i + 8 <= tiles; i += 8) {
        double v[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) v[k] = tile_sums[(size_t)(i + k) * terms + j];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) t = t + v[k];
    }
    for (; i < tiles; ++i) t = t + tile_sums[(size_t)i * terms + j];
    sums[j] = t;
}

inline bool icp_shape_ok(int h, int w, int step) { return h >= 1 && w >= 1 && step >= 1 && (long long)h * w < (1ll << 31); }

struct IcpGrid {
    int ow;
    unsigned pixels;  // oh * ow <= h * w < 2^31
    unsigned tiles;
};

inline IcpGrid icp_grid(int h, int w, int step) {
    const long long oh = ((long long)h + step - 1) / step, ow = ((long long)w + step - 1) / step;
    return {(int)ow, (unsigned)(oh * ow), (unsigned)((oh * ow + ICP_TILE - 1) / ICP_TILE)};
}

template <int COLS>
size_t icp_workspace_of(int h, int w, int step) {
    if (!icp_shape_ok(h, w, step)) return 0;
    return (size_t)icp_grid(h, w, step).tiles * icp_term_count(COLS) * sizeof(double);
}

template <int COLS>
int icp_sums_of(const CloudSel &s, long long frame, const double *live_cam, const double *model_cam, const float *model_depth, const float *model_normals, int mh, int mw,
                double max_dist2, double *sums, void *ws, size_t ws_bytes, hipStream_t stream) {
    constexpr int TERMS = icp_term_count(COLS);
    static_assert(TERMS <= ICP_TOTAL_THREADS, "one workgroup of the total");
    EDV_TRY(check_selection(s));
    EDV_CHECK(frame >= 0 && frame < s.n, "frame outside the clip");
    EDV_CHECK(live_cam && model_cam, "null cameras");
    EDV_CHECK(model_depth && model_normals && aligned_to(model_depth, 4) && aligned_to(model_normals, 4), "model depth or normals missing or not 4-byte aligned");
    EDV_CHECK(mh >= 1 && mw >= 1 && (long long)mh * mw < (1ll << 31), "mh and mw must be at least 1 and the model view below 2^31 pixels");
    EDV_CHECK(std::isfinite(max_dist2) && max_dist2 >= 0.0, "max_dist2 must be finite and >= 0");
    EDV_CHECK(sums && aligned_to(sums, 8), "sums missing or not 8-byte aligned");
    EDV_CHECK(ws && aligned_to(ws, 8) && ws_bytes >= icp_workspace_of<COLS>(s.h, s.w, s.step),
              "workspace missing, too small or not 8-byte aligned (edv_icp_workspace, edv_icp_scaled_workspace)");
    const IcpGrid g = icp_grid(s.h, s.w, s.step);
    IcpCams c;
    for (int i = 0; i < 21; ++i) c.live[i] = live_cam[i];
    for (int i = 0; i < 39; ++i) c.model[i] = model_cam[i];
    double *tile_sums = static_cast<double *>(ws);
    EDV_LAUNCH(icp_tile_kernel<COLS>, dim3(g.tiles), dim3(ICP_THREADS), 0, stream, s, frame, c, g.ow, g.pixels, model_depth, model_normals, mh, mw, max_dist2, tile_sums);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(icp_total_kernel, dim3(1), dim3(ICP_TOTAL_THREADS), 0, stream, tile_sums, g.tiles, (unsigned)TERMS, sums);
    EDV_LAUNCH_OK();
    return 0;
}

template <int COLS>
int icp_colour_sums_of(const CloudSel &s, long long frame, const uint8_t *frames, const double *live_cam, const double *model_cam, const float *model_depth,
                       const float *model_normals, const uint8_t *model_colors, int mh, int mw, double max_dist2, double *sums, void *ws, size_t ws_bytes, hipStream_t stream) {
    constexpr int TERMS = 2 * icp_term_count(COLS);
    EDV_TRY(check_selection(s));
    EDV_CHECK(frame >= 0 && frame < s.n, "frame outside the clip");
    EDV_CHECK(frames, "null frames");
    EDV_CHECK(live_cam && model_cam, "null cameras");
    EDV_CHECK(model_depth && model_normals && aligned_to(model_depth, 4) && aligned_to(model_normals, 4), "model depth or normals missing or not 4-byte aligned");
    EDV_CHECK(model_colors, "null model colours");
    EDV_CHECK(mh >= 1 && mw >= 1 && (long long)mh * mw < (1ll << 31), "mh and mw must be at least 1 and the model view below 2^31 pixels");
    EDV_CHECK(std::isfinite(max_dist2) && max_dist2 >= 0.0, "max_dist2 must be finite and >= 0");
    EDV_CHECK(sums && aligned_to(sums, 8), "sums missing or not 8-byte aligned");
    EDV_CHECK(ws && aligned_to(ws, 8) && ws_bytes >= 2 * icp_workspace_of<COLS>(s.h, s.w, s.step),
              "workspace missing, too small or not 8-byte aligned (edv_icp_colour_workspace)");
    const IcpGrid g = icp_grid(s.h, s.w, s.step);
    IcpCams c;
    for (int i = 0; i < 21; ++i) c.live[i] = live_cam[i];
    for (int i = 0; i < 39; ++i) c.model[i] = model_cam[i];
    double *tile_sums = static_cast<double *>(ws);
    EDV_LAUNCH(icp_colour_tile_kernel<COLS>, dim3(g.tiles), dim3(ICP_THREADS), 0, stream, s, frame, frames, c, g.ow, g.pixels, model_depth, model_normals, model_colors, mh, mw,
               max_dist2, tile_sums);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(icp_total_kernel, dim3((TERMS + ICP_TOTAL_THREADS - 1) / ICP_TOTAL_THREADS), dim3(ICP_TOTAL_THREADS), 0, stream, tile_sums, g.tiles, (unsigned)TERMS, sums);
    EDV_LAUNCH_OK();
    return 0;
}

template <int COLS, bool COLOUR>
int icp_robust_sums_of(const CloudSel &s, long long frame, const uint8_t *frames, const double *live_cam, const double *model_cam, const float *model_depth,
                       const float *model_normals, const uint8_t *model_colors, int mh, int mw, double max_dist2, const IcpRobust &o, double *sums, void *ws, size_t ws_bytes,
                       hipStream_t stream) {
    constexpr int TERMS = (COLOUR ? 2 : 1) * icp_term_count(COLS);
    EDV_TRY(check_selection(s));
    EDV_CHECK(frame >= 0 && frame < s.n, "frame outside the clip");
    EDV_CHECK(live_cam && model_cam, "null cameras");
    EDV_CHECK(model_depth && model_normals && aligned_to(model_depth, 4) && aligned_to(model_normals, 4), "model depth or normals missing or not 4-byte aligned");
    EDV_CHECK(mh >= 1 && mw >= 1 && (long long)mh * mw < (1ll << 31), "mh and mw must be at least 1 and the model view below 2^31 pixels");
    EDV_CHECK(std::isfinite(max_dist2) && max_dist2 >= 0.0, "max_dist2 must be finite and >= 0");
    EDV_CHECK(aligned_to(o.live_normals, 4), "live normals not 4-byte aligned");
    EDV_CHECK(std::isfinite(o.min_cos) && o.min_cos >= -1.0 && o.min_cos <= 1.0, "min_cos must be finite and in [-1, 1]");
    EDV_CHECK(o.huber > 0.0 && o.huber_colour > 0.0, "huber and huber_colour must be > 0 (+inf: no weight), not NaN");
    EDV_CHECK(sums && aligned_to(sums, 8), "sums missing or not 8-byte aligned");
    EDV_CHECK(ws && aligned_to(ws, 8) && ws_bytes >= (COLOUR ? 2 : 1) * icp_workspace_of<COLS>(s.h, s.w, s.step),
              "workspace missing, too small or not 8-byte aligned (edv_icp_robust_workspace)");
    const IcpGrid g = icp_grid(s.h, s.w, s.step);
    IcpCams c;
    for (int i = 0; i < 21; ++i) c.live[i] = live_cam[i];
    for (int i = 0; i < 39; ++i) c.model[i] = model_cam[i];
    double *tile_sums = static_cast<double *>(ws);
    EDV_LAUNCH((icp_robust_tile_kernel<COLS, COLOUR>), dim3(g.tiles), dim3(ICP_THREADS), 0, stream, s, frame, frames, c, g.ow, g.pixels, model_depth, model_normals, model_colors,
               mh, mw, max_dist2, o, tile_sums);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(icp_total_kernel, dim3((TERMS + ICP_TOTAL_THREADS - 1) / ICP_TOTAL_THREADS), dim3(ICP_TOTAL_THREADS), 0, stream, tile_sums, g.tiles, (unsigned)TERMS, sums);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace

int frame_normals(const CloudSel &s, const double *cams, int cam_stride, long long first, long long count, float *normals, hipStream_t stream) {
    EDV_TRY(check_selection(s));
    EDV_CHECK(cams && aligned_to(cams, 8), "cameras missing or not 8-byte aligned");
    EDV_CHECK(cam_stride == 0 || cam_stride == 21, "cam_stride: 0 (one camera for all frames) or 21 (a camera per frame)");
    EDV_CHECK(first >= 0 && count >= 1 && first < s.n && count <= s.n - first, "first and count must name frames of the clip, at least one");
    EDV_CHECK(normals && aligned_to(normals, 4), "normals missing or not 4-byte aligned");
    const IcpGrid g = icp_grid(s.h, s.w, s.step);
    const int oh = (int)(g.pixels / (unsigned)g.ow);
    EDV_LAUNCH(frame_normals_kernel, dim3(g.tiles, (unsigned)count), dim3(ICP_THREADS), 0, stream, s, first, cams, cam_stride, oh, g.ow, g.pixels, normals);
    EDV_LAUNCH_OK();
    return 0;
}

size_t icp_robust_workspace(int h, int w, int step, int cols, int colour) {
    if (colour != 0 && colour != 1) return 0;
    return (size_t)(colour ? 2 : 1) * (cols == 6 ? icp_workspace_of<6>(h, w, step) : cols == 7 ? icp_workspace_of<7>(h, w, step) : 0);
}

int icp_robust_sums(const CloudSel &s, long long frame, const uint8_t *frames, const double *live_cam, const double *model_cam, const float *model_depth,
                    const float *model_normals, const uint8_t *model_colors, int mh, int mw, double max_dist2, int cols, const float *live_normals, double min_cos, double huber,
                    double huber_colour, double *sums, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(cols == 6 || cols == 7, "cols: 6, or 7 with the scale");
    const IcpRobust o{live_normals, min_cos, huber, huber_colour};
    const bool colour = frames && model_colors;  // the colour block: exactly when both are given
#define EDV_ROBUST(COLS, COLOUR) \
    icp_robust_sums_of<COLS, COLOUR>(s, frame, frames, live_cam, model_cam, model_depth, model_normals, model_colors, mh, mw, max_dist2, o, sums, ws, ws_bytes, stream)
    if (cols == 6) return colour ? EDV_ROBUST(6, true) : EDV_ROBUST(6, false);
    return colour ? EDV_ROBUST(7, true) : EDV_ROBUST(7, false);
#undef EDV_ROBUST
}

int icp_tile_pixels() { return ICP_TILE; }

size_t icp_workspace(int h, int w, int step) { return icp_workspace_of<6>(h, w, step); }
size_t icp_scaled_workspace(int h, int w, int step) { return icp_workspace_of<7>(h, w, step); }

int icp_sums(const CloudSel &s, long long frame, const double *live_cam, const double *model_cam, const float *model_depth, const float *model_normals, int mh, int mw,
             double max_dist2, double *sums, void *ws, size_t ws_bytes, hipStream_t stream) {
    return icp_sums_of<6>(s, frame, live_cam, model_cam, model_depth, model_normals, mh, mw, max_dist2, sums, ws, ws_bytes, stream);
}

int icp_scaled_sums(const CloudSel &s, long long frame, const double *live_cam, const double *model_cam, const float *model_depth, const float *model_normals, int mh,
                    int mw, double max_dist2, double *sums, void *ws, size_t ws_bytes, hipStream_t stream) {
    return icp_sums_of<7>(s, frame, live_cam, model_cam, model_depth, model_normals, mh, mw, max_dist2, sums, ws, ws_bytes, stream);
}

size_t icp_colour_workspace(int h, int w, int step, int cols) {
    return cols == 6 ? 2 * icp_workspace_of<6>(h, w, step) : cols == 7 ? 2 * icp_workspace_of<7>(h, w, step) : 0;
}

int icp_colour_sums(const CloudSel &s, long long frame, const uint8_t *frames, const double *live_cam, const double *model_cam, const float *model_depth,
                    const float *model_normals, const uint8_t *model_colors, int mh, int mw, double max_dist2, int cols, double *sums, void *ws, size_t ws_bytes,
                    hipStream_t stream) {
    EDV_CHECK(cols == 6 || cols == 7, "cols: 6, or 7 with the scale");
    if (cols == 6) return icp_colour_sums_of<6>(s, frame, frames, live_cam, model_cam, model_depth, model_normals, model_colors, mh, mw, max_dist2, sums, ws, ws_bytes, stream);
    return icp_colour_sums_of<7>(s, frame, frames, live_cam, model_cam, model_depth, model_normals, model_colors, mh, mw, max_dist2, sums, ws, ws_bytes, stream);
}

}  // namespace edv
