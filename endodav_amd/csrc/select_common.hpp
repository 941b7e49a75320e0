// What metrics.hip and render.hip share (stitch.hip takes load_group): the exact radix select behind the masked median and the two order
// statistics per frame.  It works on the order-preserving integer image of the float bits in four 8-bit histogram passes, LDS counters per
// block flushed with 64-bit integer atomics into one SelState per batch item.  Both statistics are followed at once, so two ranks cost no extra
// pass, and the only atomics are integer ones: the same input gives the same bits on every call.  A select is, per pass, one launch of
// select_hist_kernel over the whole batch and one step kernel of the caller's that narrows with select_narrow and clears the counters.
// Everything here is internal to the translation unit that includes it.
#pragma once
#include "ops.hpp"

namespace edv {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u64 = unsigned long long;

// zeroed by a memset before the first pass: both prefixes empty, all counters clear
struct alignas(16) SelState {
    u64 hist[2][256];
    u64 rank[2];
    u64 total;
    unsigned prefix[2];
};
static_assert(sizeof(SelState) == 4128);  // edv_render_workspace and the layout of the metrics workspace

__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool in_gate(float g, float lo, float hi) { return lo < g && g < hi; }  // NaN fails both, as on the host

// group g of x: VW == 4 is one 16-byte load (x 16-byte aligned), VW == 1 one element
template <int VW>
__device__ __forceinline__ void load_group(const float *x, long long g, float (&v)[VW]) {
    if constexpr (VW == 4) {
        const f32x4 a = reinterpret_cast<const f32x4 *>(x)[g];
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
        v[0] = x[g];
    }
}

// one pass, grid (blocks, batch): of batch item blockIdx.y's elements x[blockIdx.y * elems ..) whose key starts with prefix[s], count the next
// 8 bits into states[blockIdx.y].  GATED: only the elements with lo < gate < hi count (gate, lo and hi are not read otherwise); x may alias
// gate, so no pointer is __restrict__.
template <int VW, bool GATED>
__global__ __launch_bounds__(256) void select_hist_kernel(const float *x, const float *gate, long long elems, float lo, float hi, int shift, SelState *states) {
    __shared__ unsigned h[2][256];
    h[0][threadIdx.x] = 0, h[1][threadIdx.x] = 0;
    __syncthreads();
    SelState *s = states + blockIdx.y;
    const float *xb = x + (long long)blockIdx.y * elems;
    const unsigned hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    const unsigned p0 = s->prefix[0], p1 = s->prefix[1];
    const bool two = p0 != p1;
    const long long groups = elems / VW;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        float xv[VW], gv[VW];
        load_group<VW>(xb, g, xv);
        if constexpr (GATED) load_group<VW>(gate + (long long)blockIdx.y * elems, g, gv);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            if constexpr (GATED)
                if (!in_gate(gv[j], lo, hi)) continue;
            const unsigned k = order_key(xv[j]);
            const unsigned bin = (k >> shift) & 255u;
            if ((k & hmask) == p0) atomicAdd(&h[0][bin], 1u);
            if (two && (k & hmask) == p1) atomicAdd(&h[1][bin], 1u);
        }
    }
    __syncthreads();
    if (h[0][threadIdx.x]) atomicAdd(&s->hist[0][threadIdx.x], (u64)h[0][threadIdx.x]);
    if (two && h[1][threadIdx.x]) atomicAdd(&s->hist[1][threadIdx.x], (u64)h[1][threadIdx.x]);
}

// one thread: narrows both statistics by the 8 bits just counted: the bin that holds rank[sel] extends prefix[sel], and rank[sel] becomes the
// rank inside that bin.  While the prefixes agree, both statistics read the one histogram that was counted.
__device__ __forceinline__ void select_narrow(SelState *s, int shift) {
    const bool two = s->prefix[0] != s->prefix[1];
    unsigned np[2];
    u64 nr[2];
    for (int sel = 0; sel < 2; ++sel) {
        const u64 *h = s->hist[two ? sel : 0];
        u64 r = s->rank[sel];
        int b = 0;
        while (b < 255 && r >= h[b]) r -= h[b], ++b;
        np[sel] = s->prefix[sel] | ((unsigned)b << shift);
        nr[sel] = r;
    }
    s->prefix[0] = np[0], s->prefix[1] = np[1];
    s->rank[0] = nr[0], s->rank[1] = nr[1];
}

}  // namespace
}  // namespace edv
