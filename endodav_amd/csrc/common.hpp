// Shared device/host helpers for libendodav_hip (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace edv {

// thread-local error text behind edv_last_error()
void set_error(const std::string &msg);
const char *get_error();

#define EDV_CHECK(cond, msg)                                                     \
    do {                                                                         \
        if (!(cond)) {                                                           \
            ::edv::set_error(std::string(__func__) + ": " + (msg));              \
            return 1;                                                            \
        }                                                                        \
    } while (0)

#define EDV_HIP(expr)                                                            \
    do {                                                                         \
        hipError_t e_ = (expr);                                                  \
        if (e_ != hipSuccess) {                                                  \
            ::edv::set_error(std::string(__func__) + ": " #expr ": " + hipGetErrorString(e_)); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

#define EDV_TRY(expr)                                                            \
    do {                                                                         \
        int r_ = (expr);                                                         \
        if (r_ != 0) return r_;                                                  \
    } while (0)

// after a kernel launch
#define EDV_LAUNCH_OK() EDV_HIP(hipGetLastError())

constexpr int WAVE = 64;

// Kernel timing for edv_profile_enable (round 3).  While the engine has a Bracket open on this thread, every launch carries the bracket's event
// pair INSIDE its dispatch (hipExtLaunchKernelGGL: the start event is stamped when the kernel starts, the stop event when it ends), so a bracket
// measures the kernel(s) alone -- the same interval rocprofv3's kernel trace reports -- instead of "the in-order gap before the launch + the kernel"
// that hipEventRecord before / after the launch measures (12 us against 8 us for a LayerNorm launch in round 2).  A bracket around several launches
// spans from the first kernel's start to the last one's end.
struct LaunchTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    bool started = false;
};
extern thread_local LaunchTimer *g_launch_timer;
#define EDV_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                                                   \
    do {                                                                                                                                      \
        ::edv::LaunchTimer *lt_ = ::edv::g_launch_timer;                                                                                      \
        if (lt_) {                                                                                                                            \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, lt_->started ? nullptr : lt_->start, lt_->stop, 0, __VA_ARGS__);        \
            lt_->started = true;                                                                                                              \
        } else {                                                                                                                              \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                                              \
        }                                                                                                                                     \
    } while (0)

// Launch geometry that depends on the DEVICE (resident workgroups of a persistent kernel = CUs x occupancy) is cached per HIP device, not per
// process: nn.DataParallel drives several devices from one process, and a partitioned or mixed node may give them different CU counts.
// `query` runs on the current device; 0 = the query failed (not cached).
constexpr int EDV_MAX_DEVICES = 64;
struct DeviceSlotCache {
    std::atomic<int> v[EDV_MAX_DEVICES];  // static storage: zero-initialised
    template <class Q>
    int get(Q query) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EDV_MAX_DEVICES) return query();
        int s = v[dev].load(std::memory_order_relaxed);
        if (s == 0) {
            s = query();
            v[dev].store(s, std::memory_order_relaxed);
        }
        return s;
    }
};
// Resident workgroups of a persistent kernel on the current device: CUs x workgroups per CU, cached in `cache`; 0 = a query failed.  Per CU it is
// what the occupancy API answers for `threads` threads and `lds_bytes` of dynamic LDS (opted into first when not zero; `sibling`, an
// instantiation launched with the same LDS size, gets the attribute too), at most `cap` (0: no cap -- the API over-reports where LDS bounds the
// residency, and a persistent grid beyond what is really resident starts its surplus workgroups only when others finish), unless the environment
// variable `override_env` gives a positive number.  EDV_DEBUG_SLOTS prints the result under `label` (null: silent).
inline int resident_workgroups(DeviceSlotCache &cache, const void *kernel, int threads, size_t lds_bytes, int cap, const char *override_env, const char *label,
                               const void *sibling = nullptr) {
    return cache.get([&] {
        int dev = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        for (const void *k : {kernel, sibling})
            if (k && lds_bytes && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) return 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes) != hipSuccess) return 0;
        if (cap > 0 && per_cu > cap) per_cu = cap;
        if (const char *e = override_env ? getenv(override_env) : nullptr) per_cu = atoi(e) > 0 ? atoi(e) : per_cu;
        if (label && getenv("EDV_DEBUG_SLOTS")) fprintf(stderr, "%s: %d CUs x %d resident workgroups\n", label, cus, per_cu);
        return cus * per_cu;
    });
}

// Row remap: logical row m of a [frames * period] matrix lives at physical row
//   (m / period) * stride + offset + inner * (m % period).
// period == 0 means identity.  Used to skip the cls row of each frame's token block, to
// broadcast the position table over frames (stride 0), to broadcast one row per frame over
// that frame's rows (inner 0) and to address sub-ranges in place.
struct RowMap {
    int period, stride, offset;
    int inner = 1;
    __host__ __device__ inline long long operator()(long long m) const {
        if (period == 0) return m;
        long long f = m / period;
        return f * stride + offset + inner * (m - f * period);
    }
};
inline RowMap identity_map() { return RowMap{0, 0, 0}; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The sum over a block of 256 threads of Q per-thread partials -> dst[0..Q), thread q < Q storing sum q: a wave butterfly, then the four per-wave
// sums r0..r3.  The two helpers add them in DIFFERENT orders, each the one its callers' results were pinned with: the fp32 one in pairs,
// (r0 + r1) + (r2 + r3); the fp64 one in wave order, ((r0 + r1) + r2) + r3.  dst may be LDS: the caller then syncs before it reads.
template <int Q>
__device__ __forceinline__ void block_sum_pairs_store(const float (&a)[Q], float *dst) {
    __shared__ float red[4][Q];
    float s[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = wave_sum(a[q]);
    if ((threadIdx.x & 63) == 0) {  // the Q stores under one test: a test per store costs each caller a few instructions per partial
#pragma unroll
        for (int q = 0; q < Q; ++q) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if ((int)threadIdx.x < Q) dst[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
template <int Q>
__device__ __forceinline__ void block_sum_store(double (&a)[Q], double *dst) {
    __shared__ double red[4][Q];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        a[q] = wave_sum_f64(a[q]);
        if (lane == 0) red[wave][q] = a[q];
    }
    __syncthreads();
    if ((int)threadIdx.x < Q) dst[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// exact-erf GELU, the nn.GELU() / F.gelu default used everywhere in the reference
// (layers/block.py:58, motion_module/attention.py:378)
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// an integer A/B knob from the environment (callers read it once: a function-local static)
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// blocks of 256 threads for a grid-stride loop over `groups` items: one item a thread, at least one block and at most `cap`
inline int blocks_for(long long groups, int cap) { return (int)std::max<long long>(1, std::min<long long>((groups + 255) / 256, cap)); }

}  // namespace edv
