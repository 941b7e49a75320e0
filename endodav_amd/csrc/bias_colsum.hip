// Batched column sums for the bias gradients (bias="all", endodav/layers.py:5-34): every job reduces the rows of one [M, N] gradient
// (row selection through a RowMap, any N >= 1) to a [N] vector, optionally scaled per column (LayerScale gamma).
//
//   stage 1  colsum_stage1   one launch for up to CS_MAX_JOBS jobs: job j is cut into `parts` row chunks x ceil(N / CW) column blocks,
//                            one workgroup each.  CW = the next power of two >= N (at most 256); the 256 / CW row lanes of a workgroup
//                            walk the chunk's rows with stride 256 / CW (four independent accumulators each), then the row lanes of every
//                            column are added in pairs in fp64 (a halving tree in LDS), rounded once, and one partial row goes into the
//                            job's slab region [parts, N].
//   stage 2  colsum_stage2   one launch for up to CS_MAX_OUTS outputs: output o adds `rows` consecutive partial rows of the slab in index
//                            order (several jobs that feed one tensor -- pretrained.norm.bias is reached from four taps -- lie back to
//                            back), multiplies by scale[n] and writes or accumulates dst[n].
//
// No float atomics: every sum has a fixed order, so the result is bit-reproducible run to run.  Stage 1 runs where the gradients are
// live (they sit in reused scratch); stage 2 may run much later, once, for everything the slab holds.
#include <vector>

#include "common.hpp"
#include "ops.hpp"

namespace edv {
namespace {

__device__ __forceinline__ int find_item(const int *begin, int n, int bid) {
    int j = 0;
    while (j + 1 < n && bid >= begin[j + 1]) ++j;
    return j;
}

struct Stage1Args {
    ColsumJob job[CS_MAX_JOBS];
    int wg_begin[CS_MAX_JOBS];
    int n;
};
struct Stage2Args {
    ColsumOut out[CS_MAX_OUTS];
    int wg_begin[CS_MAX_OUTS];
    int n;
};

__global__ __launch_bounds__(256) void colsum_stage1(const Stage1Args a) {
    __shared__ double red[256];
    const int j = find_item(a.wg_begin, a.n, blockIdx.x);
    const ColsumJob &jb = a.job[j];
    const int local = blockIdx.x - a.wg_begin[j];
    const int cw = 1 << jb.cw_log, rl_n = 256 >> jb.cw_log;
    const int col_blocks = (jb.N + cw - 1) / cw;
    const int part = local / col_blocks, cb = local - part * col_blocks;
    const int cc = threadIdx.x & (cw - 1), rl = threadIdx.x >> jb.cw_log;
    const int col = cb * cw + cc;
    const long long r0 = (long long)part * jb.chunk;
    const long long r1 = r0 + jb.chunk < jb.rows ? r0 + jb.chunk : jb.rows;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (col < jb.N) {
        const float *src = jb.src + col;
        long long r = r0 + rl;
        for (; r + 3 * rl_n < r1; r += 4 * rl_n) {
            s0 += src[jb.map(r) * jb.ld];
            s1 += src[jb.map(r + rl_n) * jb.ld];
            s2 += src[jb.map(r + 2 * rl_n) * jb.ld];
            s3 += src[jb.map(r + 3 * rl_n) * jb.ld];
        }
        for (; r < r1; r += rl_n) s0 += src[jb.map(r) * jb.ld];
    }
    red[threadIdx.x] = ((double)s0 + (double)s1) + ((double)s2 + (double)s3);
    __syncthreads();
    // The row lanes of a column (threads cc, cc + cw, ...) are joined in pairs, halving, in fp64, and rounded to fp32 once.  One lane adding
    // the other 255 in fp32 in sequence (N = 1) lost 6 u of sum |P| on rows with a mean, seventeen times torch's own sum; an fp32 tree still 1.5 u.
    for (int h = rl_n >> 1; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h * cw) red[threadIdx.x] += red[threadIdx.x + h * cw];
        __syncthreads();
    }
    if (rl == 0 && col < jb.N) jb.slab[(long long)part * jb.N + col] = (float)red[cc];
}

__global__ __launch_bounds__(256) void colsum_stage2(const Stage2Args a) {
    const int o = find_item(a.wg_begin, a.n, blockIdx.x);
    const ColsumOut &ot = a.out[o];
    const int n = (blockIdx.x - a.wg_begin[o]) * 256 + threadIdx.x;
    if (n >= ot.N) return;
    float s = 0.f;
    for (int q = 0; q < ot.rows; ++q) s += ot.slab[(long long)q * ot.N + n];
    if (ot.scale) s *= ot.scale[n];
    ot.dst[n] = ot.accumulate ? ot.dst[n] + s : s;
}

}  // namespace

ColsumJob colsum_job(const float *src, long long ld, long long rows, RowMap map, int N) {
    ColsumJob j;
    j.src = src; j.ld = ld; j.rows = rows; j.map = map; j.N = N;
    // about 64 K elements per workgroup, at most CS_MAX_PARTS partial rows
    long long parts = (rows * (long long)N + 65535) / 65536;
    parts = parts < 1 ? 1 : (parts > CS_MAX_PARTS ? CS_MAX_PARTS : parts);
    if (parts > rows) parts = rows > 0 ? rows : 1;
    j.chunk = (rows + parts - 1) / parts;
    if (j.chunk < 1) j.chunk = 1;
    j.parts = (int)((rows + j.chunk - 1) / j.chunk);
    if (j.parts < 1) j.parts = 1;
    int lg = 0;
    while ((1 << lg) < N && lg < 8) ++lg;
    j.cw_log = lg;
    return j;
}

int colsum_stage1_launch(const ColsumJob *jobs, int n, hipStream_t st) {
    for (int b = 0; b < n; b += CS_MAX_JOBS) {
        Stage1Args a{};
        a.n = n - b < CS_MAX_JOBS ? n - b : CS_MAX_JOBS;
        long long wgs = 0;
        for (int k = 0; k < a.n; ++k) {
            const ColsumJob &jb = jobs[b + k];
            EDV_CHECK(jb.N >= 1 && jb.rows >= 1 && jb.src && jb.slab && jb.ld >= jb.N, "colsum job: bad shape");
            a.job[k] = jb;
            a.wg_begin[k] = (int)wgs;
            const int cw = 1 << jb.cw_log;
            wgs += (long long)jb.parts * ((jb.N + cw - 1) / cw);
        }
        EDV_CHECK(wgs < (1ll << 31), "colsum: too many workgroups");
        EDV_LAUNCH(colsum_stage1, dim3((unsigned)wgs), dim3(256), 0, st, a);
        EDV_LAUNCH_OK();
    }
    return 0;
}

int colsum_stage2_launch(const ColsumOut *outs, int n, hipStream_t st) {
    for (int b = 0; b < n; b += CS_MAX_OUTS) {
        Stage2Args a{};
        a.n = n - b < CS_MAX_OUTS ? n - b : CS_MAX_OUTS;
        int wgs = 0;
        for (int k = 0; k < a.n; ++k) {
            const ColsumOut &ot = outs[b + k];
            EDV_CHECK(ot.N >= 1 && ot.rows >= 1 && ot.slab && ot.dst, "colsum output: bad shape");
            a.out[k] = ot;
            a.wg_begin[k] = wgs;
            wgs += (ot.N + 255) / 256;
        }
        EDV_LAUNCH(colsum_stage2, dim3((unsigned)wgs), dim3(256), 0, st, a);
        EDV_LAUNCH_OK();
    }
    return 0;
}

size_t colsum_batch_workspace(int n, const long long *rows, const int *cols) {
    size_t f = 0;
    for (int k = 0; k < n; ++k) {
        const ColsumJob j = colsum_job(nullptr, cols[k], rows[k], identity_map(), cols[k]);
        f += (size_t)j.parts * cols[k];
    }
    return f;
}

int colsum_batch(int n, const float *const *src, const long long *ld, const long long *rows, const RowMap *maps, const int *cols, const float *const *scale,
                 float *const *dst, const int *accumulate, float *ws, size_t ws_floats, hipStream_t st) {
    std::vector<ColsumJob> jobs(n);
    std::vector<ColsumOut> outs(n);
    size_t off = 0;
    for (int k = 0; k < n; ++k) {
        jobs[k] = colsum_job(src[k], ld[k], rows[k], maps[k], cols[k]);
        jobs[k].slab = ws + off;
        const size_t need = (size_t)jobs[k].parts * cols[k];
        EDV_CHECK(off + need <= ws_floats, "colsum_batch workspace too small (colsum_batch_workspace)");
        outs[k] = ColsumOut{ws + off, jobs[k].parts, cols[k], scale ? scale[k] : nullptr, dst[k], accumulate && accumulate[k] ? 1 : 0};
        off += need;
    }
    EDV_TRY(colsum_stage1_launch(jobs.data(), n, st));
    return colsum_stage2_launch(outs.data(), n, st);
}

}  // namespace edv
