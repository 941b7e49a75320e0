// Shared by the engine's translation units (internal, not installed): the context, the buffer pools, the profiling brackets and `Run`, the
// state and op wrappers every phase of a forward / backward enqueues through.  Where things live:
//   engine_prepare.hip   weight folding and packing (edv_prepare, edv_refresh_lora), the bf16x6 planes, the backward's transposed weights
//   engine_forward.hip   encoder, DPT head with its two-stream schedule, output heads
//   engine_backward.hip  the adjoints of the above, bias-gradient batching, LoRA / SSB factor gradients
//   engine.hip           the extern "C" entry points
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/endodav_hip.h"
#include "ops.hpp"

namespace edv {

struct Param {
    const float *p;
    std::vector<int64_t> shape;
    long long numel() const {
        long long n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};
struct Buf {
    float *p = nullptr;
    size_t cap = 0;  // floats
};

// kernel classes for the optional HIP-event bracketing (edv_profile_enable / edv_profile_read)
// KC_LINEAR_ENC: the F.linear launches of the encoder blocks (qkv, proj, fc1, fc2: 96 % of the dense-GEMM work), a sub-class bracketed
// with the same mask bit as KC_LINEAR and reported separately (the head's small GEMMs are HBM- and launch-bound, not MFMA-bound)
constexpr int PE_K = 608;  // patch-embed im2col width 3 * 14 * 14 = 588, padded to a multiple of 32

// KC_GROUPNORM .. KC_PATCHIFY: the HBM-bound kernels of the forward, each with its algorithmic bytes (tensor in + tensor out, once) for
// bench.py's roofline_hbm object
enum { KC_LINEAR = 0, KC_CONV3 = 1, KC_ATTN_SPATIAL = 2, KC_ATTN_TEMPORAL = 3, KC_NORM = 4, KC_OTHER = 5, KC_LINEAR_ENC = 6, KC_GROUPNORM = 7,
       KC_BILINEAR = 8, KC_GEGLU = 9, KC_DOT = 10, KC_PATCHIFY = 11, KC_ATTN_SPATIAL_BWD = 12, KC_COUNT = 13 };
struct EvPool {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
};
}  // namespace edv
using namespace edv;

struct edv_ctx {
    edv_config cfg{};
    unsigned prof_mask = 0;
    EvPool prof[KC_COUNT];
    double prof_flops[KC_COUNT] = {};  // algorithmic work of the bracketed launches (edv_profile_work)
    double prof_bytes[KC_COUNT] = {};
    int enc_streams = 0;                      // 0: automatic (2 for small clips); n >= 1: that many frame groups on internal streams
    int enc_streams_initial = 0;              // what EDV_ENC_STREAMS asked for at edv_create (edv_set_encoder_streams(-1) restores it)
    hipStream_t sub[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_x[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // cross-stream edges of the head (r3, r1r2, u3, u2, u1)
    std::unordered_map<std::string, Param> params;
    std::unordered_map<std::string, Buf> packed;  // derived weights, owned
    std::unordered_map<std::string, Buf> ws;      // activations, owned
    bool prepared = false;
    int products = EDV_PRODUCTS_F32;  // arithmetic of the encoder's linears in inference (edv_set_products)
    std::unordered_map<const float *, const void *> x6;  // effective weight of an encoder linear -> its bf16 planes (gemm_x6.hip), owned by `packed`
    const float *skws_zeroed = nullptr;  // stream-K workspace whose arrival counters have been zeroed (gemm_dma.hip)
    bool capture = false;
    bool train = false;           // forward keeps the activations the backward needs (edv_set_train)
    bool train_prepared = false;  // transposed / flipped weights of the input-gradient GEMMs are current
    bool have_saved = false;      // a training forward has run since the last backward
    bool grad_encoder = true;     // which factor gradients the caller wants (edv_set_grad_scope): the trainer alternates
    bool grad_temporal = true;    // spatial and temporal tuning phases (trainer_end_to_end_video.py:327-339)
    bool grad_res = false;        // parameters of the residual bottleneck blocks (residual_*, trainable by default in the reference)
    bool grad_head = false;       // weight / bias gradients of the output-head convolutions (conv_depth_*, or scratch.output_conv* with --train_output_conv)
    bool grad_enc_bias = false;   // every pretrained.*bias (edv_set_bias_grads; bias="all" of endodav/layers.py:5-34)
    bool grad_head_bias = false;  // every head.*bias the forward reaches
    std::unordered_map<std::string, Buf> grads;  // gradients of the trainable parameters, owned
    // Caller-owned flat gradient buffer (edv_grad_bind_flat): a gradient whose name is listed here is written straight into its slice
    // of that buffer instead of into `grads` -- the host's .grad tensors are views of it and the data-parallel all-reduce runs on
    // it in place (trainer_end_to_end_video.py:269-271's reduce), with no per-tensor copy on either side.
    struct FlatSlot {
        float *p;
        size_t numel;
        bool written;
    };
    std::unordered_map<std::string, FlatSlot> flat;
    int device = 0;                 // HIP device the context was created on (edv_destroy frees there)
    uint64_t generation = 0;        // counts training forwards; the kept activations belong to forward number `saved_generation`
    uint64_t saved_generation = 0;
    int launches = 0;
    size_t bytes = 0;
    // geometry of the last forward (for edv_stage_copy)
    int F = 0, T = 0, ph = 0, pw = 0, ntok = 0;
    std::unordered_map<std::string, std::pair<const float *, size_t>> stages;
};

namespace edv {

inline int alloc_buf(edv_ctx *c, std::unordered_map<std::string, Buf> &pool, const std::string &name, size_t n, hipStream_t st, float **out) {
    Buf &b = pool[name];
    if (b.cap < n) {
        if (b.p) {
            EDV_HIP(hipStreamSynchronize(st));  // kernels in flight may still read the old block
            EDV_HIP(hipFree(b.p));
            c->bytes -= b.cap * sizeof(float);
            b.p = nullptr;
            b.cap = 0;
        }
        void *p = nullptr;
        EDV_HIP(hipMalloc(&p, n * sizeof(float)));
        b.p = (float *)p;
        b.cap = n;
        c->bytes += n * sizeof(float);
    }
    *out = b.p;
    return 0;
}

// Times the launch(es) made while it is alive when their class is being profiled: the event pair travels inside the dispatches (EDV_LAUNCH,
// common.hpp), so the pair measures the kernels alone, as rocprofv3's kernel trace does.  Brackets nest like scopes (an inner one times its own launches).
struct Bracket {
    LaunchTimer timer;
    LaunchTimer *prev = nullptr;
    bool on = false;
    hipStream_t st;
    Bracket(edv_ctx *c, int cls, hipStream_t s) : st(s) {
        if (!(c->prof_mask & (1u << (cls == KC_LINEAR_ENC ? KC_LINEAR : cls)))) return;  // the sub-class shares its parent's mask bit
        EvPool &p = c->prof[cls];
        if (p.used == p.ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            p.ev.emplace_back(a, b);
        }
        auto &pr = p.ev[p.used++];
        timer.start = pr.first;
        timer.stop = pr.second;
        prev = g_launch_timer;
        g_launch_timer = &timer;
        on = true;
    }
    ~Bracket() {
        if (!on) return;
        g_launch_timer = prev;
        if (!timer.started) {  // nothing was launched inside: keep the pair well-formed (zero-length interval on the stream)
            (void)hipEventRecord(timer.start, st);
            (void)hipEventRecord(timer.stop, st);
        }
    }
};

// Bracket for a bandwidth-bound launch: also books its algorithmic bytes (every tensor it reads or writes, once)
struct HbmScope {
    Bracket b;
    HbmScope(edv_ctx *c, int cls, hipStream_t st, double bytes) : b(c, cls, st) {
        if (c->prof_mask & (1u << cls)) c->prof_bytes[cls] += bytes;
    }
};

// An on-by-default switch for A/B runs: on unless the variable is set to 0.  Call sites keep the answer in a static (read once per process).
inline bool env_flag(const char *name, bool dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

struct Run {
    edv_ctx *c;
    hipStream_t st;
    const edv_config &cfg;
    int D, depth, heads, Fe;
    int F = 0, B = 0, T = 0, ph = 0, pw = 0, P0 = 0, ntok = 0, c0 = 0;
    int h0 = 0, w0 = 0, h1 = 0, w1 = 0, h2 = 0, w2 = 0, h3 = 0, w3 = 0, h4 = 0, w4 = 0;  // path_1's map (8x the patch grid) .. layer4_rn's (half of it)
    int Fh = 0;                                                                          // channels inside an output head

    Run(edv_ctx *ctx, hipStream_t s) : c(ctx), st(s), cfg(ctx->cfg) {
        D = cfg.embed_dim;
        depth = cfg.depth;
        heads = cfg.num_heads;
        Fe = cfg.features;
    }
    // The clip and pyramid geometry, for the forward and the backward alike (F also counts one frame group while the encoder is forked)
    void set_geometry(int B_, int T_) {
        B = B_; T = T_; F = B * T;
        ph = cfg.image_h / 14; pw = cfg.image_w / 14; P0 = ph * pw;
        c0 = cfg.include_cls_token ? 1 : 0;
        ntok = P0 + c0;
        h0 = 8 * ph; w0 = 8 * pw; h1 = 4 * ph; w1 = 4 * pw; h2 = 2 * ph; w2 = 2 * pw; h3 = ph; w3 = pw; h4 = (ph - 1) / 2 + 1; w4 = (pw - 1) / 2 + 1;
        Fh = Fe / 2;
    }

    // ---- lookup helpers -------------------------------------------------------------------
    int param(const std::string &name, const float **out, int ndim_expect = -1) {
        auto it = c->params.find(name);
        EDV_CHECK(it != c->params.end(), "parameter not bound: " + name);
        if (ndim_expect >= 0) EDV_CHECK((int)it->second.shape.size() == ndim_expect, "unexpected rank for " + name);
        *out = it->second.p;
        return 0;
    }
    bool has(const std::string &name) const { return c->params.count(name) != 0; }
    int packedw(const std::string &name, const float **out) {
        auto it = c->packed.find(name);
        EDV_CHECK(it != c->packed.end() && it->second.p, "packed weight missing (edv_prepare not run?): " + name);
        *out = it->second.p;
        return 0;
    }
    int wsbuf(const std::string &name, size_t n, float **out) { return alloc_buf(c, c->ws, name, n, st, out); }
    int pk(const std::string &name, size_t n, float **out) { return alloc_buf(c, c->packed, name, n, st, out); }
    // bias of a ResidualConvUnit convolution: with use_bn the one edv_prepare folded the BatchNorm into
    int rcu_bias(const std::string &conv, const float **out) {
        if (cfg.use_bn) return packedw(conv + ".bias", out);
        return param(conv + ".bias", out);
    }

    // ---- op wrappers ----------------------------------------------------------------------
    bool in_encoder = false;  // linear() is being called from the encoder block loop (profiling sub-class KC_LINEAR_ENC)
    float *skws = nullptr;  // stream-K split workspace of the stream this Run is enqueueing on
    size_t skws_floats = 0;
    int gemm_ws(GemmDesc &g) {
        g.ws = skws;
        g.ws_floats = skws_floats;
        return gemm(g, st);
    }
    int linear(const float *A, long long M, int K, const float *W, int N, const float *bias, float *C, int act = ACT_NONE,
               const float *gamma = nullptr, const float *R1 = nullptr) {
        GemmDesc g;
        g.A = A; g.lda = K; g.W = W; g.ldw = K; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K;
        g.bias = bias; g.act = act; g.gamma = gamma; g.R1 = R1; g.ldr1 = N;
        if (in_encoder && !c->train && c->products == EDV_PRODUCTS_BF16X6) {
            auto it = c->x6.find(W);
            if (it != c->x6.end()) g.Wx6 = it->second;
        }
        c->launches++;
        const int cls = in_encoder ? KC_LINEAR_ENC : KC_LINEAR;
        if (c->prof_mask & (1u << KC_LINEAR)) {  // 2 M N K; A, W read once, C written once (+ the residual read)
            c->prof_flops[cls] += 2.0 * (double)M * N * K;
            c->prof_bytes[cls] += 4.0 * ((double)M * K + (double)N * K + (double)M * N * (R1 ? 2 : 1));
        }
        Bracket b_(c, cls, st);
        return gemm_ws(g);
    }
    int conv3(const float *x, int H, int W, int Cin, const float *wp, const float *bias, int Cout, int stride, float *y, bool pre_relu,
              int act = ACT_NONE, const float *R1 = nullptr, const float *R2 = nullptr) {
        GemmDesc g;
        const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
        g.A = x; g.W = wp; g.ldw = 9 * Cin; g.C = y; g.ldc = Cout; g.M = (long long)F * OH * OW; g.N = Cout; g.K = 9 * Cin;
        g.bias = bias; g.act = act; g.R1 = R1; g.ldr1 = Cout; g.R2 = R2; g.ldr2 = Cout;
        g.loader = LOAD_CONV3; g.cH = H; g.cW = W; g.cC = Cin; g.cOH = OH; g.cOW = OW; g.cS = stride; g.pre_relu = pre_relu ? 1 : 0;
        c->launches++;
        if (c->prof_mask & (1u << KC_CONV3)) {  // 2 M N K; input and output tensors once, the packed weight once
            c->prof_flops[KC_CONV3] += 2.0 * (double)g.M * g.N * g.K;
            c->prof_bytes[KC_CONV3] += 4.0 * ((double)F * H * W * Cin + (double)g.N * g.K + (double)g.M * g.N * (1 + (R1 ? 1 : 0) + (R2 ? 1 : 0)));
        }
        Bracket b_(c, KC_CONV3, st);
        return gemm_ws(g);
    }
    int ln(const float *x, RowMap im, const std::string &prefix, float *y, long long rows, int dim, float eps, const float *pe = nullptr,
           int rpf = 0, int TT = 0) {
        const float *w, *b;
        EDV_TRY(param(prefix + ".weight", &w));
        EDV_TRY(param(prefix + ".bias", &b));
        c->launches++;
        HbmScope b_(c, KC_NORM, st, 8.0 * (double)rows * dim);
        return layernorm(x, im, w, b, y, identity_map(), rows, dim, eps, pe, rpf, TT, st);
    }

    // effective weight of a (possibly folded) linear
    int lin_w(const std::string &p, const float **out) {
        auto it = c->packed.find(p + ".weight");
        if (it != c->packed.end() && it->second.p) {
            *out = it->second.p;
            return 0;
        }
        return param(p + ".weight", out);
    }
};

// What the entry points (and the backward, for its transposed weights) run: each builds the Run of its phase on `st`
int run_prepare(edv_ctx *c, hipStream_t st);
int run_refresh_lora(edv_ctx *c, hipStream_t st);
int run_build_x6(edv_ctx *c, hipStream_t st);
int run_prepare_train(edv_ctx *c, hipStream_t st);
int run_forward(edv_ctx *c, hipStream_t st, const float *x, int B, int T, int H, int W, float *const disp[4]);
int run_backward(edv_ctx *c, hipStream_t st, const float *disp0, const float *const g[4]);

}  // namespace edv
