// The C ABI of the engine (include/endodav_hip.h): context life cycle, parameter binding, settings, and the entry points that hand a clip
// to the prepare / forward / backward orchestrators (engine_prepare.hip, engine_forward.hip, engine_backward.hip).
#include "engine.hpp"

namespace edv {
static thread_local std::string g_err;
thread_local LaunchTimer *g_launch_timer = nullptr;
void set_error(const std::string &m) { g_err = m; }
const char *get_error() { return g_err.c_str(); }
}  // namespace edv

// =============================================================================================
extern "C" {

int edv_abi_version(void) { return EDV_ABI_VERSION; }
const char *edv_last_error(void) { return edv::get_error(); }

int edv_create(const edv_config *cfg, edv_ctx **out) {
    EDV_CHECK(cfg && out, "null argument");
    *out = nullptr;  // every check comes before the allocation: an error leaves the handle null and nothing to free
    EDV_CHECK(cfg->abi_version == EDV_ABI_VERSION, "ABI version mismatch");
    EDV_CHECK(cfg->embed_dim > 0 && cfg->num_heads > 0 && cfg->embed_dim == cfg->num_heads * 64, "head dim must be 64");
    EDV_CHECK(cfg->embed_dim <= 1024, "embed_dim > 1024 unsupported");
    EDV_CHECK(cfg->depth > 0, "depth");
    EDV_CHECK(cfg->image_h > 0 && cfg->image_w > 0 && cfg->image_h % 14 == 0 && cfg->image_w % 14 == 0,
              "image_shape must be a multiple of the 14-pixel patch");
    EDV_CHECK(cfg->num_frames > 0, "num_frames must be positive");  // dpt_temporal.py:34
    EDV_CHECK(cfg->features > 0 && cfg->features % 32 == 0, "features must be a multiple of 32 (GroupNorm(32) + 8 heads)");
    for (int j = 0; j < 4; ++j) EDV_CHECK(cfg->out_channels[j] > 0 && cfg->out_channels[j] % 4 == 0, "out_channels must be multiples of 4");
    EDV_CHECK(cfg->out_channels[2] % 32 == 0 && cfg->out_channels[3] % 32 == 0, "out_channels[2:] must be multiples of 32");
    EDV_CHECK(cfg->features <= 1024 && cfg->out_channels[2] <= 1024 && cfg->out_channels[3] <= 1024, "temporal width > 1024 unsupported");
    EDV_CHECK(cfg->lora_type >= 0 && cfg->lora_type <= EDV_LORA_DASH, "lora_type");
    EDV_CHECK(cfg->depth <= 32 && (cfg->depth == 32 || (cfg->residual_mask >> cfg->depth) == 0), "residual_mask names a block >= depth");
    EDV_CHECK(cfg->residual_mask == 0 || (cfg->embed_dim / 8) % 4 == 0, "residual blocks need embed_dim / 8 to be a multiple of 4");
    for (int j = 0; j < 4; ++j) EDV_CHECK(cfg->taps[j] >= 0 && cfg->taps[j] < cfg->depth && (j == 0 || cfg->taps[j] > cfg->taps[j - 1]), "taps");
    const char *products = getenv("EDV_PRODUCTS");  // "f32" | "bf16x6": initial arithmetic of the encoder's linears (edv_set_products changes it)
    EDV_CHECK(!products || !strcmp(products, "f32") || !strcmp(products, "bf16x6"), "EDV_PRODUCTS must be f32 or bf16x6");
    *out = new edv_ctx();
    (*out)->cfg = *cfg;
    if (hipGetDevice(&(*out)->device) != hipSuccess) (*out)->device = -1;  // no device visible (host-only checks of the configuration)
    if (const char *e = getenv("EDV_ENC_STREAMS")) (*out)->enc_streams = (*out)->enc_streams_initial = atoi(e);
    if (products) (*out)->products = !strcmp(products, "bf16x6") ? EDV_PRODUCTS_BF16X6 : EDV_PRODUCTS_F32;
    return 0;
}

int edv_destroy(edv_ctx *ctx) {
    if (!ctx) return 0;
    // free on the device the context lives on, whatever device the calling thread has current (nn.DataParallel destroys replicas'
    // contexts from the main thread), and give the caller its device back
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (ctx->device >= 0 && cur != ctx->device) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto &kv : ctx->packed)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto &kv : ctx->ws)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto &kv : ctx->grads)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (int h = 0; h < 4; ++h) {
        if (ctx->sub[h]) (void)hipStreamDestroy(ctx->sub[h]);
        if (ctx->ev_join[h]) (void)hipEventDestroy(ctx->ev_join[h]);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (int k = 0; k < 6; ++k)
        if (ctx->ev_x[k]) (void)hipEventDestroy(ctx->ev_x[k]);
    for (auto &p : ctx->prof)
        for (auto &e : p.ev) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    const int dev = ctx->device;
    delete ctx;
    if (dev >= 0 && cur >= 0 && cur != dev) (void)hipSetDevice(cur);
    return 0;
}

int edv_bind_param(edv_ctx *ctx, const char *name, const float *data_dev, const int64_t *shape, int32_t ndim) {
    EDV_CHECK(ctx && name && data_dev && (shape || ndim == 0) && ndim >= 0 && ndim <= 8, "bad argument");
    EDV_CHECK(((uintptr_t)data_dev % 16) == 0, std::string("parameter not 16-byte aligned: ") + name);
    Param p;
    p.p = data_dev;
    p.shape.assign(shape, shape + ndim);
    ctx->params[name] = p;
    ctx->prepared = false;
    return 0;
}

int edv_prepare(edv_ctx *ctx, void *stream) {
    EDV_CHECK(ctx, "null context");
    return run_prepare(ctx, (hipStream_t)stream);
}

int edv_refresh_lora(edv_ctx *ctx, void *stream) {
    EDV_CHECK(ctx, "null context");
    return run_refresh_lora(ctx, (hipStream_t)stream);
}

int edv_set_products(edv_ctx *ctx, int32_t products, void *stream) {
    EDV_CHECK(ctx, "null context");
    EDV_CHECK(products == EDV_PRODUCTS_F32 || products == EDV_PRODUCTS_BF16X6, "products: EDV_PRODUCTS_F32 or EDV_PRODUCTS_BF16X6");
    const bool turned_on = products == EDV_PRODUCTS_BF16X6 && ctx->products != EDV_PRODUCTS_BF16X6;
    ctx->products = products;
    if (turned_on && ctx->prepared) {  // planes are kept current only while the mode is on (edv_prepare / edv_refresh_lora): rebuild, never reuse
        ctx->x6.clear();
        return run_build_x6(ctx, (hipStream_t)stream);
    }
    return 0;
}

int edv_get_products(const edv_ctx *ctx) { return ctx ? ctx->products : -1; }

int edv_set_capture(edv_ctx *ctx, int on) {
    EDV_CHECK(ctx, "null context");
    ctx->capture = on != 0;
    return 0;
}

int edv_forward(edv_ctx *ctx, const float *x_dev, int32_t B, int32_t T, int32_t H, int32_t W, float *const disp_dev[4], void *stream) {
    EDV_CHECK(ctx && x_dev && disp_dev, "null argument");
    EDV_CHECK(ctx->prepared, "edv_prepare must run after binding parameters");
    EDV_CHECK(B > 0 && T > 0 && H > 1 && W > 1, "empty clip");
    // motion_module.py:197: the position table is sliced to T -> size mismatch beyond num_frames
    EDV_CHECK(T <= ctx->cfg.num_frames, "T exceeds num_frames (temporal_max_len)");
    // The reference takes any T <= num_frames (dpt_temporal.py:35-40, motion_module.py:180-198).  The temporal-attention kernels hold one pixel's
    // T x T scores on chip: the forward is built up to T = 64 (round 3), the backward up to 32 = the reference's own window length and
    // num_frames default (endodav.py:47, :62; its training scripts use T = 16)
    EDV_CHECK(T <= 64, "T > 64 frames per clip is not built");
    EDV_CHECK(!ctx->train || T <= 32, "a training forward with T > 32 frames per clip is not built (the backward of the temporal attention stops at 32)");

    EDV_CHECK((long long)B * T <= 65535, "too many frames in one call");
    for (int k = 0; k < 4; ++k) EDV_CHECK(disp_dev[k], "null output");
    if (ctx->train) {
        EDV_CHECK(!(ctx->cfg.use_bn), "the fine-tune step with use_bn=True is not built (train-mode BatchNorm uses batch statistics)");
        EDV_CHECK(!ctx->capture, "stage capture and training are exclusive");
    }
    if (ctx->train) ++ctx->generation;  // the kept activations are about to be overwritten
    const int rc = run_forward(ctx, (hipStream_t)stream, x_dev, B, T, H, W, disp_dev);
    if (rc && ctx->sub[0]) {
        // The error may have struck between a fork and its join: kernels already enqueued on the internal streams still write the
        // shared workspaces, and nothing makes the caller's stream wait for them.  Drain them before reporting, so that whatever the
        // caller enqueues next (another edv_forward on this context included) cannot overlap them.
        const std::string msg = edv::get_error();
        for (int h = 0; h < 4; ++h)
            if (ctx->sub[h]) (void)hipStreamSynchronize(ctx->sub[h]);
        edv::set_error(msg);
    }
    ctx->have_saved = rc == 0 && ctx->train;
    if (ctx->have_saved) ctx->saved_generation = ctx->generation;
    return rc;
}

int edv_generation(const edv_ctx *ctx, uint64_t *generation) {
    EDV_CHECK(ctx && generation, "null argument");
    *generation = ctx->generation;
    return 0;
}

int edv_set_train(edv_ctx *ctx, int32_t on) {
    EDV_CHECK(ctx, "null context");
    ctx->train = on != 0;
    if (!ctx->train) ctx->have_saved = false;
    return 0;
}

int edv_set_encoder_streams(edv_ctx *ctx, int32_t n) {
    EDV_CHECK(ctx, "null context");
    EDV_CHECK(n >= -1 && n <= 4, "encoder streams: -1 (initial setting), 0 (automatic), 1 .. 4");
    ctx->enc_streams = n < 0 ? ctx->enc_streams_initial : n;
    return 0;
}

int edv_set_grad_scope(edv_ctx *ctx, int32_t encoder_factors, int32_t temporal_factors, int32_t head_convs, int32_t residual_blocks) {
    EDV_CHECK(ctx, "null context");
    ctx->grad_res = residual_blocks != 0;
    ctx->grad_encoder = encoder_factors != 0;
    ctx->grad_temporal = temporal_factors != 0;
    ctx->grad_head = head_convs != 0;
    return 0;
}

int edv_set_bias_grads(edv_ctx *ctx, int32_t encoder_biases, int32_t head_biases) {
    EDV_CHECK(ctx, "null context");
    ctx->grad_enc_bias = encoder_biases != 0;
    ctx->grad_head_bias = head_biases != 0;
    return 0;
}

int edv_backward(edv_ctx *ctx, uint64_t generation, const float *disp0_dev, const float *const grad_disp_dev[4], void *stream) {
    EDV_CHECK(ctx && disp0_dev && grad_disp_dev, "null argument");
    for (int k = 0; k < 4; ++k) EDV_CHECK(grad_disp_dev[k], "null gradient");
    // One set of kept activations per context: a second training forward overwrites them, and a backward of the first forward's graph
    // would then silently differentiate the second clip.  The caller names the forward it is differentiating.
    EDV_CHECK(generation == 0 || !ctx->have_saved || generation == ctx->saved_generation,
              "edv_backward for training forward #" + std::to_string(generation) + ", but the kept activations are those of forward #" +
                  std::to_string(ctx->saved_generation) + ": a later grad-enabled forward on this context overwrote them (one backward per forward)");
    for (auto &kv : ctx->flat) kv.second.written = false;
    const int rc = run_backward(ctx, (hipStream_t)stream, disp0_dev, grad_disp_dev);
    if (rc) return rc;
    for (auto &kv : ctx->flat)
        EDV_CHECK(kv.second.written, "the flat gradient buffer lists " + kv.first + ", but this backward produced no gradient for it (edv_set_grad_scope)");
    return 0;
}

int edv_grad_bind_flat(edv_ctx *ctx, int32_t n, const char *const *names, const int64_t *numels, float *flat_dev, int64_t flat_floats, int64_t *offsets_out) {
    EDV_CHECK(ctx && n >= 0 && (n == 0 || (names && numels && offsets_out)), "bad argument");
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
        EDV_CHECK(names[i] && numels[i] > 0, "bad slice");
        offsets_out[i] = off;
        off += (numels[i] + 3) & ~(int64_t)3;  // every slice starts on a 16-byte boundary (float4 stores of the reduction kernels)
    }
    if (n) offsets_out[n] = off;
    if (!flat_dev) return 0;  // layout query
    EDV_CHECK(flat_floats >= off && (uintptr_t)flat_dev % 16 == 0, "flat gradient buffer too small or not 16-byte aligned");
    ctx->flat.clear();
    for (int i = 0; i < n; ++i) {
        ctx->flat[names[i]] = edv_ctx::FlatSlot{flat_dev + offsets_out[i], (size_t)numels[i], false};
        // an owned buffer of an earlier unbound backward would otherwise keep answering edv_grad with a stale gradient once the name is unbound again
        auto old = ctx->grads.find(names[i]);
        if (old != ctx->grads.end()) {
            if (old->second.p) {
                ctx->bytes -= old->second.cap * sizeof(float);
                (void)hipFree(old->second.p);
            }
            ctx->grads.erase(old);
        }
    }
    return 0;
}

// Where the latest backward left the gradient of `name`: its slice of the caller's flat buffer when the name is bound (edv_grad_bind_flat), the
// context-owned buffer otherwise.  A bound name never falls through to an owned buffer of an earlier, unbound backward (binding erases those).
static int find_grad(edv_ctx *ctx, const char *name, float **p, size_t *n) {
    auto f = ctx->flat.find(name);
    if (f != ctx->flat.end()) {
        EDV_CHECK(f->second.written, std::string("no gradient for ") + name + " yet: it is bound to the flat buffer and no backward has written it");
        *p = f->second.p;
        *n = f->second.numel;
        return 0;
    }
    auto it = ctx->grads.find(name);
    EDV_CHECK(it != ctx->grads.end() && it->second.p, std::string("no gradient for ") + name);
    *p = it->second.p;
    *n = it->second.cap;
    return 0;
}

int edv_grad_copy(edv_ctx *ctx, const char *name, float *dst_dev, int64_t numel, void *stream) {
    EDV_CHECK(ctx && name && dst_dev, "null argument");
    float *p;
    size_t n;
    EDV_TRY(find_grad(ctx, name, &p, &n));
    EDV_CHECK(numel > 0 && (size_t)numel <= n, std::string("gradient size mismatch for ") + name);
    return copy_f32(p, dst_dev, numel, (hipStream_t)stream);
}

int edv_grad(edv_ctx *ctx, const char *name, float **grad_dev, int64_t *numel) {
    EDV_CHECK(ctx && name && grad_dev && numel, "null argument");
    size_t n;
    EDV_TRY(find_grad(ctx, name, grad_dev, &n));
    *numel = (int64_t)n;
    return 0;
}

int edv_output_shape(const edv_ctx *ctx, int32_t scale, int32_t *h, int32_t *w) {
    EDV_CHECK(ctx && h && w && scale >= 0 && scale < 4, "bad argument");
    const edv_config &c = ctx->cfg;
    if (!c.conv_head) {
        int sh = c.image_h, sw = c.image_w;
        for (int k = 0; k < scale; ++k) { sh /= 2; sw /= 2; }
        *h = sh; *w = sw;
    } else {
        const int ph = c.image_h / 14, pw = c.image_w / 14;
        const int mul[4] = {16, 8, 4, 2};
        *h = ph * mul[scale]; *w = pw * mul[scale];
    }
    return 0;
}

int edv_stage_copy(edv_ctx *ctx, const char *name, float *dst_dev, size_t *n, void *stream) {
    EDV_CHECK(ctx && name && n, "bad argument");
    if (std::string(name).rfind("ws:", 0) == 0) {  // any workspace buffer by name, whole capacity (gradient-stage parity tests)
        auto w = ctx->ws.find(std::string(name).substr(3));
        EDV_CHECK(w != ctx->ws.end() && w->second.p, std::string("no such workspace buffer: ") + name);
        *n = w->second.cap;
        if (dst_dev) return copy_f32(w->second.p, dst_dev, (long long)w->second.cap, (hipStream_t)stream);
        return 0;
    }
    auto it = ctx->stages.find(name);
    EDV_CHECK(it != ctx->stages.end(), std::string("stage not available (capture off or unknown): ") + name);
    *n = it->second.second;
    if (dst_dev) return copy_f32(it->second.first, dst_dev, (long long)it->second.second, (hipStream_t)stream);
    return 0;
}

int edv_profile_enable(edv_ctx *ctx, uint32_t class_mask) {
    EDV_CHECK(ctx, "null context");
    EDV_CHECK(class_mask < (1u << KC_COUNT), "unknown kernel class in mask");
    ctx->prof_mask = class_mask;
    for (auto &p : ctx->prof) p.used = 0;
    for (int k = 0; k < KC_COUNT; ++k) ctx->prof_flops[k] = ctx->prof_bytes[k] = 0.0;
    return 0;
}

int edv_profile_set_mask(edv_ctx *ctx, uint32_t class_mask) {
    EDV_CHECK(ctx, "null context");
    EDV_CHECK(class_mask < (1u << KC_COUNT), "unknown kernel class in mask");
    ctx->prof_mask = class_mask;  // nothing recorded so far is dropped
    return 0;
}

int edv_profile_read(edv_ctx *ctx, int32_t kernel_class, int32_t *launches, double *total_ms) {
    EDV_CHECK(ctx && launches && total_ms, "null argument");
    EDV_CHECK(kernel_class >= 0 && kernel_class < KC_COUNT, "unknown kernel class");
    EvPool &p = ctx->prof[kernel_class];
    double sum = 0.0;
    for (size_t i = 0; i < p.used; ++i) {
        EDV_HIP(hipEventSynchronize(p.ev[i].second));
        float ms = 0.f;
        EDV_HIP(hipEventElapsedTime(&ms, p.ev[i].first, p.ev[i].second));
        sum += ms;
    }
    *launches = (int32_t)p.used;
    *total_ms = sum;
    p.used = 0;
    return 0;
}

int edv_profile_work(edv_ctx *ctx, int32_t kernel_class, double *flops, double *bytes) {
    EDV_CHECK(ctx && flops && bytes, "null argument");
    EDV_CHECK(kernel_class >= 0 && kernel_class < KC_COUNT, "unknown kernel class");
    *flops = ctx->prof_flops[kernel_class];
    *bytes = ctx->prof_bytes[kernel_class];
    ctx->prof_flops[kernel_class] = ctx->prof_bytes[kernel_class] = 0.0;
    return 0;
}

size_t edv_device_bytes(const edv_ctx *ctx) { return ctx ? ctx->bytes : 0; }
int edv_last_launch_count(const edv_ctx *ctx) { return ctx ? ctx->launches : 0; }

}  // extern "C"
