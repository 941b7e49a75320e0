// =========================================================================================
// Backward.  Trainable: the LoRA / DV-LoRA factors of mlp.fc1 / mlp.fc2 in every encoder
// block (endodav/layers.py:5-34 names lora_A, lora_B, lora_U, lora_V), the scopes of edv_set_grad_scope and, under
// edv_set_bias_grads, the biases (bias="all"); everything else is frozen, so each operator contributes its input gradient only.  Mirrors forward() in reverse on the activations a training forward kept.
#include "engine.hpp"

namespace {

struct Backward : Run {
    using Run::Run;
    const float *const *g = nullptr;  // dL/d disp[0..3], the caller's
    // gradients one phase hands to the next: of path_1..path_4, layer1_rn..layer4_rn, the resized levels 1..4, the encoder taps
    float *d_p[5], *d_r[5], *d_l[5], *d_tap[4], *d_tapcls[4] = {nullptr, nullptr, nullptr, nullptr};
    float *lora_ws = nullptr;  // workspace of lora_grads for the whole backward
    size_t lora_ws_n = 0;
    int gradbuf(const std::string &name, size_t n, float **out) {
        auto it = c->flat.find(name);
        if (it != c->flat.end()) {  // the caller's flat buffer holds this gradient (edv_grad_bind_flat)
            EDV_CHECK(it->second.numel == n, "flat gradient slice of " + name + " has " + std::to_string(it->second.numel) + " floats, the gradient " +
                                                 std::to_string(n));
            it->second.written = true;
            *out = it->second.p;
            return 0;
        }
        return alloc_buf(c, c->grads, name, n, st, out);
    }
    int saved(const std::string &name, const float **out) {
        auto it = c->ws.find(name);
        EDV_CHECK(it != c->ws.end() && it->second.p, "activation not saved (run a forward with edv_set_train first): " + name);
        *out = it->second.p;
        return 0;
    }
    // ---- bias gradients (edv_set_bias_grads).  Stage 1 of the batched column sum (bias_colsum.hip) runs where each dY is still live --
    // bias_flush() before a buffer that a pending job reads is overwritten -- and stage 2 runs once, in bias_finish(), for every tensor.
    float *bias_slab = nullptr;
    size_t bias_slab_n = 0, bias_slab_off = 0;
    std::vector<ColsumJob> bias_jobs;  // stage 1, not launched yet
    struct BiasOut {
        std::string name;
        size_t off;
        int rows, N;
        const float *scale;
    };
    std::vector<BiasOut> bias_outs;
    struct BiasSrc {
        const float *p;
        long long rows;
        int ld;
        RowMap map;
    };
    // gradient of `name` = scale (.) sum of the rows of every source (all [rows, N], row stride ld)
    int bias_grad(const std::string &name, const std::vector<BiasSrc> &srcs, int N, const float *scale = nullptr) {
        BiasOut o{name, bias_slab_off, 0, N, scale};
        for (const BiasSrc &sr : srcs) {
            ColsumJob j = colsum_job(sr.p, sr.ld, sr.rows, sr.map, N);
            EDV_CHECK(bias_slab_off + (size_t)j.parts * N <= bias_slab_n, "bias gradient slab too small for " + name);
            j.slab = bias_slab + bias_slab_off;
            bias_slab_off += (size_t)j.parts * N;
            o.rows += j.parts;
            bias_jobs.push_back(j);
        }
        bias_outs.push_back(o);
        return 0;
    }
    int bias_grad(const std::string &name, const float *p, long long rows, int N, const float *scale = nullptr) {
        return bias_grad(name, {BiasSrc{p, rows, N, identity_map()}}, N, scale);
    }
    int bias_flush() {
        if (bias_jobs.empty()) return 0;
        c->launches += ((int)bias_jobs.size() + CS_MAX_JOBS - 1) / CS_MAX_JOBS;
        EDV_TRY(colsum_stage1_launch(bias_jobs.data(), (int)bias_jobs.size(), st));
        bias_jobs.clear();
        return 0;
    }
    int bias_finish() {
        EDV_TRY(bias_flush());
        if (bias_outs.empty()) return 0;
        std::vector<ColsumOut> outs;
        for (const BiasOut &o : bias_outs) {
            float *dst;
            EDV_TRY(gradbuf(o.name, (size_t)o.N, &dst));
            outs.push_back(ColsumOut{bias_slab + o.off, o.rows, o.N, o.scale, dst, 0});
        }
        c->launches += ((int)outs.size() + CS_MAX_OUTS - 1) / CS_MAX_OUTS;
        EDV_TRY(colsum_stage2_launch(outs.data(), (int)outs.size(), st));
        bias_outs.clear();
        return 0;
    }
    int bias_begin() {
        bias_jobs.clear();
        bias_outs.clear();
        bias_slab_off = 0;
        if (!c->grad_enc_bias && !c->grad_head_bias) return 0;
        // every source job holds at most CS_MAX_PARTS partial rows; pretrained.norm.bias has up to eight sources (four taps, four cls rows)
        size_t n = 8 * (size_t)D;
        for (const auto &kv : c->params)
            if (kv.first.size() > 5 && kv.first.compare(kv.first.size() - 5, 5, ".bias") == 0) n += kv.second.numel();
        bias_slab_n = n * CS_MAX_PARTS;
        return wsbuf("g.bias.slab", bias_slab_n, &bias_slab);
    }
    bool head_params() const { return c->grad_head || c->grad_head_bias; }
    // dX[M, K] = dY[M, N] W  through the NT GEMM with the cached transposed weight ("T." + key is [K, N])
    int dgemm(const float *dY, long long M, int N, const std::string &key, int K, float *dX, const float *R1 = nullptr) {
        const float *wt;
        EDV_TRY(packedw("T." + key, &wt));
        return linear(dY, M, N, wt, K, nullptr, dX, ACT_NONE, nullptr, R1);
    }
    int dconv3(const float *dY, int H, int W, int Cout_fwd, const std::string &p, int Cin_fwd, float *dX, const float *add = nullptr) {
        const float *wb;
        EDV_TRY(packedw("B." + p, &wb));
        return conv3(dY, H, W, Cout_fwd, wb, nullptr, Cin_fwd, 1, dX, false, ACT_NONE, add);
    }
    // weight + bias gradient of a trainable 3x3 convolution p (x: its input, dY: the gradient of its output), when the caller asked for them
    int conv_param_grads(const std::string &p, const float *x, const float *dY, int H, int W, int Cin, int Cout) {
        if (!c->grad_head) return c->grad_head_bias ? bias_grad(p + ".bias", dY, (long long)F * H * W, Cout) : 0;
        float *dw, *db, *ws;
        EDV_TRY(gradbuf(p + ".weight", (size_t)Cout * Cin * 9, &dw));
        EDV_TRY(gradbuf(p + ".bias", (size_t)Cout, &db));
        size_t need = conv3_wgrad_workspace(F, H, W, Cin, Cout);
        const size_t cs = colsum_workspace(Cout);
        need = need > cs ? need : cs;
        EDV_TRY(wsbuf("g.wgrad", need, &ws));
        EDV_TRY(conv3_wgrad(x, dY, dw, F, H, W, Cin, Cout, ws, need, false, st));
        EDV_TRY(colsum_rows(dY, nullptr, (long long)F * H * W, Cout, ws, need, db, false, st));
        c->launches += 4;
        return 0;
    }
    // weight + bias gradient of a 1x1 convolution to one channel: dW[c] = sum_p gz[p] o2[p, c], db = sum_p gz[p]
    int dot_param_grads(const std::string &p, const float *o2, const float *gz, long long npix, int C) {
        if (!c->grad_head) return c->grad_head_bias ? bias_grad(p + ".bias", gz, npix, 1) : 0;
        float *dw, *db, *ws;
        EDV_TRY(gradbuf(p + ".weight", (size_t)C, &dw));
        EDV_TRY(gradbuf(p + ".bias", 1, &db));
        const size_t need = colsum_workspace(C);
        EDV_TRY(wsbuf("g.wgrad1", need, &ws));
        EDV_TRY(colsum_rows(o2, gz, npix, C, ws, need, dw, false, st));
        EDV_TRY(colsum_rows(gz, nullptr, npix, 1, ws, need, db, false, st));
        c->launches += 4;
        return 0;
    }

    // y = LN(x) * w + b over `dim` channels: input gradient into dx, and (grad_res) dL/dw = colsum(dy * xhat), dL/db = colsum(dy)
    int ln_affine_bwd(const std::string &norm, const float *x, const float *dy, float *dx, long long rows, int dim) {
        const float *w;
        EDV_TRY(param(norm + ".weight", &w));
        EDV_TRY(layernorm_bwd(x, identity_map(), w, dy, identity_map(), dx, identity_map(), rows, dim, 1e-6f, false, st));
        if (!c->grad_res && c->grad_enc_bias) {  // bias="all" without the residual scope: the bias only, as the residual scope makes it
            float *part, *db;
            EDV_TRY(wsbuf("g.rb.part", (size_t)TALL_SPLITS * D, &part));
            EDV_TRY(gradbuf(norm + ".bias", (size_t)dim, &db));
            return col_dot(dy, nullptr, rows, dim, nullptr, part, db, st);
        }
        if (!c->grad_res) return 0;
        float *ones, *zeros, *xhat, *part, *dw, *db;
        EDV_TRY(wsbuf("g.rb.ones", (size_t)D, &ones));
        EDV_TRY(wsbuf("g.rb.zeros", (size_t)D, &zeros));
        EDV_HIP(hipMemsetD32Async((hipDeviceptr_t)ones, 0x3f800000, (size_t)D, st));
        EDV_HIP(hipMemsetAsync(zeros, 0, (size_t)D * sizeof(float), st));
        EDV_TRY(wsbuf("g.rb.xhat", (size_t)rows * D, &xhat));
        EDV_TRY(wsbuf("g.rb.part", (size_t)TALL_SPLITS * D, &part));
        EDV_TRY(gradbuf(norm + ".weight", (size_t)dim, &dw));
        EDV_TRY(gradbuf(norm + ".bias", (size_t)dim, &db));
        EDV_TRY(layernorm(x, identity_map(), ones, zeros, xhat, identity_map(), rows, dim, 1e-6f, nullptr, 0, 0, st));
        EDV_TRY(col_dot(dy, xhat, rows, dim, nullptr, part, dw, st));
        EDV_TRY(col_dot(dy, nullptr, rows, dim, nullptr, part, db, st));
        return 0;
    }
    // dW[N, K] = dY^T X for a 1x1 convolution / linear without bias (dY [M, N], X [M, K]): both operands transposed, then the NT GEMM
    int linear_wgrad(const std::string &name, const float *dY, int N, const float *X, int K, long long M) {
        if (!c->grad_res) return 0;
        float *dyt, *xt_, *dw;
        EDV_TRY(wsbuf("g.rb.dyt", (size_t)M * D, &dyt));
        EDV_TRY(wsbuf("g.rb.xt", (size_t)M * D, &xt_));
        EDV_TRY(gradbuf(name, (size_t)N * K, &dw));
        EDV_TRY(transpose_scale(dY, N, nullptr, dyt, (int)M, N, st));  // [M, N] -> [N, M]
        EDV_TRY(transpose_scale(X, K, nullptr, xt_, (int)M, K, st));   // [M, K] -> [K, M]
        return linear(dyt, N, (int)M, xt_, K, nullptr, dw);
    }
    // backward of the residual block of encoder block i: dxt (gradient of the block output, [F*ntok, D]) gains, on its patch rows,
    // the gradient that flows through conv1 .. norm3 (the identity path is already in dxt)
    int res_bottleneck_bwd(int i, float *dxt) {
        const std::string p = "pretrained.blocks." + std::to_string(i) + ".residual_", tg = "rbt" + std::to_string(i) + ".";
        const int Cb = D / 8;
        const long long MP = (long long)F * P0;
        const float *xp, *t1a, *ln1, *a1, *t1b, *ln2, *a2, *t3;
        EDV_TRY(saved(tg + "xp", &xp));
        EDV_TRY(saved(tg + "t1a", &t1a));
        EDV_TRY(saved(tg + "ln1", &ln1));
        EDV_TRY(saved(tg + "a1", &a1));
        EDV_TRY(saved(tg + "t1b", &t1b));
        EDV_TRY(saved(tg + "ln2", &ln2));
        EDV_TRY(saved(tg + "a2", &a2));
        EDV_TRY(saved(tg + "t3", &t3));
        float *dout, *dD, *dC1, *dC2;
        EDV_TRY(wsbuf("g.rb.dout", (size_t)MP * D, &dout));
        EDV_TRY(wsbuf("g.rb.dD", (size_t)MP * D, &dD));
        EDV_TRY(wsbuf("g.rb.dC1", (size_t)MP * Cb, &dC1));
        EDV_TRY(wsbuf("g.rb.dC2", (size_t)MP * Cb, &dC2));
        for (int f = 0; f < F; ++f) EDV_TRY(copy_f32(dxt + ((size_t)f * ntok + c0) * D, dout + (size_t)f * P0 * D, (long long)P0 * D, st));
        EDV_TRY(ln_affine_bwd(p + ".norm3", t3, dout, dD, MP, D));                 // out = LN3(t3)
        EDV_TRY(linear_wgrad(p + ".conv3.weight", dD, D, a2, Cb, MP));            // t3 = a2 W3^T
        EDV_TRY(dgemm(dD, MP, D, p + ".conv3", Cb, dC1));
        EDV_TRY(ew_bwd(dC1, ln2, nullptr, dC1, MP * Cb, 1, st));                   // a2 = gelu(ln2)
        EDV_TRY(ln_affine_bwd(p + ".norm2", t1b, dC1, dC2, MP, Cb));              // ln2 = LN2(t1b)
        if (c->grad_res) {
            float *dw, *ws;
            EDV_TRY(gradbuf(p + ".conv2.weight", (size_t)Cb * Cb * 9, &dw));
            const size_t need = conv3_wgrad_workspace(F, ph, pw, Cb, Cb);
            EDV_TRY(wsbuf("g.wgrad", need, &ws));
            EDV_TRY(conv3_wgrad(a1, dC2, dw, F, ph, pw, Cb, Cb, ws, need, false, st));  // t1b = conv2(a1)
        }
        EDV_TRY(dconv3(dC2, ph, pw, Cb, p + ".conv2", Cb, dC1));
        EDV_TRY(ew_bwd(dC1, ln1, nullptr, dC1, MP * Cb, 1, st));                   // a1 = gelu(ln1)
        EDV_TRY(ln_affine_bwd(p + ".norm1", t1a, dC1, dC2, MP, Cb));              // ln1 = LN1(t1a)
        EDV_TRY(linear_wgrad(p + ".conv1.weight", dC2, Cb, xp, D, MP));           // t1a = xp W1^T
        EDV_TRY(dgemm(dC2, MP, Cb, p + ".conv1", D, dD));
        for (int f = 0; f < F; ++f) {  // patch rows of dxt += the branch's input gradient
            float *dst = dxt + ((size_t)f * ntok + c0) * D;
            EDV_TRY(ew_bwd(dD + (size_t)f * P0 * D, nullptr, dst, dst, (long long)P0 * D, 0, st));
        }
        c->launches += 20 + 2 * F;
        return 0;
    }

    // motion module backward, in place on d [F, P, C] (dL/d output -> dL/d input)
    int motion_module_bwd(int m, float *d, int P, int C) {
        const std::string p = "head.motion_modules." + std::to_string(m) + ".temporal_transformer";
        const std::string tb = p + ".transformer_blocks.0";
        const std::string tg = "mm" + std::to_string(m) + ".";
        const long long M = (long long)F * P;
        float *dh, *t1, *t3, *t4, *t8, *sums;
        EDV_TRY(wsbuf("g.mm.dh", (size_t)M * C, &dh));
        EDV_TRY(wsbuf("g.mm.t1", (size_t)M * C, &t1));
        EDV_TRY(wsbuf("g.mm.t3", (size_t)M * 3 * C, &t3));
        EDV_TRY(wsbuf("g.mm.t4", (size_t)M * 4 * C, &t4));
        EDV_TRY(wsbuf("g.mm.t8", (size_t)M * 8 * C, &t8));
        EDV_TRY(wsbuf("g.mm.sums", (size_t)F * 32 * 2, &sums));
        const float *xin, *stats, *hsv[3], *qkvs[2], *ff1, *w;
        EDV_TRY(saved(tg + "xin", &xin));
        EDV_TRY(saved(tg + "stats", &stats));
        EDV_TRY(saved(tg + "h", &hsv[0]));
        EDV_TRY(saved(tg + "h1", &hsv[1]));
        EDV_TRY(saved(tg + "h2", &hsv[2]));
        EDV_TRY(saved(tg + "qkv0", &qkvs[0]));
        EDV_TRY(saved(tg + "qkv1", &qkvs[1]));
        EDV_TRY(saved(tg + "ff1", &ff1));
        EDV_TRY(dgemm(d, M, C, p + ".proj_out", C, dh));                   // x = xin + proj_out(h3)
        if (cfg.temporal_lora && cfg.lora_type != EDV_LORA_NONE && c->grad_temporal) {  // temporal LoRA on ff.net.2 (endodav.py:119-137)
            const float *ff2;
            EDV_TRY(saved(tg + "ff2", &ff2));
            EDV_TRY(lora_step(tb + ".ff.net.2", ff2, 4 * C, dh, C, M, cfg.lora_rank, (cfg.lora_type == EDV_LORA_LORA || cfg.lora_type == EDV_LORA_DASH) ? 2.0f : 1.0f, "", lora_ws, lora_ws_n));
        }
        EDV_TRY(dgemm(dh, M, C, tb + ".ff.net.2", 4 * C, t4));             // h3 = h2 + ff2 W2
        EDV_TRY(geglu_bwd(ff1, t4, t8, M, 4 * C, st));
        EDV_TRY(dgemm(t8, M, 8 * C, tb + ".ff.net.0.proj", C, t1));
        const bool hb = c->grad_head_bias;
        if (hb) {  // dh, t1 are about to change: each bias's dY while it is live
            EDV_TRY(bias_grad(p + ".proj_out.bias", d, M, C));
            EDV_TRY(bias_grad(tb + ".ff.net.2.bias", dh, M, C));
            EDV_TRY(bias_grad(tb + ".ff.net.0.proj.bias", t8, M, 8 * C));
            EDV_TRY(bias_grad(tb + ".ff_norm.bias", t1, M, C));
            EDV_TRY(bias_flush());
        }
        EDV_TRY(param(tb + ".ff_norm.weight", &w));
        EDV_TRY(layernorm_bwd(hsv[2], identity_map(), w, t1, identity_map(), dh, identity_map(), M, C, 1e-5f, true, st));
        for (int a = 1; a >= 0; --a) {
            const std::string ab = tb + ".attention_blocks." + std::to_string(a);
            if (hb) EDV_TRY(bias_grad(ab + ".to_out.0.bias", dh, M, C));
            EDV_TRY(dgemm(dh, M, C, ab + ".to_out.0", C, t1));             // h(a+1) = h(a) + to_out(att)
            EDV_TRY(attn_temporal_bwd(qkvs[a], t1, t3, B, T, P, C, 8, st));  // qkvs[a] holds the rotated q|k under pe="rope"
            if (cfg.pe_rope) {
                const float *rope;
                EDV_TRY(param(ab + ".freqs_cis", &rope, 3));
                EDV_TRY(rope_qk(t3, rope, B, T, P, C, true, st));
            }
            EDV_TRY(dgemm(t3, M, 3 * C, ab + ".qkv", C, t1));
            if (hb) {
                EDV_TRY(bias_grad(tb + ".norms." + std::to_string(a) + ".bias", t1, M, C));
                EDV_TRY(bias_flush());
            }
            EDV_TRY(param(tb + ".norms." + std::to_string(a) + ".weight", &w));
            EDV_TRY(layernorm_bwd(hsv[a], identity_map(), w, t1, identity_map(), dh, identity_map(), M, C, 1e-5f, true, st));
        }
        EDV_TRY(dgemm(dh, M, C, p + ".proj_in", C, t1));
        if (hb) {
            EDV_TRY(bias_grad(p + ".proj_in.bias", dh, M, C));
            EDV_TRY(bias_grad(p + ".norm.bias", t1, M, C));  // GroupNorm: d beta = sum of dy
            EDV_TRY(bias_flush());
        }
        EDV_TRY(param(p + ".norm.weight", &w));
        EDV_TRY(groupnorm_bwd(xin, stats, w, t1, sums, d, F, P, C, 32, true, st));
        c->launches += 8;
        return 0;
    }

    // FeatureFusionBlock backward: d_out [F,oh,ow,Fe] -> d_x (and d_skip when the block has a skip input), both [F,h,w,Fe]
    int fusion_bwd(int j, const float *d_out, const float *cur_or_x, const float *skip, int h, int w, int oh, int ow, float *d_x, float *d_skip) {
        const std::string p = "head.scratch.refinenet" + std::to_string(j);
        const std::string tg = "fu" + std::to_string(j) + ".";
        const size_t n = (size_t)F * h * w * Fe;
        const long long MP_ = (long long)F * h * w;
        float *a, *b2, *a0;
        EDV_TRY(wsbuf("g.fu.a", n, &a));
        EDV_TRY(wsbuf("g.fu.b", n, &b2));
        const bool hb = c->grad_head_bias;
        a0 = a;
        if (hb) EDV_TRY(wsbuf("g.fu.a0", n, &a0));  // out_conv's dY stays live until the first flush below
        const float *t1a = nullptr, *t1b, *cur = cur_or_x;
        EDV_TRY(saved(tg + "t1b", &t1b));
        if (skip) {
            EDV_TRY(saved(tg + "t1a", &t1a));
            EDV_TRY(saved(tg + "s", &cur));
        }
        EDV_TRY(bilinear_bwd(d_out, a0, F, h, w, Fe, oh, ow, false, st));                     // out = up(out_conv(t2))
        EDV_TRY(dgemm(a0, MP_, Fe, p + ".out_conv", Fe, d_x));                                 // d_x <- d_t2 for now
        EDV_TRY(dconv3(d_x, h, w, Fe, p + ".resConfUnit2.conv2", Fe, a));                      // t2 = cur + conv2(relu(t1b))
        EDV_TRY(ew_bwd(a, t1b, nullptr, a, (long long)n, 2, st));
        if (hb) {  // the upsample's weights sum to one: out_conv's bias gradient is the column sum before or after it
            EDV_TRY(bias_grad(p + ".out_conv.bias", a0, MP_, Fe));
            EDV_TRY(bias_grad(p + ".resConfUnit2.conv2.bias", d_x, MP_, Fe));
            EDV_TRY(bias_grad(p + ".resConfUnit2.conv1.bias", a, MP_, Fe));
            EDV_TRY(bias_flush());
        }
        EDV_TRY(dconv3(a, h, w, Fe, p + ".resConfUnit2.conv1", Fe, b2));                       // t1b = conv1(relu(cur))
        EDV_TRY(ew_bwd(b2, cur, d_x, d_x, (long long)n, 2, st));                               // d_cur = d_t2 + mask(cur) * .
        if (skip) {                                                                            // cur = x + skip + conv2a(relu(t1a))
            EDV_TRY(dconv3(d_x, h, w, Fe, p + ".resConfUnit1.conv2", Fe, a));
            EDV_TRY(ew_bwd(a, t1a, nullptr, a, (long long)n, 2, st));
            EDV_TRY(dconv3(a, h, w, Fe, p + ".resConfUnit1.conv1", Fe, b2));                   // t1a = conv1a(relu(skip))
            EDV_TRY(ew_bwd(b2, skip, d_x, d_skip, (long long)n, 2, st));
            if (hb) {
                EDV_TRY(bias_grad(p + ".resConfUnit1.conv2.bias", d_x, MP_, Fe));
                EDV_TRY(bias_grad(p + ".resConfUnit1.conv1.bias", a, MP_, Fe));
                EDV_TRY(bias_flush());
            }
        }
        c->launches += 6;
        return 0;
    }

    int workspaces() {
        const int *oc = cfg.out_channels;
        const long long MT = (long long)F * ntok;
        {   // the input-gradient GEMMs run on the caller's stream alone: stream-K region 0 of the forward's workspace, if there is one
            auto it = c->ws.find("skws");
            const bool have = it != c->ws.end() && it->second.p && c->skws_zeroed == it->second.p;
            skws = have ? it->second.p : nullptr;
            skws_floats = have ? gemm_workspace() : 0;
        }
        {   // one workspace for every LoRA-gradient call: encoder MLPs (M = F*ntok, D <-> 4D) and, with temporal_lora, ff.net.2
            size_t need = 4;
            if (cfg.lora_type != EDV_LORA_NONE) {
                need = lora_grads_workspace(MT, D, 4 * D, cfg.lora_rank);
                if (cfg.temporal_lora) {
                    const long long Ms[4] = {(long long)F * h3 * w3, (long long)F * h4 * w4, (long long)F * h3 * w3, (long long)F * h2 * w2};
                    const int Cs[4] = {oc[2], oc[3], Fe, Fe};
                    for (int m = 0; m < 4; ++m) {
                        const size_t n = lora_grads_workspace(Ms[m], 4 * Cs[m], Cs[m], cfg.lora_rank);
                        need = n > need ? n : need;
                    }
                }
            }
            EDV_TRY(wsbuf("g.lora", need, &lora_ws));
            lora_ws_n = need;
        }
        return 0;
    }

    // HeadDepth k on path_(k+1) (endodav/layers.py:206-221, dpt_pyramid.py:103-109): gradient of the path, written to dst or added to it
    int head_depth_bwd(int k, int h, int w, const std::string &path, float *dst, bool add) {
        const std::string hp = "head.conv_depth_" + std::to_string(k + 1) + ".head.", tg = "hd" + std::to_string(k) + ".";
        const long long px = (long long)F * h * w;
        const float *pk, *o1, *up, *o2, *dk, *w4;
        EDV_TRY(saved(path, &pk));
        EDV_TRY(saved(tg + "o1", &o1));
        EDV_TRY(saved(tg + "up", &up));
        EDV_TRY(saved(tg + "o2", &o2));
        EDV_TRY(saved(tg + "disp", &dk));
        (void)o1;
        float *d_o2, *d_up, *d_o1, *gz;
        EDV_TRY(wsbuf("g.o2", (size_t)F * 4 * h0 * w0 * 32, &d_o2));
        EDV_TRY(wsbuf("g.up", (size_t)F * 4 * h0 * w0 * Fh, &d_up));
        EDV_TRY(wsbuf("g.o1", (size_t)F * h0 * w0 * Fh, &d_o1));
        EDV_TRY(wsbuf("g.gz", (size_t)F * 4 * h0 * w0, &gz));
        EDV_TRY(param(hp + "4.weight", &w4));
        EDV_TRY(dot_channels_bwd(g[k], dk, w4, o2, d_o2, gz, px * 4, 32, cfg.inv_sigmoid ? 2 : 1, st));
        EDV_TRY(dot_param_grads(hp + "4", o2, gz, px * 4, 32));
        EDV_TRY(conv_param_grads(hp + "2", up, d_o2, 2 * h, 2 * w, Fh, 32));
        EDV_TRY(dconv3(d_o2, 2 * h, 2 * w, 32, hp + "2", Fh, d_up));
        EDV_TRY(bilinear_bwd(d_up, d_o1, F, h, w, Fh, 2 * h, 2 * w, false, st));
        EDV_TRY(conv_param_grads(hp + "0", pk, d_o1, h, w, Fe, Fh));
        EDV_TRY(dconv3(d_o1, h, w, Fh, hp + "0", Fe, dst, add ? dst : nullptr));
        EDV_TRY(bias_flush());  // the next head reuses g.o2 / g.o1 / g.gz
        c->launches += 2;
        return 0;
    }
    int vda_head_bwd(const float *disp0) {
        const int ih = cfg.image_h, iw = cfg.image_w;
            // ---------------- VDA head: disp[k] = down(disp[k-1]); disp[0] = relu(dot(relu(conv2(up(conv1(p1)))))) ----
            int sh[4], sw[4];
            sh[0] = ih; sw[0] = iw;
            for (int k = 1; k < 4; ++k) { sh[k] = sh[k - 1] / 2; sw[k] = sw[k - 1] / 2; }
            float *gd[3];
            const float *g3 = g[3], *mask0 = disp0;
            if (cfg.out_sigmoid) {  // disp[k] = sigmoid(raw[k]) (dpt_pyramid.py:97-101): dL/d raw[k] = g[k] s (1 - s); the ReLU mask is the raw map's
                float *g3s;
                const float *sg;
                EDV_TRY(wsbuf("g.d3", (size_t)F * sh[3] * sw[3], &g3s));
                EDV_TRY(saved("hd.sg3", &sg));
                EDV_TRY(sigmoid_bwd(g[3], sg, g3s, (long long)F * sh[3] * sw[3], st));
                g3 = g3s;
                EDV_TRY(saved("hd.raw0", &mask0));
            }
            for (int k = 2; k >= 0; --k) {
                EDV_TRY(wsbuf("g.d" + std::to_string(k), (size_t)F * sh[k] * sw[k], &gd[k]));
                if (cfg.out_sigmoid) {
                    const float *sg;
                    EDV_TRY(saved("hd.sg" + std::to_string(k), &sg));
                    EDV_TRY(sigmoid_bwd(g[k], sg, gd[k], (long long)F * sh[k] * sw[k], st));
                } else {
                    EDV_TRY(copy_f32(g[k], gd[k], (long long)F * sh[k] * sw[k], st));
                }
                EDV_TRY(bilinear_bwd(k == 2 ? g3 : gd[k + 1], gd[k], F, sh[k], sw[k], 1, sh[k + 1], sw[k + 1], true, st));
            }
            float *d_o2, *d_up, *d_o1, *gz = nullptr;
            const float *o2, *w, *p1, *up;
            EDV_TRY(saved("hd.o2", &o2));
            EDV_TRY(wsbuf("g.o2", (size_t)F * ih * iw * 32, &d_o2));
            EDV_TRY(wsbuf("g.up", (size_t)F * ih * iw * Fh, &d_up));
            EDV_TRY(wsbuf("g.o1", (size_t)F * h0 * w0 * Fh, &d_o1));
            if (head_params()) EDV_TRY(wsbuf("g.gz", (size_t)F * ih * iw, &gz));  // --train_output_conv (endodav/layers.py:5-34), bias="all"
            EDV_TRY(param("head.scratch.output_conv2.2.weight", &w));
            EDV_TRY(dot_channels_bwd(gd[0], mask0, w, o2, d_o2, gz, (long long)F * ih * iw, 32, 0, st));
            if (head_params()) {
                EDV_TRY(saved("hd.up", &up));
                EDV_TRY(saved("p1", &p1));
                EDV_TRY(dot_param_grads("head.scratch.output_conv2.2", o2, gz, (long long)F * ih * iw, 32));
                EDV_TRY(conv_param_grads("head.scratch.output_conv2.0", up, d_o2, ih, iw, Fh, 32));
            }
            EDV_TRY(dconv3(d_o2, ih, iw, 32, "head.scratch.output_conv2.0", Fh, d_up));
            EDV_TRY(bilinear_bwd(d_up, d_o1, F, h0, w0, Fh, ih, iw, false, st));
            if (head_params()) EDV_TRY(conv_param_grads("head.scratch.output_conv1", p1, d_o1, h0, w0, Fe, Fh));
            EDV_TRY(dconv3(d_o1, h0, w0, Fh, "head.scratch.output_conv1", Fe, d_p[1]));
        return 0;
    }
    int fuse_bwd() {  // fusion blocks and the two motion modules between them (and, with conv_head, HeadDepth heads 2..4 on their paths)
        const int hs[5] = {h0, h1, h2, h3, h4}, wsz[5] = {w0, w1, w2, w3, w4};
        for (int k = 2; k <= 4; ++k) EDV_TRY(wsbuf("g.p" + std::to_string(k), (size_t)F * hs[k - 1] * wsz[k - 1] * Fe, &d_p[k]));
        for (int j = 1; j <= 4; ++j) EDV_TRY(wsbuf("g.r" + std::to_string(j), (size_t)F * hs[j] * wsz[j] * Fe, &d_r[j]));
        const float *r[5];
        for (int j = 1; j <= 4; ++j) EDV_TRY(saved("r" + std::to_string(j), &r[j]));
        EDV_TRY(fusion_bwd(1, d_p[1], nullptr, r[1], h1, w1, h0, w0, d_p[2], d_r[1]));
        if (cfg.conv_head) EDV_TRY(head_depth_bwd(1, h1, w1, "p2", d_p[2], true));   // path_2 also feeds conv_depth_2
        EDV_TRY(fusion_bwd(2, d_p[2], nullptr, r[2], h2, w2, h1, w1, d_p[3], d_r[2]));
        if (cfg.conv_head) EDV_TRY(head_depth_bwd(2, h2, w2, "p3", d_p[3], true));   // path_3 (after motion module 3) feeds conv_depth_3
        EDV_TRY(motion_module_bwd(3, d_p[3], h2 * w2, Fe));
        EDV_TRY(fusion_bwd(3, d_p[3], nullptr, r[3], h3, w3, h2, w2, d_p[4], d_r[3]));
        if (cfg.conv_head) EDV_TRY(head_depth_bwd(3, h3, w3, "p4", d_p[4], true));
        EDV_TRY(motion_module_bwd(2, d_p[4], h3 * w3, Fe));
        EDV_TRY(fusion_bwd(4, d_p[4], r[4], nullptr, h4, w4, h3, w3, d_r[4], nullptr));
        return 0;
    }
    int levels_bwd() {  // layerN_rn and motion modules 0 / 1: gradient of the four resized levels
        const int *oc = cfg.out_channels;
        const int hs_[5] = {0, h1, h2, h3, h4}, ws_[5] = {0, w1, w2, w3, w4};
        for (int j = 1; j <= 4; ++j) {
            EDV_TRY(wsbuf("g.l" + std::to_string(j), (size_t)F * hs_[j] * ws_[j] * oc[j - 1], &d_l[j]));
            EDV_TRY(dconv3(d_r[j], hs_[j], ws_[j], Fe, "head.scratch.layer" + std::to_string(j) + "_rn", oc[j - 1], d_l[j]));
        }
        EDV_TRY(motion_module_bwd(0, d_l[3], h3 * w3, oc[2]));
        EDV_TRY(motion_module_bwd(1, d_l[4], h4 * w4, oc[3]));
        return 0;
    }
    // reassemble and projects (with use_clstoken the readout too): gradient of the four taps
    int reassemble_bwd(bool enc) {
        const int *oc = cfg.out_channels;
        const int hs_[5] = {0, h1, h2, h3, h4}, ws_[5] = {0, w1, w2, w3, w4};
        const long long MP = (long long)F * P0;
        const bool hb = c->grad_head_bias;
        float *d_pj;
        {
            int mx = oc[0];
            for (int j = 1; j < 4; ++j) mx = oc[j] > mx ? oc[j] : mx;
            EDV_TRY(wsbuf("g.pj", (size_t)MP * mx, &d_pj));
        }
        for (int j = 0; j < 4; ++j) {
            EDV_TRY(wsbuf("g.tap" + std::to_string(j), (size_t)MP * D, &d_tap[j]));
            if (hb && j != 2) EDV_TRY(wsbuf("g.pj" + std::to_string(j), (size_t)MP * oc[j], &d_pj));  // projects[j]'s dY stays live for its bias
            const float *src = d_pj;
            if (j < 2) {
                const int s = j == 0 ? 4 : 2;
                float *A;
                EDV_TRY(wsbuf("g.unsh", (size_t)MP * s * s * oc[j], &A));
                EDV_TRY(pixel_unshuffle(d_l[j + 1], A, F, ph, pw, oc[j], s, st));
                EDV_TRY(dgemm(A, MP, s * s * oc[j], "head.resize_layers." + std::to_string(j), oc[j], d_pj));
            } else if (j == 2) {
                src = d_l[3];
            } else {
                // stride-2 input gradient = stride-1 input-gradient convolution of the zero-inserted dY (MFMA path; the
                // direct kernel conv3x3_s2_bwd took 2.2 ms here and stays as the unit-test reference of this identity)
                float *z;
                EDV_TRY(wsbuf("g.dil", (size_t)MP * oc[3], &z));
                EDV_TRY(dilate2(d_l[4], z, F, ph, pw, oc[3], st));
                EDV_TRY(dconv3(z, ph, pw, oc[3], "head.resize_layers.3", oc[3], d_pj));
            }
            if (hb) {  // resize_layers.{0,1,3}: dY of the transposed / stride-2 convolution = d_l; projects[j]: dY = src
                if (j != 2) EDV_TRY(bias_grad("head.resize_layers." + std::to_string(j) + ".bias", d_l[j + 1], (long long)F * hs_[j + 1] * ws_[j + 1], oc[j]));
                EDV_TRY(bias_grad("head.projects." + std::to_string(j) + ".bias", src, MP, oc[j]));
            }
            if (enc || (hb && cfg.use_clstoken)) EDV_TRY(dgemm(src, MP, oc[j], "head.projects." + std::to_string(j), D, d_tap[j]));
            if (cfg.use_clstoken) {
                // projects[j] read GELU(W1 tap + (W2 cls + b)) (dpt_pyramid.py:54-57): through the GELU, W1 back to the patch rows,
                // the per-frame sums of the pre-activation gradient through W2 back to the frame's cls row of the tap
                const std::string rp = "head.readout_projects." + std::to_string(j) + ".0";
                const float *pre;
                float *dpre, *dfb, *part;
                EDV_TRY(saved("ro" + std::to_string(j) + ".pre", &pre));
                EDV_TRY(wsbuf(hb ? "g.ro.dpre" + std::to_string(j) : std::string("g.ro.dpre"), (size_t)MP * D, &dpre));
                EDV_TRY(ew_bwd(d_tap[j], pre, nullptr, dpre, MP * D, 1, st));
                if (hb) EDV_TRY(bias_grad(rp + ".bias", dpre, MP, D));  // the pre-GELU gradient over the patch rows
                c->launches += 1;
                if (enc) {
                    EDV_TRY(wsbuf("g.ro.dfb", (size_t)F * D, &dfb));
                    EDV_TRY(wsbuf("g.ro.part", (size_t)TALL_SPLITS * D, &part));
                    EDV_TRY(wsbuf("g.tapcls" + std::to_string(j), (size_t)F * D, &d_tapcls[j]));
                    for (int f = 0; f < F; ++f) EDV_TRY(col_dot(dpre + (size_t)f * P0 * D, nullptr, P0, D, nullptr, part, dfb + (size_t)f * D, st));
                    EDV_TRY(dgemm(dpre, MP, D, rp + ".w1", D, d_tap[j]));
                    EDV_TRY(dgemm(dfb, F, D, rp + ".w2", D, d_tapcls[j]));
                    c->launches += 2 + 2 * F;
                }
            }
        }
        c->launches += 12;
        return 0;
    }
    int encoder_bwd() {
        const long long MT = (long long)F * ntok, MP = (long long)F * P0;
        const bool eb = c->grad_enc_bias;
        if (eb) {  // pretrained.norm.bias: the final norm's dy at all four taps and, with use_clstoken, at every frame's token 0
            std::vector<BiasSrc> srcs;
            for (int j = 0; j < 4; ++j) srcs.push_back(BiasSrc{d_tap[j], MP, D, identity_map()});
            if (cfg.use_clstoken)
                for (int j = 0; j < 4; ++j) srcs.push_back(BiasSrc{d_tapcls[j], (long long)F, D, identity_map()});
            EDV_TRY(bias_grad("pretrained.norm.bias", srcs, D));
        }

        if (!eb) EDV_TRY(bias_flush());  // the head's bias jobs (only encoder jobs share the encoder's flushes)
        float *dxt, *t1, *t3, *t4, *delta, *lws;
        EDV_TRY(wsbuf("g.xt", (size_t)MT * D, &dxt));
        EDV_TRY(wsbuf("g.e1", (size_t)MT * D, &t1));
        EDV_TRY(wsbuf("g.e3", (size_t)MT * 3 * D, &t3));
        EDV_TRY(wsbuf("g.e4", (size_t)MT * 4 * D, &t4));
        EDV_TRY(wsbuf("g.delta", (size_t)F * heads * ntok, &delta));
        float *abws = nullptr;
        const size_t abws_n = attn_spatial_bwd_workspace(F, ntok, heads);
        if (abws_n) EDV_TRY(wsbuf("g.attbws", abws_n, &abws));
        const int rank = cfg.lora_rank;
        const bool lora = cfg.lora_type != EDV_LORA_NONE && c->grad_encoder;
        const size_t lws_n = lora_ws_n;
        lws = lora_ws;
        EDV_HIP(hipMemsetAsync(dxt, 0, (size_t)MT * D * sizeof(float), st));
        // lora_alpha / r (endodav.py:108-117).  dash: the gradient of lora_A / lora_B is LoRA's in both phases -- past the warm-up the
        // extra term U_top diag(lora_index) Vt_top is part of the folded (frozen) weight the input gradients already use
        const float lscale = (cfg.lora_type == EDV_LORA_LORA || cfg.lora_type == EDV_LORA_DASH) ? 2.0f : 1.0f;
        const float *nw;
        EDV_TRY(param("pretrained.norm.weight", &nw));
        int tapj = 3;
        for (int i = depth - 1; i >= 0; --i) {
            const std::string bp = "pretrained.blocks." + std::to_string(i), is = "." + std::to_string(i);
            const float *x_in, *x_mid, *x_out, *xn2, *qkv, *att, *lse, *pre, *hid, *w2;
            EDV_TRY(saved("t.x." + std::to_string(i), &x_in));
            EDV_TRY(saved("t.x." + std::to_string(i + 1), &x_out));
            EDV_TRY(saved("t.xmid" + is, &x_mid));
            EDV_TRY(saved("t.xn2" + is, &xn2));
            EDV_TRY(saved("t.qkv" + is, &qkv));
            EDV_TRY(saved("t.att" + is, &att));
            EDV_TRY(saved("t.lse" + is, &lse));
            EDV_TRY(saved("t.pre" + is, &pre));
            EDV_TRY(saved("t.hid" + is, &hid));
            if (tapj >= 0 && cfg.taps[tapj] == i) {  // tap = norm(x_out) on the patch rows (vision_transformer.py:317-321)
                EDV_TRY(layernorm_bwd(x_out, RowMap{P0, ntok, c0}, nw, d_tap[tapj], identity_map(), dxt, RowMap{P0, ntok, c0}, MP, D, 1e-6f, true, st));
                if (cfg.use_clstoken)  // the readout's class-token input: the final norm of token 0 of every frame (vision_transformer.py:322-324)
                    EDV_TRY(layernorm_bwd(x_out, RowMap{1, ntok, 0}, nw, d_tapcls[tapj], identity_map(), dxt, RowMap{1, ntok, 0}, F, D, 1e-6f, true, st));
                --tapj;
            }
            if (cfg.residual_mask & (1u << i)) EDV_TRY(res_bottleneck_bwd(i, dxt));  // x_out = x' + residual_(x' patch rows)
            // x' = x_mid + ls2 * fc2(gelu(fc1(norm2(x_mid))))
            if (lora) EDV_TRY(lora_step(bp + ".mlp.fc2", hid, 4 * D, dxt, D, MT, rank, lscale, bp + ".ls2.gamma", lws, lws_n));
            EDV_TRY(dgemm(dxt, MT, D, bp + ".mlp.fc2", 4 * D, t4));
            EDV_TRY(ew_bwd(t4, pre, nullptr, t4, MT * 4 * D, 1, st));
            if (lora) EDV_TRY(lora_step(bp + ".mlp.fc1", xn2, D, t4, 4 * D, MT, rank, lscale, "", lws, lws_n));
            EDV_TRY(dgemm(t4, MT, 4 * D, bp + ".mlp.fc1", D, t1));
            if (eb) {  // dxt is about to gain norm2's input gradient, t1 / t4 are reused: the MLP's biases now
                const float *g2;
                EDV_TRY(param(bp + ".ls2.gamma", &g2));
                EDV_TRY(bias_grad(bp + ".mlp.fc2.bias", dxt, MT, D, g2));  // LayerScale multiplies the bias (folded into W and the epilogue)
                EDV_TRY(bias_grad(bp + ".mlp.fc1.bias", t4, MT, 4 * D));    // the pre-activation gradient
                EDV_TRY(bias_grad(bp + ".norm2.bias", t1, MT, D));
                EDV_TRY(bias_flush());
            }
            EDV_TRY(param(bp + ".norm2.weight", &w2));
            EDV_TRY(layernorm_bwd(x_mid, identity_map(), w2, t1, identity_map(), dxt, identity_map(), MT, D, 1e-6f, true, st));
            if (i == 0 && !eb) break;  // nothing trainable below block 0's MLP
            // x_mid = x_in + ls1 * proj(attn(qkv(norm1(x_in))))
            EDV_TRY(dgemm(dxt, MT, D, bp + ".attn.proj", D, t1));
            {
                Bracket b_(c, KC_ATTN_SPATIAL_BWD, st);  // both passes (dQ; dK, dV) + their combine launches: seven N x N x 64 products per head
                EDV_TRY(attn_spatial_bwd(qkv, att, t1, lse, delta, t3, F, ntok, heads, abws, abws_n, st));
            }
            EDV_TRY(dgemm(t3, MT, 3 * D, bp + ".attn.qkv", D, t1));
            if (eb) {
                const float *g1;
                EDV_TRY(param(bp + ".ls1.gamma", &g1));
                EDV_TRY(bias_grad(bp + ".attn.proj.bias", dxt, MT, D, g1));
                EDV_TRY(bias_grad(bp + ".attn.qkv.bias", t3, MT, 3 * D));
                EDV_TRY(bias_grad(bp + ".norm1.bias", t1, MT, D));
                EDV_TRY(bias_flush());
            }
            EDV_TRY(param(bp + ".norm1.weight", &w2));
            EDV_TRY(layernorm_bwd(x_in, identity_map(), w2, t1, identity_map(), dxt, identity_map(), MT, D, 1e-6f, true, st));
            c->launches += 6;
            if (i == 0)  // bias="all" went on through block 0: x_0 = patch_embed(x) + pos on the patch rows, the cls row does not see the bias
                EDV_TRY(bias_grad("pretrained.patch_embed.proj.bias", {BiasSrc{dxt, MP, D, RowMap{P0, ntok, c0}}}, D));
        }
        return 0;
    }

    int backward(const float *disp0, const float *const g_[4]) {
        EDV_CHECK(c->train && c->have_saved, "edv_backward needs the activations of a forward run under edv_set_train(1): none are kept (no such forward yet, "
                                             "a backward already consumed them, or an inference forward on this context ran in between)");
        if (!c->train_prepared) EDV_TRY(run_prepare_train(c, st));
        set_geometry(c->F / c->T, c->T);
        EDV_CHECK(F == c->F && ph == c->ph && pw == c->pw && ntok == c->ntok, "the clip geometry the forward left in the context is not the configuration's");
        g = g_;
        EDV_TRY(workspaces());
        EDV_TRY(bias_begin());
        EDV_TRY(wsbuf("g.p1", (size_t)F * h0 * w0 * Fe, &d_p[1]));
        EDV_TRY(cfg.conv_head ? head_depth_bwd(0, h0, w0, "p1", d_p[1], false) : vda_head_bwd(disp0));
        EDV_TRY(fuse_bwd());
        EDV_TRY(levels_bwd());
        const bool res_grads = c->grad_res && cfg.residual_mask != 0;
        const bool enc = (c->grad_encoder && cfg.lora_type != EDV_LORA_NONE) || res_grads || c->grad_enc_bias;  // anything trainable below the head
        // neither: the temporal-only phase stops here.  Head biases only: the backward stops at the head.
        if (enc || c->grad_head_bias) EDV_TRY(reassemble_bwd(enc));
        if (enc) EDV_TRY(encoder_bwd());
        EDV_TRY(bias_finish());
        c->have_saved = false;
        return 0;
    }
    // Linear_SSB (mylora/layers.py:396-430), y = gamma * (((x * a) W^T) * b + bias):  with z = (x * a) W^T and
    // u = (G * gamma * b) W:   db[n] = gamma[n] sum_m G[m,n] z[m,n],   da[k] = sum_m x[m,k] u[m,k].
    // Two extra GEMMs per linear (a and b may pass through zero, so neither is recovered by dividing y or dX).
    int ssb_step(const std::string &p, const float *X, int nin, const float *G, int nout, long long M, const std::string &gamma_name) {
        const float *W, *a, *b, *gam = nullptr;
        EDV_TRY(param(p + ".weight", &W, 2));
        EDV_TRY(param(p + ".lora_A", &a));
        EDV_TRY(param(p + ".lora_B", &b));
        if (!gamma_name.empty()) EDV_TRY(param(gamma_name, &gam));
        float *Wa, *gb, *Tu, *z, *u, *part, *da, *db;
        EDV_TRY(wsbuf("g.ssb.wa", (size_t)nout * nin, &Wa));
        EDV_TRY(wsbuf("g.ssb.tu", (size_t)nout * nin, &Tu));
        EDV_TRY(wsbuf("g.ssb.gb", (size_t)nout, &gb));
        EDV_TRY(wsbuf("g.ssb.z", (size_t)M * nout, &z));
        EDV_TRY(wsbuf("g.ssb.u", (size_t)M * nin, &u));
        EDV_TRY(wsbuf("g.ssb.part", (size_t)TALL_SPLITS * (nin > nout ? nin : nout), &part));
        EDV_TRY(gradbuf(p + ".lora_A", (size_t)nin, &da));
        EDV_TRY(gradbuf(p + ".lora_B", (size_t)nout, &db));
        EDV_TRY(ssb_prep(W, a, b, gam, Wa, gb, nout, nin, st));
        EDV_TRY(transpose_scale(W, nin, gb, Tu, nout, nin, st));          // Tu [nin, nout] = (gamma b W)^T
        EDV_TRY(linear(X, M, nin, Wa, nout, nullptr, z));                 // z = (x * a) W^T
        EDV_TRY(linear(G, M, nout, Tu, nin, nullptr, u));                 // u = (G gamma b) W
        EDV_TRY(col_dot(G, z, M, nout, gam, part, db, st));
        EDV_TRY(col_dot(X, u, M, nin, nullptr, part, da, st));
        c->launches += 6;
        return 0;
    }
    // gradients of the LoRA factors of one linear into c->grads["<p>.lora_A"] ... (mylora/layers.py:148-157, 384-393)
    int lora_step(const std::string &p, const float *X, int nin, const float *G, int nout, long long M, int r, float s, const std::string &gamma_name,
                  float *lws, size_t lws_n) {
        if (!has(p + ".lora_A")) return 0;
        if (cfg.lora_type == EDV_LORA_SSB) return ssb_step(p, X, nin, G, nout, M, gamma_name);
        const float *A, *Bm, *U = nullptr, *V = nullptr, *gam = nullptr;
        EDV_TRY(param(p + ".lora_A", &A));
        EDV_TRY(param(p + ".lora_B", &Bm));
        if (cfg.lora_type == EDV_LORA_DVLORA) {
            EDV_TRY(param(p + ".lora_U", &U));
            EDV_TRY(param(p + ".lora_V", &V));
        }
        if (!gamma_name.empty()) EDV_TRY(param(gamma_name, &gam));
        float *dA, *dB, *dU = nullptr, *dV = nullptr;
        EDV_TRY(gradbuf(p + ".lora_A", (size_t)r * nin, &dA));
        EDV_TRY(gradbuf(p + ".lora_B", (size_t)r * nout, &dB));
        if (U) {
            EDV_TRY(gradbuf(p + ".lora_U", (size_t)r, &dU));
            EDV_TRY(gradbuf(p + ".lora_V", (size_t)nout, &dV));
        }
        c->launches += 8;
        EDV_TRY(lora_grads(X, nin, G, nout, M, nin, nout, r, A, Bm, U, V, s, gam, lws, lws_n, dA, dB, dU, dV, st));
        if (cfg.lora_type == EDV_LORA_DASH && cfg.dash_active) {
            // DashLinear past its warm-up adds x (U_top diag(idx) Vt_top)^T (mylora/layers.py:580-582) and frees lora_index:
            // d idx[j] = sum_m ((G * gamma) U_top)[m, j] (x Vt_top^T)[m, j] -- two skinny products and a column dot
            const float *Ut, *Vt;
            EDV_TRY(param(p + ".weight_u_top", &Ut));
            EDV_TRY(param(p + ".weight_vt_top", &Vt));
            const int ri = (int)c->params[p + ".lora_index"].shape[0];
            float *utg, *t1, *t2, *part, *didx;
            EDV_TRY(wsbuf("g.dash.utg", (size_t)ri * nout, &utg));
            EDV_TRY(wsbuf("g.dash.t1", (size_t)M * ri, &t1));
            EDV_TRY(wsbuf("g.dash.t2", (size_t)M * ri, &t2));
            EDV_TRY(wsbuf("g.dash.part", (size_t)TALL_SPLITS * ri, &part));
            EDV_TRY(gradbuf(p + ".lora_index", (size_t)ri, &didx));
            EDV_TRY(transpose_scale(Ut, ri, gam, utg, nout, ri, st));  // [nout, ri] -> [ri, nout], rows scaled by gamma
            EDV_TRY(skinny_xwt(G, M, nout, nout, utg, ri, t1, st));
            EDV_TRY(skinny_xwt(X, M, nin, nin, Vt, ri, t2, st));
            EDV_TRY(col_dot(t1, t2, M, ri, nullptr, part, didx, st));
            c->launches += 5;
        }
        return 0;
    }
};

}  // namespace

namespace edv {
int run_backward(edv_ctx *c, hipStream_t st, const float *disp0, const float *const g[4]) { return Backward(c, st).backward(disp0, g); }
}  // namespace edv
