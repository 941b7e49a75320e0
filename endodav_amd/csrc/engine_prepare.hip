// Weights as the kernels read them: LoRA folds, packed / BatchNorm-folded convolutions, bf16x6 planes (edv_prepare, edv_refresh_lora,
// edv_set_products) and the transposed / flipped copies the input-gradient GEMMs of the backward use (prepare_train).
#include "engine.hpp"

namespace {

struct Prepare : Run {
    using Run::Run;

    int fold_linear(const std::string &p, bool lora_here) {
        // result registered under packed[p + ".weight"]; a plain pointer alias when no LoRA applies
        const float *W;
        EDV_TRY(param(p + ".weight", &W, 2));
        const Param &pw_ = c->params[p + ".weight"];
        const int nout = (int)pw_.shape[0], nin = (int)pw_.shape[1];
        if (!lora_here || cfg.lora_type == EDV_LORA_NONE || !has(p + ".lora_A")) return 0;
        float *out;
        EDV_TRY(pk(p + ".weight", (size_t)nout * nin, &out));
        const float *A, *Bm;
        EDV_TRY(param(p + ".lora_A", &A));
        EDV_TRY(param(p + ".lora_B", &Bm));
        const int r = cfg.lora_rank;
        switch (cfg.lora_type) {
            case EDV_LORA_LORA:  // lora_alpha = 2r  (endodav.py:111-112)
                return fold_lora(W, A, Bm, nullptr, nullptr, 2.0f, out, nout, nin, r, st);
            case EDV_LORA_DVLORA: {  // lora_alpha = r  (endodav.py:108-109)
                const float *U, *V;
                EDV_TRY(param(p + ".lora_U", &U));
                EDV_TRY(param(p + ".lora_V", &V));
                return fold_lora(W, A, Bm, U, V, 1.0f, out, nout, nin, r, st);
            }
            case EDV_LORA_SSB:
                return fold_ssb(W, A, Bm, out, nout, nin, st);
            case EDV_LORA_DASH: {
                EDV_TRY(fold_lora(W, A, Bm, nullptr, nullptr, 2.0f, out, nout, nin, r, st));
                if (cfg.dash_active) {
                    const float *Ut, *idx, *Vt;
                    EDV_TRY(param(p + ".weight_u_top", &Ut));
                    EDV_TRY(param(p + ".lora_index", &idx));
                    EDV_TRY(param(p + ".weight_vt_top", &Vt));
                    const int ri = (int)c->params[p + ".lora_index"].shape[0];
                    return fold_dash(Ut, idx, Vt, out, nout, nin, ri, st);
                }
                return 0;
            }
            default:
                EDV_CHECK(false, "unknown lora_type");
        }
        return 0;
    }
    // bf16 planes of an encoder linear's effective weight (after the LoRA fold) for gemm_x6.hip
    int make_x6(const std::string &p) {
        const float *W;
        EDV_TRY(lin_w(p, &W));
        const Param &q = c->params[p + ".weight"];
        const int nout = (int)q.shape[0], nin = (int)q.shape[1];
        if (nin % 16 != 0 || nout < 64) return 0;
        float *pl;
        EDV_TRY(pk(p + ".x6", (gemm_x6_planes_bytes(nout, nin) + 3) / 4, &pl));
        EDV_TRY(gemm_x6_split(W, pl, nout, nin, st));
        c->x6[W] = pl;
        return 0;
    }
    int build_x6(bool mlp_only) {
        if (c->products != EDV_PRODUCTS_BF16X6) return 0;
        for (int i = 0; i < depth; ++i) {
            const std::string bp = "pretrained.blocks." + std::to_string(i);
            if (!mlp_only) {
                EDV_TRY(make_x6(bp + ".attn.qkv"));
                EDV_TRY(make_x6(bp + ".attn.proj"));
            }
            EDV_TRY(make_x6(bp + ".mlp.fc1"));
            EDV_TRY(make_x6(bp + ".mlp.fc2"));
        }
        return 0;
    }
    int pack_c3(const std::string &p) {
        const float *w;
        EDV_TRY(param(p + ".weight", &w, 4));
        const Param &q = c->params[p + ".weight"];
        EDV_CHECK(q.shape[2] == 3 && q.shape[3] == 3, "expected a 3x3 kernel: " + p);
        float *out;
        EDV_TRY(pk(p + ".weight", (size_t)q.numel(), &out));
        return pack_conv3x3(w, out, (int)q.shape[0], (int)q.shape[1], st);
    }
    // eval-mode BatchNorm after convolution `conv` (util/blocks.py:80-86) folded into its packed weight and a packed bias
    int fold_bn_into(const std::string &conv, const std::string &bn) {
        const float *b, *g, *beta, *mean, *var;
        EDV_TRY(param(conv + ".bias", &b));
        EDV_TRY(param(bn + ".weight", &g));
        EDV_TRY(param(bn + ".bias", &beta));
        EDV_TRY(param(bn + ".running_mean", &mean));
        EDV_TRY(param(bn + ".running_var", &var));
        const Param &q = c->params[conv + ".weight"];
        const int nout = (int)q.shape[0], K = (int)(q.numel() / q.shape[0]);
        float *w, *bo;
        EDV_TRY(pk(conv + ".weight", (size_t)q.numel(), &w));
        EDV_TRY(pk(conv + ".bias", (size_t)nout, &bo));
        return fold_bn(w, b, g, beta, mean, var, 1e-5f, bo, nout, K, st);
    }

    // The packings that embed a bias (pack_convT replicates it s^2 times, fold_bn folds the BatchNorm into it, pack_geglu interleaves
    // it): edv_prepare builds them, edv_refresh_lora rebuilds them, so that a changed bias reaches the next forward either way.
    int pack_resize() {  // ConvTranspose k=s -> GEMM weights
        const int *oc = cfg.out_channels;
        const int ss[2] = {4, 2};
        for (int j = 0; j < 2; ++j) {
            const std::string p = "head.resize_layers." + std::to_string(j);
            const float *w, *b;
            EDV_TRY(param(p + ".weight", &w, 4));
            EDV_TRY(param(p + ".bias", &b));
            float *wo, *bo;
            EDV_TRY(pk(p + ".weight", (size_t)ss[j] * ss[j] * oc[j] * oc[j], &wo));
            EDV_TRY(pk(p + ".bias", (size_t)ss[j] * ss[j] * oc[j], &bo));
            EDV_TRY(pack_convT(w, wo, b, bo, oc[j], oc[j], ss[j], st));
        }
        return 0;
    }
    // the ResidualConvUnits' convolutions; bn_only: just those whose packing folds a BatchNorm (and with it the conv bias)
    int pack_rcus(bool bn_only) {
        if (bn_only && !cfg.use_bn) return 0;
        for (int j = 1; j <= 4; ++j)
            for (int u = 1; u <= 2; ++u) {
                if (j == 4 && u == 1) continue;  // refinenet4.resConfUnit1 is never reached (dpt_pyramid.py:81)
                const std::string p = "head.scratch.refinenet" + std::to_string(j) + ".resConfUnit" + std::to_string(u);
                EDV_TRY(pack_c3(p + ".conv1"));
                EDV_TRY(pack_c3(p + ".conv2"));
                if (cfg.use_bn) {
                    EDV_TRY(fold_bn_into(p + ".conv1", p + ".bn1"));
                    EDV_TRY(fold_bn_into(p + ".conv2", p + ".bn2"));
                }
            }
        return 0;
    }
    int pack_geglus() {  // interleaved copy of ff.net.0.proj for the fused GEGLU launch of the inference forward
        const int *oc = cfg.out_channels;
        const int mmC[4] = {oc[2], oc[3], Fe, Fe};
        for (int m = 0; m < 4; ++m) {
            const std::string tb = "head.motion_modules." + std::to_string(m) + ".temporal_transformer.transformer_blocks.0";
            const int C = mmC[m];
            if ((8 * C) % 64 == 0 && C % 32 == 0) {
                const float *w0, *b0;
                float *wi, *bi;
                EDV_TRY(param(tb + ".ff.net.0.proj.weight", &w0, 2));
                EDV_TRY(param(tb + ".ff.net.0.proj.bias", &b0));
                EDV_TRY(pk(tb + ".ff.net.0.geglu.w", (size_t)8 * C * C, &wi));
                EDV_TRY(pk(tb + ".ff.net.0.geglu.b", (size_t)8 * C, &bi));
                EDV_TRY(pack_geglu(w0, b0, wi, bi, 8 * C, C, st));
            }
        }
        return 0;
    }

    // the 3x3 convolutions of the output heads (trainable: HeadDepth heads, or scratch.output_conv* with --train_output_conv)
    std::vector<std::string> output_convs() const {
        if (!cfg.conv_head) return {"head.scratch.output_conv1", "head.scratch.output_conv2.0"};
        std::vector<std::string> v;
        for (int k = 1; k <= 4; ++k)
            for (const char *l : {".head.0", ".head.2"}) v.push_back("head.conv_depth_" + std::to_string(k) + l);
        return v;
    }
    int prepare() {
        c->launches = 0;
        {   // patch-embed weight [D, 3*14*14 = 588] with its rows zero-padded to PE_K = 608 = 19 x 32: the im2col GEMM then runs on the
            // LDS-DMA kernel (K % 32 == 0) instead of the register-staged one (89 -> 57 us at T=8)
            const float *w;
            float *wp;
            EDV_TRY(param("pretrained.patch_embed.proj.weight", &w, 4));
            EDV_TRY(pk("pretrained.patch_embed.proj.weight", (size_t)D * PE_K, &wp));
            EDV_HIP(hipMemsetAsync(wp, 0, (size_t)D * PE_K * sizeof(float), st));
            EDV_HIP(hipMemcpy2DAsync(wp, PE_K * sizeof(float), w, 588 * sizeof(float), 588 * sizeof(float), (size_t)D, hipMemcpyDeviceToDevice, st));
        }
        for (int i = 0; i < depth; ++i) {
            const std::string b = "pretrained.blocks." + std::to_string(i) + ".mlp.";
            EDV_TRY(fold_linear(b + "fc1", true));
            EDV_TRY(fold_linear(b + "fc2", true));
        }
        for (int i = 0; i < depth; ++i)
            if (cfg.residual_mask & (1u << i)) EDV_TRY(pack_c3("pretrained.blocks." + std::to_string(i) + ".residual_.conv2"));
        const int *oc = cfg.out_channels;
        EDV_TRY(pack_resize());
        EDV_TRY(pack_c3("head.resize_layers.3"));
        for (int j = 1; j <= 4; ++j) EDV_TRY(pack_c3("head.scratch.layer" + std::to_string(j) + "_rn"));
        EDV_TRY(pack_rcus(false));
        for (const std::string &cv : output_convs()) EDV_TRY(pack_c3(cv));
        const int mmC[4] = {oc[2], oc[3], Fe, Fe};
        for (int m = 0; m < 4; ++m) {
            const std::string tb = "head.motion_modules." + std::to_string(m) + ".temporal_transformer.transformer_blocks.0";
            const int C = mmC[m];
            for (int a = 0; a < 2; ++a) {
                const std::string ab = tb + ".attention_blocks." + std::to_string(a);
                float *qkvw;
                EDV_TRY(pk(ab + ".qkv", (size_t)3 * C * C, &qkvw));
                const char *names[3] = {".to_q.weight", ".to_k.weight", ".to_v.weight"};
                for (int j = 0; j < 3; ++j) {
                    const float *w;
                    EDV_TRY(param(ab + names[j], &w, 2));
                    EDV_TRY(copy_f32(w, qkvw + (size_t)j * C * C, (long long)C * C, st));
                }
            }
            EDV_TRY(fold_linear(tb + ".ff.net.2", cfg.temporal_lora != 0));
        }
        EDV_TRY(pack_geglus());
        c->x6.clear();
        EDV_TRY(build_x6(false));
        c->prepared = true;
        c->train_prepared = false;  // the folded LoRA weights changed: their transposes are stale
        return 0;
    }

    // After an optimizer step only trainable tensors changed: re-fold the linears that carry LoRA factors and re-pack the trainable
    // convolutions (HeadDepth heads or scratch.output_conv*, residual blocks) -- and, once the backward has run, their transposed /
    // flipped copies -- instead of re-packing every frozen weight as edv_prepare does.
    int refresh_lora() {
        EDV_CHECK(c->prepared, "edv_prepare has not run");
        for (int i = 0; i < depth; ++i) {
            const std::string bp = "pretrained.blocks." + std::to_string(i);
            EDV_TRY(fold_linear(bp + ".mlp.fc1", true));
            EDV_TRY(fold_linear(bp + ".mlp.fc2", true));
            if (c->train_prepared) {
                const float *g2;
                EDV_TRY(param(bp + ".ls2.gamma", &g2));
                EDV_TRY(make_t_lin(bp + ".mlp.fc1"));
                EDV_TRY(make_t_lin(bp + ".mlp.fc2", g2));
            }
            if (cfg.residual_mask & (1u << i)) {
                EDV_TRY(pack_c3(bp + ".residual_.conv2"));
                if (c->train_prepared) {
                    EDV_TRY(make_t_lin(bp + ".residual_.conv1"));
                    EDV_TRY(make_t_lin(bp + ".residual_.conv3"));
                    EDV_TRY(make_b_c3(bp + ".residual_.conv2"));
                }
            }
        }
        if (cfg.temporal_lora)
            for (int m = 0; m < 4; ++m) {
                const std::string p = "head.motion_modules." + std::to_string(m) + ".temporal_transformer.transformer_blocks.0.ff.net.2";
                EDV_TRY(fold_linear(p, true));
                if (c->train_prepared) EDV_TRY(make_t_lin(p));
            }
        for (const std::string &cv : output_convs()) {
            EDV_TRY(pack_c3(cv));
            if (c->train_prepared) EDV_TRY(make_b_c3(cv));
        }
        // bias="all": every bias may have changed.  Most are read straight from the bound tensor; these three packings copy one.
        EDV_TRY(pack_resize());
        EDV_TRY(pack_rcus(true));
        EDV_TRY(pack_geglus());
        EDV_TRY(build_x6(true));  // fc1 / fc2 carry the factors: their planes follow the fold
        return 0;
    }

    // transposed (NT-form) weight of dX = (dY * gamma) W, cached under "T." + key
    int make_t(const std::string &key, const float *W, int ldw, int N, int K, const float *gamma) {
        float *wt;
        EDV_TRY(pk("T." + key, (size_t)N * K, &wt));
        return transpose_scale(W, ldw, gamma, wt, N, K, st);
    }
    int make_t_lin(const std::string &p, const float *gamma = nullptr) {
        const float *W;
        EDV_TRY(lin_w(p, &W));
        const Param &q = c->params[p + ".weight"];
        EDV_CHECK(q.shape.size() >= 2, "rank of " + p);
        long long in = 1;
        for (size_t k = 1; k < q.shape.size(); ++k) in *= q.shape[k];
        return make_t(p, W, (int)in, (int)q.shape[0], (int)in, gamma);
    }
    int make_b_c3(const std::string &p) {  // flipped, in/out-swapped packed weight of the stride-1 input-gradient convolution
        const float *w;
        EDV_TRY(param(p + ".weight", &w, 4));
        const Param &q = c->params[p + ".weight"];
        float *out;
        EDV_TRY(pk("B." + p, (size_t)q.numel(), &out));
        return pack_conv3x3_bwd(w, out, (int)q.shape[0], (int)q.shape[1], st);
    }
    int prepare_train() {
        EDV_CHECK(!cfg.use_bn, "the fine-tune step with use_bn=True is not built (train-mode BatchNorm uses batch statistics)");
        EDV_CHECK(c->prepared, "edv_prepare has not run");
        const int *oc = cfg.out_channels;
        for (int i = 0; i < depth; ++i) {
            const std::string bp = "pretrained.blocks." + std::to_string(i);
            const float *g1, *g2;
            EDV_TRY(param(bp + ".ls1.gamma", &g1));
            EDV_TRY(param(bp + ".ls2.gamma", &g2));
            EDV_TRY(make_t_lin(bp + ".attn.qkv"));
            EDV_TRY(make_t_lin(bp + ".attn.proj", g1));
            EDV_TRY(make_t_lin(bp + ".mlp.fc1"));
            EDV_TRY(make_t_lin(bp + ".mlp.fc2", g2));
        }
        for (int i = 0; i < depth; ++i)
            if (cfg.residual_mask & (1u << i)) {
                const std::string rp = "pretrained.blocks." + std::to_string(i) + ".residual_";
                EDV_TRY(make_t_lin(rp + ".conv1"));
                EDV_TRY(make_t_lin(rp + ".conv3"));
                EDV_TRY(make_b_c3(rp + ".conv2"));
            }
        for (int j = 0; j < 4; ++j) EDV_TRY(make_t_lin("head.projects." + std::to_string(j)));
        if (cfg.use_clstoken)
            for (int j = 0; j < 4; ++j) {  // readout_projects[j].0.weight = [W1 | W2] (dpt.py:92-98): both halves, transposed
                const std::string rp = "head.readout_projects." + std::to_string(j) + ".0";
                const float *rw;
                EDV_TRY(param(rp + ".weight", &rw, 2));
                EDV_TRY(make_t(rp + ".w1", rw, 2 * D, D, D, nullptr));
                EDV_TRY(make_t(rp + ".w2", rw + D, 2 * D, D, D, nullptr));
            }
        for (int j = 0; j < 2; ++j) {
            const std::string rp = "head.resize_layers." + std::to_string(j);
            const int s2 = (j == 0 ? 16 : 4);
            const float *wp;
            EDV_TRY(packedw(rp + ".weight", &wp));
            EDV_TRY(make_t(rp, wp, oc[j], s2 * oc[j], oc[j], nullptr));
        }
        for (int j = 1; j <= 4; ++j) EDV_TRY(make_b_c3("head.scratch.layer" + std::to_string(j) + "_rn"));
        EDV_TRY(make_b_c3("head.resize_layers.3"));
        for (int j = 1; j <= 4; ++j) {
            const std::string p = "head.scratch.refinenet" + std::to_string(j);
            for (int u = 1; u <= 2; ++u) {
                if (j == 4 && u == 1) continue;
                EDV_TRY(make_b_c3(p + ".resConfUnit" + std::to_string(u) + ".conv1"));
                EDV_TRY(make_b_c3(p + ".resConfUnit" + std::to_string(u) + ".conv2"));
            }
            EDV_TRY(make_t_lin(p + ".out_conv"));
        }
        for (const std::string &cv : output_convs()) EDV_TRY(make_b_c3(cv));
        const int mmC[4] = {oc[2], oc[3], Fe, Fe};
        for (int m = 0; m < 4; ++m) {
            const std::string p = "head.motion_modules." + std::to_string(m) + ".temporal_transformer";
            const std::string tb = p + ".transformer_blocks.0";
            const int C = mmC[m];
            EDV_TRY(make_t_lin(p + ".proj_in"));
            EDV_TRY(make_t_lin(p + ".proj_out"));
            for (int a = 0; a < 2; ++a) {
                const std::string ab = tb + ".attention_blocks." + std::to_string(a);
                const float *wq;
                EDV_TRY(packedw(ab + ".qkv", &wq));
                EDV_TRY(make_t(ab + ".qkv", wq, C, 3 * C, C, nullptr));
                EDV_TRY(make_t_lin(ab + ".to_out.0"));
            }
            EDV_TRY(make_t_lin(tb + ".ff.net.0.proj"));
            EDV_TRY(make_t_lin(tb + ".ff.net.2"));
        }
        c->train_prepared = true;
        return 0;
    }
};

}  // namespace

namespace edv {
int run_prepare(edv_ctx *c, hipStream_t st) { return Prepare(c, st).prepare(); }
int run_refresh_lora(edv_ctx *c, hipStream_t st) { return Prepare(c, st).refresh_lora(); }
int run_build_x6(edv_ctx *c, hipStream_t st) { return Prepare(c, st).build_x6(false); }
int run_prepare_train(edv_ctx *c, hipStream_t st) { return Prepare(c, st).prepare_train(); }
}  // namespace edv
