// The forward: encoder, DPT head, output heads (edv_forward).
//
// Sequences EndoDAV's per-clip forward (reference models/endodav/endodav.py:150-160) as ~25 kernel
// launches per encoder block + ~120 for the DPT head on one HIP stream.  No host sync inside a
// forward once the workspace for a clip geometry exists.  Layouts: encoder activations are
// tokens-major [frames*tokens, D]; head activations channels-last [frames, h, w, C], so that
//   - the 1x1 "projects" convs, proj_in/out and every Linear are plain GEMMs on the same buffers,
//   - the five NCHW<->NLC permutes per motion module (motion_module.py:105,112,121,124,232,295)
//     and the tap permute (dpt_pyramid.py:61) vanish,
//   - temporal attention reaches the frame axis by a constant address stride.
#include "engine.hpp"

namespace {

// While one is alive the Run enqueues on the internal stream `s` with the stream-K workspace region `ws`; its destructor gives the Run back the
// caller's stream, that stream's region and the clip's frame count on every exit path.  An error (EDV_TRY) thus leaves the scope after the
// restore and before anything else is recorded on the caller's stream: edv_forward waits for the internal streams before it reports the error.
struct OnStream {
    Run &r;
    const hipStream_t st;
    float *const skws;
    const int F;
    OnStream(Run &run, hipStream_t s, float *ws) : r(run), st(run.st), skws(run.skws), F(run.F) { r.st = s; r.skws = ws; }
    ~OnStream() { r.st = st; r.skws = skws; r.F = F; }
};

struct Forward : Run {
    using Run::Run;
    std::string rb_suffix;
    int enc_F = 0, enc_f0 = 0;    // all frames of the clip / first frame of the group encoder_range is working on (training buffers hold all frames)
    bool stagger_record = false;  // encoder_range records ev_x[5] after block 0's qkv GEMM (start signal for the next frame group)
    // the buffers one phase of the forward hands to the next: encoder taps; per level j the projection, the resized map and layer(j+1)_rn; path_1..path_4
    float *tap[4], *tapcls[4] = {nullptr, nullptr, nullptr, nullptr}, *pj[4], *lv[4], *rn[4], *path[5], *readout = nullptr, *fbias = nullptr;

    // position table for the current patch grid (vision_transformer.py:186-217)
    int pos_table(const float **out) {
        const float *pos;
        EDV_TRY(param("pretrained.pos_embed", &pos, 3));
        const int Npos = cfg.pos_tokens - 1;
        const int npatch = ntok - 1;
        if (npatch == Npos && cfg.image_h == cfg.image_w) {
            *out = pos;
            return 0;
        }
        const int S = (int)std::lround(std::sqrt((double)Npos));
        EDV_CHECK(S * S == Npos, "pos_embed grid is not square");
        float *tab;
        EDV_TRY(wsbuf("pos_eff", (size_t)ntok * D, &tab));
        // ATen receives scale_factor as double and uses float(1/scale) (UpSample.h compute_scales_value)
        const double sh = ((double)ph + 0.1) / std::sqrt((double)Npos), sw = ((double)pw + 0.1) / std::sqrt((double)Npos);
        EDV_CHECK((int)std::floor(S * sh) == ph && (int)std::floor(S * sw) == pw, "pos-embed resample size mismatch");
        if (c0) EDV_TRY(copy_f32(pos, tab, D, st));
        EDV_TRY(bicubic_pos(pos + D, tab + (size_t)c0 * D, S, D, ph, pw, (float)(1.0 / sh), (float)(1.0 / sw), st));
        c->launches += 2;
        *out = tab;
        return 0;
    }

    int snapshot(const std::string &name, const float *src, size_t n) {
        if (c->capture) {
            float *dst;
            EDV_TRY(wsbuf("stage." + name, n, &dst));
            EDV_TRY(copy_f32(src, dst, (long long)n, st));
            c->stages[name] = {dst, n};
        }
        return 0;
    }

    // ---- motion module, in place on x [F, P, C] channels-last (motion_module.py:102-126,164-177) ----
    // extra (optional, shaped like x): added to the output as well -- the skip branch of the following fusion block
    int motion_module(int m, float *x, int P, int C, const float *extra = nullptr) {
        const std::string p = "head.motion_modules." + std::to_string(m) + ".temporal_transformer";
        const std::string tb = p + ".transformer_blocks.0";
        const long long M = (long long)F * P;
        float *gn, *h, *hn, *qkv3, *att, *ff1, *ff2, *stats;
        // training keeps: the module input, the GroupNorm statistics, h before each of its three residual updates,
        // both q|k|v and the GEGLU input (names tagged with the module index); inference reuses one set of buffers
        // scratch that nobody reads later comes in two sets: "mmb." for module 1, which may run beside module 0 on another stream
        const std::string sc_ = m == 1 ? "mmb." : "mm.";
        const std::string tg = c->train ? "mm" + std::to_string(m) + "." : sc_;
        float *hs[4];  // h after proj_in, after attention 0, after attention 1, after the feed-forward
        const float *xin = x;
        EDV_TRY(wsbuf(sc_ + "gn", (size_t)M * C, &gn));
        EDV_TRY(wsbuf(tg + "h", (size_t)M * C, &h));
        hs[0] = hs[1] = hs[2] = hs[3] = h;
        if (c->train) {
            float *xc;
            EDV_TRY(wsbuf(tg + "xin", (size_t)M * C, &xc));
            EDV_TRY(copy_f32(x, xc, M * C, st));
            xin = xc;
            for (int k = 1; k < 4; ++k) EDV_TRY(wsbuf(tg + "h" + std::to_string(k), (size_t)M * C, &hs[k]));
        }
        EDV_TRY(wsbuf(sc_ + "hn", (size_t)M * C, &hn));
        EDV_TRY(wsbuf(sc_ + "att", (size_t)M * C, &att));
        EDV_TRY(wsbuf(tg + "ff1", (size_t)M * 8 * C, &ff1));
        EDV_TRY(wsbuf(c->train ? tg + "ff2" : sc_ + "ff2", (size_t)M * 4 * C, &ff2));  // input of ff.net.2: its LoRA gradient needs it
        EDV_TRY(wsbuf(tg + "stats", (size_t)F * 32 * 2, &stats));
        const float *w, *b;
        EDV_TRY(param(p + ".norm.weight", &w));
        EDV_TRY(param(p + ".norm.bias", &b));
        // coalesced two-stage statistics for the large maps only: [8,1369,192] 23.3 -> 16.3 us, [8,5476,64] 34.5 -> 18.3 us, but the small ones
        // ([8,361,384] 11.1 -> 14.7 us) lose to the third launch
        float *gnpart = nullptr;
        size_t gnpart_n = 0;
        if ((long long)F * P * C >= 1500000ll) {
            gnpart_n = groupnorm_workspace(F, P, C);
            EDV_TRY(wsbuf(sc_ + "gnpart", gnpart_n, &gnpart));
        }
        {
            HbmScope b_(c, KC_GROUPNORM, st, 8.0 * (double)M * C);  // statistics + apply, 2-3 launches
            EDV_TRY(groupnorm(xin, w, b, gn, stats, F, P, C, 32, 1e-6f, st, gnpart, gnpart_n));
        }
        c->launches += 2;
        EDV_TRY(param(p + ".proj_in.weight", &w));
        EDV_TRY(param(p + ".proj_in.bias", &b));
        EDV_TRY(linear(gn, M, C, w, C, b, hs[0]));
        for (int a = 0; a < 2; ++a) {
            const std::string ab = tb + ".attention_blocks." + std::to_string(a);
            const float *pe = nullptr, *rope = nullptr;  // "ape": sinusoid added by the LayerNorm kernel; "rope": q|k rotated after the projection
            if (cfg.pe_rope) EDV_TRY(param(ab + ".freqs_cis", &rope, 3));
            else EDV_TRY(param(ab + ".pos_encoder.pe", &pe));
            EDV_TRY(wsbuf(c->train ? tg + "qkv" + std::to_string(a) : sc_ + "qkv", (size_t)M * 3 * C, &qkv3));
            EDV_TRY(ln(hs[a], identity_map(), tb + ".norms." + std::to_string(a), hn, M, C, 1e-5f, pe, P, T));
            const float *wqkv;
            EDV_TRY(packedw(ab + ".qkv", &wqkv));
            EDV_TRY(linear(hn, M, C, wqkv, 3 * C, nullptr, qkv3));
            if (rope) {
                EDV_TRY(rope_qk(qkv3, rope, B, T, P, C, false, st));
                c->launches++;
            }
            {
                Bracket b_(c, KC_ATTN_TEMPORAL, st);
                EDV_TRY(attn_temporal(qkv3, att, B, T, P, C, 8, st));
            }
            c->launches++;
            EDV_TRY(param(ab + ".to_out.0.weight", &w));
            EDV_TRY(param(ab + ".to_out.0.bias", &b));
            EDV_TRY(linear(att, M, C, w, C, b, hs[a + 1], ACT_NONE, nullptr, hs[a]));
        }
        EDV_TRY(ln(hs[2], identity_map(), tb + ".ff_norm", hn, M, C, 1e-5f));
        EDV_TRY(param(tb + ".ff.net.0.proj.weight", &w));
        EDV_TRY(param(tb + ".ff.net.0.proj.bias", &b));
        // Inference: the projection and the GEGLU are ONE launch (EP = 6 of gemm_dma.hip on the interleaved weight made by edv_prepare): the [M, 8C]
        // projection is never written.  Training keeps it (the GEGLU backward reads it), so it runs the two launches.  EDV_GEGLU_FUSED=0: A/B.
        static const bool geglu_fused = env_flag("EDV_GEGLU_FUSED", true);
        bool fused = false;
        if (!c->train && geglu_fused && c->packed.count(tb + ".ff.net.0.geglu.w")) {
            GemmDesc g;
            const float *wi, *bi;
            EDV_TRY(packedw(tb + ".ff.net.0.geglu.w", &wi));
            EDV_TRY(packedw(tb + ".ff.net.0.geglu.b", &bi));
            g.A = hn; g.lda = C; g.W = wi; g.ldw = C; g.C = ff2; g.ldc = 4 * C; g.M = M; g.N = 8 * C; g.K = C; g.bias = bi; g.geglu = 1;
            if (gemm_geglu_supported(g)) {
                c->launches++;
                if (c->prof_mask & (1u << KC_LINEAR)) {  // 2 M N K; A, W read once, the half-width output written once
                    c->prof_flops[KC_LINEAR] += 2.0 * (double)M * (8 * C) * C;
                    c->prof_bytes[KC_LINEAR] += 4.0 * ((double)M * C + (double)8 * C * C + (double)M * 4 * C);
                }
                Bracket b_(c, KC_LINEAR, st);
                EDV_TRY(gemm_ws(g));
                fused = true;
            }
        }
        if (!fused) {
            EDV_TRY(linear(hn, M, C, w, 8 * C, b, ff1));
            {
                HbmScope b_(c, KC_GEGLU, st, 4.0 * (double)M * 12 * C);
                EDV_TRY(geglu(ff1, ff2, M, 4 * C, st));
            }
            c->launches++;
        }
        EDV_TRY(lin_w(tb + ".ff.net.2", &w));
        EDV_TRY(param(tb + ".ff.net.2.bias", &b));
        EDV_TRY(linear(ff2, M, 4 * C, w, C, b, hs[3], ACT_NONE, nullptr, hs[2]));
        EDV_TRY(param(p + ".proj_out.weight", &w));
        EDV_TRY(param(p + ".proj_out.bias", &b));
        {
            GemmDesc g;
            g.A = hs[3]; g.lda = C; g.W = w; g.ldw = C; g.C = x; g.ldc = C; g.M = M; g.N = C; g.K = C;
            g.bias = b; g.R1 = x; g.ldr1 = C; g.R2 = extra; g.ldr2 = C;
            c->launches++;
            Bracket b_(c, KC_LINEAR, st);
            EDV_TRY(gemm_ws(g));
        }
        return 0;
    }

    // ---- FeatureFusionBlock (util/blocks.py:135-162); x, skip: [F,h,w,Fe]; out: [F,oh,ow,Fe] ----
    // The 1x1 out_conv is applied BEFORE the bilinear upsample: both are linear, the interpolation
    // weights sum to one, so conv1x1(up(x)) == up(conv1x1(x)) exactly in real arithmetic, at 1/4 of
    // the GEMM work.
    // ResidualConvUnit (util/blocks.py:68-91): x + conv2(relu(conv1(relu(x)))).  The inner ReLU is applied by conv1's epilogue (its output has no
    // other reader) instead of on conv2's A fragments: 32 v_max_f32 per k-tile less in conv2's loop, same values.  The backward's mask
    // (t1 > 0) reads the same from relu(t1).
    int rcu(const std::string &unit, const float *x, int h, int w, float *t1, float *out, const float *R1, const float *R2) {
        const float *w1, *b1, *w2, *b2;
        EDV_TRY(packedw(unit + ".conv1.weight", &w1));
        EDV_TRY(rcu_bias(unit + ".conv1", &b1));
        EDV_TRY(packedw(unit + ".conv2.weight", &w2));
        EDV_TRY(rcu_bias(unit + ".conv2", &b2));
        EDV_TRY(conv3(x, h, w, Fe, w1, b1, Fe, 1, t1, true, ACT_RELU));
        return conv3(t1, h, w, Fe, w2, b2, Fe, 1, out, false, ACT_NONE, R1, R2);
    }
    // skip == null: x is already the sum s = x + resConfUnit1(skip) (or the block has no skip input: refinenet4), and the block is
    //   out = up(out_conv(s + conv2(relu(conv1(relu(s)))))) (+ add)
    int fusion(int j, const float *x, const float *skip, int h, int w, int oh, int ow, float *out, const float *add = nullptr) {
        const std::string p = "head.scratch.refinenet" + std::to_string(j);
        const size_t n = (size_t)F * h * w * Fe;
        float *t1, *t2, *s, *t1a, *t1b;
        // training keeps both conv1 outputs and the sum s (ReLU masks of the backward), tagged with the block index
        const std::string tg = c->train ? "fu" + std::to_string(j) + "." : "fu.";
        EDV_TRY(wsbuf("fu.t1", n, &t1));
        EDV_TRY(wsbuf("fu.t2", n, &t2));
        t1a = t1b = t1;
        if (c->train) {
            EDV_TRY(wsbuf(tg + "t1a", n, &t1a));
            EDV_TRY(wsbuf(tg + "t1b", n, &t1b));
        }
        if (skip) {
            EDV_TRY(wsbuf(tg + "s", n, &s));
            // s = x + rcu1(skip) = x + skip + conv2(relu(t1)): both adds ride the conv2 epilogue
            // (skip_add at util/blocks.py:90 and :146)
            EDV_TRY(rcu(p + ".resConfUnit1", skip, h, w, t1a, s, skip, x));
            x = s;
        }
        EDV_TRY(rcu(p + ".resConfUnit2", x, h, w, t1b, t2, x, nullptr));
        const float *wo, *bo;
        EDV_TRY(param(p + ".out_conv.weight", &wo));
        EDV_TRY(param(p + ".out_conv.bias", &bo));
        EDV_TRY(linear(t2, (long long)F * h * w, Fe, wo, Fe, bo, t1));
        {
            HbmScope b_(c, KC_BILINEAR, st, 4.0 * (double)F * Fe * ((double)h * w + (double)oh * ow * (add ? 2 : 1)));
            EDV_TRY(bilinear(t1, out, F, h, w, Fe, oh, ow, ACT_NONE, st, add));
        }
        c->launches++;
        return 0;
    }
    // The skip branch of fusion block j without its x:  u = skip + conv2(relu(conv1(relu(skip))))  (resConfUnit1, blocks.py:146).
    // It depends on layerN_rn only, so it can run beside the fusion chain on another stream; whoever produces x adds u.
    int skip_branch(int j, const float *skip, int h, int w, float *u) {
        float *t;
        EDV_TRY(wsbuf("fus.t" + std::to_string(j), (size_t)F * h * w * Fe, &t));
        return rcu("head.scratch.refinenet" + std::to_string(j) + ".resConfUnit1", skip, h, w, t, u, skip, nullptr);
    }
    // The fusion chain path_4 -> path_1 with motion modules 2 and 3 inside it (dpt_pyramid.py:80-86).  u == null: every block computes its own
    // skip branch.  Otherwise u[3], u[2], u[1] come from the internal stream (events ev_x[2], [3], [4]) and whoever produces a block's x adds
    // its u: motion modules 2 and 3 in their proj_out epilogue, fusion block 2 in its upsample.
    int fuse(float *const *u) {
        auto ready = [&](int k) -> int {
            if (u) EDV_HIP(hipStreamWaitEvent(st, c->ev_x[k], 0));
            return 0;
        };
        EDV_TRY(fusion(4, rn[3], nullptr, h4, w4, h3, w3, path[4]));
        EDV_TRY(ready(2));
        EDV_TRY(motion_module(2, path[4], h3 * w3, Fe, u ? u[3] : nullptr));  // with u: p4 <- motion(p4) + u3 = the s of fusion block 3
        EDV_TRY(fusion(3, path[4], u ? nullptr : rn[2], h3, w3, h2, w2, path[3]));
        EDV_TRY(ready(3));
        EDV_TRY(motion_module(3, path[3], h2 * w2, Fe, u ? u[2] : nullptr));  // with u: p3 <- motion(p3) + u2
        EDV_TRY(ready(4));
        EDV_TRY(fusion(2, path[3], u ? nullptr : rn[1], h2, w2, h1, w1, path[2], u ? u[1] : nullptr));  // with u: p2 <- up(...) + u1
        return fusion(1, path[2], u ? nullptr : rn[0], h1, w1, h0, w0, path[1]);
    }

    // ---- ResBottleneckBlock on the patch tokens of encoder block i (block.py:146-150, layers/utils.py:90-153):
    // 1x1 -> LN -> GELU -> 3x3 -> LN -> GELU -> 1x1 -> LN, added to the patch rows of the residual stream.
    // Inference ping-pongs between two scratch buffers, reads the patch rows through a row map and lets GELU ride the LayerNorm launch.  Training
    // keeps every intermediate the backward needs (for all frames of the clip: trainbuf), so it copies the patch rows to a compact buffer
    // (block.py:146: .clone()) and runs LayerNorm and GELU as separate launches: the same arithmetic.
    int res_bottleneck(int i, float *xt) {
        // the reference reshapes to the Block's construction-time grid, input_size=(224,280) -> 16x20 (block.py:70-73)
        EDV_CHECK(ph == 16 && pw == 20, "shape '[B, 16, 20, C]' is invalid for the patch tokens: residual blocks need image_shape (224, 280)");
        const std::string p = "pretrained.blocks." + std::to_string(i) + ".residual_", tg = "rbt" + std::to_string(i) + ".";
        const bool tr = c->train;
        const int Cb = D / 8;
        const long long MP = (long long)F * P0;
        float *xp = nullptr, *t1a, *ln1, *a1, *t1b, *ln2, *a2, *t3;
        if (tr) {
            EDV_TRY(trainbuf(tg + "xp", (size_t)P0 * D, &xp));
            EDV_TRY(trainbuf(tg + "t1a", (size_t)P0 * Cb, &t1a));
            EDV_TRY(trainbuf(tg + "ln1", (size_t)P0 * Cb, &ln1));
            EDV_TRY(trainbuf(tg + "a1", (size_t)P0 * Cb, &a1));
            EDV_TRY(trainbuf(tg + "t1b", (size_t)P0 * Cb, &t1b));
            EDV_TRY(trainbuf(tg + "ln2", (size_t)P0 * Cb, &ln2));
            EDV_TRY(trainbuf(tg + "a2", (size_t)P0 * Cb, &a2));
            EDV_TRY(trainbuf(tg + "t3", (size_t)P0 * D, &t3));
        } else {
            EDV_TRY(wsbuf("rb.t1" + rb_suffix, (size_t)MP * Cb, &t1a));
            EDV_TRY(wsbuf("rb.t2" + rb_suffix, (size_t)MP * Cb, &ln1));
            EDV_TRY(wsbuf("rb.t3" + rb_suffix, (size_t)MP * D, &t3));
            t1b = t1a;
            a1 = ln2 = a2 = ln1;
        }
        const float *w;
        auto norm_gelu = [&](const std::string &norm, const float *in, float *lnout, float *act) -> int {
            const float *nw, *nb;
            EDV_TRY(param(norm + ".weight", &nw));
            EDV_TRY(param(norm + ".bias", &nb));
            EDV_TRY(layernorm(in, identity_map(), nw, nb, lnout, identity_map(), MP, Cb, 1e-6f, nullptr, 0, 0, st, tr ? ACT_NONE : ACT_GELU));
            return tr ? ew_bwd(lnout, nullptr, nullptr, act, MP * Cb, 3, st) : 0;
        };
        EDV_TRY(param(p + ".conv1.weight", &w, 4));
        if (tr) {
            for (int f = 0; f < F; ++f)  // the patch rows of the residual stream, compact
                EDV_TRY(copy_f32(xt + ((size_t)f * ntok + c0) * D, xp + (size_t)f * P0 * D, (long long)P0 * D, st));
            EDV_TRY(linear(xp, MP, D, w, Cb, nullptr, t1a));
        } else {
            GemmDesc g;
            g.A = xt; g.lda = D; g.a_map = RowMap{P0, ntok, c0}; g.W = w; g.ldw = D; g.C = t1a; g.ldc = Cb; g.M = MP; g.N = Cb; g.K = D;
            c->launches++;
            Bracket b_(c, KC_LINEAR, st);
            EDV_TRY(gemm_ws(g));
        }
        EDV_TRY(norm_gelu(p + ".norm1", t1a, ln1, a1));
        EDV_TRY(packedw(p + ".conv2.weight", &w));
        EDV_TRY(conv3(a1, ph, pw, Cb, w, nullptr, Cb, 1, t1b, false));
        EDV_TRY(norm_gelu(p + ".norm2", t1b, ln2, a2));
        EDV_TRY(param(p + ".conv3.weight", &w, 4));
        EDV_TRY(linear(a2, MP, Cb, w, D, nullptr, t3));
        const float *nw, *nb;
        EDV_TRY(param(p + ".norm3.weight", &nw));
        EDV_TRY(param(p + ".norm3.bias", &nb));
        EDV_TRY(layernorm(t3, identity_map(), nw, nb, xt, RowMap{P0, ntok, c0}, MP, D, 1e-6f, nullptr, 0, 0, st, ACT_NONE, true));
        c->launches += tr ? 5 + F : 3;
        return 0;
    }

    struct EncBufs {
        float *cols, *xt, *xn, *qkv, *att, *hid;
        float *tap[4], *tapcls[4];
        const float *pos;
        float *attws;      // attention split workspace, one region of attws_each floats per encoder stream
        size_t attws_each;
    };
    int ensure_streams() {
        if (c->sub[0]) return 0;
        for (int h = 0; h < 4; ++h) {
            EDV_HIP(hipStreamCreateWithFlags(&c->sub[h], hipStreamNonBlocking));
            EDV_HIP(hipEventCreateWithFlags(&c->ev_join[h], hipEventDisableTiming));
        }
        EDV_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        for (int k = 0; k < 6; ++k) EDV_HIP(hipEventCreateWithFlags(&c->ev_x[k], hipEventDisableTiming));
        return 0;
    }
    // a kept activation with `per_frame` floats per frame: sized for every frame of the clip, returned at this frame group's offset
    int trainbuf(const std::string &name, size_t per_frame, float **out) {
        float *base;
        EDV_TRY(wsbuf(name, (size_t)enc_F * per_frame, &base));
        *out = base + (size_t)enc_f0 * per_frame;
        return 0;
    }
    // encoder on frames [f0, f0 + nf) enqueued on the current stream (vision_transformer.py:279-289 + :317-321)
    int encoder_range(const EncBufs &eb, const float *x, int f0, int nf, int H, int W, int lane = 0) {
        F = nf;
        enc_f0 = f0;
        const long long MT = (long long)nf * ntok;
        float *cols = eb.cols + (size_t)f0 * P0 * PE_K, *xt = eb.xt + (size_t)f0 * ntok * D, *xn = eb.xn + (size_t)f0 * ntok * D;
        float *qkv = eb.qkv + (size_t)f0 * ntok * 3 * D, *att = eb.att + (size_t)f0 * ntok * D, *hid = eb.hid + (size_t)f0 * ntok * 4 * D;
        float *tap[4], *tapcls[4];
        for (int j = 0; j < 4; ++j) {
            tap[j] = eb.tap[j] + (size_t)f0 * P0 * D;
            tapcls[j] = eb.tapcls[j] ? eb.tapcls[j] + (size_t)f0 * D : nullptr;
        }
        const float *pos = eb.pos;
        rb_suffix = "." + std::to_string(f0);
        if (c->train) EDV_TRY(trainbuf("t.x.0", (size_t)ntok * D, &xt));  // block i reads t.x.i and writes t.xmid.i, t.x.(i+1)
        {
            HbmScope b_(c, KC_PATCHIFY, st, 4.0 * (double)F * (3.0 * H * W + (double)P0 * PE_K));
            EDV_TRY(patchify(x + (size_t)f0 * 3 * H * W, cols, F, H, W, cfg.image_h, cfg.image_w, st, PE_K));
        }
        c->launches++;
        {
            const float *w, *b;
            EDV_TRY(packedw("pretrained.patch_embed.proj.weight", &w));  // rows padded from 588 to PE_K (edv_prepare)
            EDV_TRY(param("pretrained.patch_embed.proj.bias", &b));
            GemmDesc g;
            g.A = cols; g.lda = PE_K; g.W = w; g.ldw = PE_K; g.C = xt; g.ldc = D; g.M = (long long)F * P0; g.N = D; g.K = PE_K;
            g.bias = b;
            g.c_map = RowMap{P0, ntok, c0};
            g.R1 = pos; g.ldr1 = D; g.r1_map = RowMap{P0, 0, c0};
            EDV_TRY(gemm_ws(g));
            c->launches++;
            if (c0) {
                const float *cls;
                EDV_TRY(param("pretrained.cls_token", &cls));
                EDV_TRY(cls_rows(cls, pos, xt, F, ntok, D, st));
                c->launches++;
            }
        }
        EDV_TRY(snapshot("tokens", xt, (size_t)MT * D));

        // EDV_X6_ATTN=0: in the BF16X6 mode only the linears change, the attention stays on the fp32 kernel (A/B runs)
        static const bool attn_x6 = env_flag("EDV_X6_ATTN", true);
        int tapj = 0;
        in_encoder = true;
        for (int i = 0; i < depth; ++i) {
            const std::string bp = "pretrained.blocks." + std::to_string(i);
            const float *w, *b, *gam;
            // inference: one residual stream updated in place; training: every block keeps its input, its mid-point,
            // its normed MLP input, q|k|v, the attention output + log-sum-exp and the fc1 pre-activation
            float *x_in = xt, *x_mid = xt, *x_out = xt, *xn2 = xn, *lse = nullptr, *pre = nullptr;
            if (c->train) {
                const std::string is = "." + std::to_string(i);
                x_in = xt;
                EDV_TRY(trainbuf("t.xmid" + is, (size_t)ntok * D, &x_mid));
                EDV_TRY(trainbuf("t.x." + std::to_string(i + 1), (size_t)ntok * D, &x_out));
                EDV_TRY(trainbuf("t.xn2" + is, (size_t)ntok * D, &xn2));
                EDV_TRY(trainbuf("t.qkv" + is, (size_t)ntok * 3 * D, &qkv));
                EDV_TRY(trainbuf("t.att" + is, (size_t)ntok * D, &att));
                EDV_TRY(trainbuf("t.lse" + is, (size_t)heads * ntok, &lse));
                EDV_TRY(trainbuf("t.pre" + is, (size_t)ntok * 4 * D, &pre));
                EDV_TRY(trainbuf("t.hid" + is, (size_t)ntok * 4 * D, &hid));
            }
            EDV_TRY(ln(x_in, identity_map(), bp + ".norm1", xn, MT, D, 1e-6f));
            EDV_TRY(param(bp + ".attn.qkv.weight", &w));
            EDV_TRY(param(bp + ".attn.qkv.bias", &b));
            EDV_TRY(linear(xn, MT, D, w, 3 * D, b, qkv));
            if (i == 0 && stagger_record) EDV_HIP(hipEventRecord(c->ev_x[5], st));  // the next frame group may start
            {
                Bracket b_(c, KC_ATTN_SPATIAL, st);
                EDV_TRY(attn_spatial(qkv, att, F, ntok, heads, eb.attws + (size_t)lane * eb.attws_each, eb.attws_each, st, lse,
                                     !c->train && c->products == EDV_PRODUCTS_BF16X6 && attn_x6));
            }
            c->launches++;
            EDV_TRY(param(bp + ".attn.proj.weight", &w));
            EDV_TRY(param(bp + ".attn.proj.bias", &b));
            EDV_TRY(param(bp + ".ls1.gamma", &gam));
            EDV_TRY(linear(att, MT, D, w, D, b, x_mid, ACT_NONE, gam, x_in));
            EDV_TRY(ln(x_mid, identity_map(), bp + ".norm2", xn2, MT, D, 1e-6f));
            EDV_TRY(lin_w(bp + ".mlp.fc1", &w));
            EDV_TRY(param(bp + ".mlp.fc1.bias", &b));
            if (pre) {  // same values as the fused epilogue: GELU of the stored fp32 pre-activation
                EDV_TRY(linear(xn2, MT, D, w, 4 * D, b, pre, ACT_NONE));
                EDV_TRY(ew_bwd(pre, nullptr, nullptr, hid, MT * 4 * D, 3, st));
                c->launches++;
            } else {
                EDV_TRY(linear(xn2, MT, D, w, 4 * D, b, hid, ACT_GELU));
            }
            EDV_TRY(lin_w(bp + ".mlp.fc2", &w));
            EDV_TRY(param(bp + ".mlp.fc2.bias", &b));
            EDV_TRY(param(bp + ".ls2.gamma", &gam));
            EDV_TRY(linear(hid, MT, 4 * D, w, D, b, x_out, ACT_NONE, gam, x_mid));
            xt = x_out;
            if (cfg.residual_mask & (1u << i)) EDV_TRY(res_bottleneck(i, xt));
            if (i == 0) EDV_TRY(snapshot("block0", xt, (size_t)MT * D));
            if (tapj < 4 && i == cfg.taps[tapj]) {
                // final norm on the tap, cls row dropped (vision_transformer.py:317-321)
                EDV_TRY(ln(xt, RowMap{P0, ntok, c0}, "pretrained.norm", tap[tapj], (long long)F * P0, D, 1e-6f));
                                // token 0 of every frame, normed: the cls token, or with include_cls_token=False the first patch
                // ("not real cls tokens", vision_transformer.py:322-324)
                if (cfg.use_clstoken) EDV_TRY(ln(xt, RowMap{1, ntok, 0}, "pretrained.norm", tapcls[tapj], F, D, 1e-6f));
                ++tapj;
            }
        }
        in_encoder = false;
        EDV_CHECK(tapj == 4, "taps must be increasing block indices < depth");
        return 0;
    }
    int encode(const float *x, int H, int W) {
        const long long MT = (long long)F * ntok;
        float *cols, *xt, *xn, *qkv, *att, *hid;
        EDV_TRY(wsbuf("cols", (size_t)F * P0 * PE_K, &cols));
        EDV_TRY(wsbuf("xt", (size_t)MT * D, &xt));
        EDV_TRY(wsbuf("xn", (size_t)MT * D, &xn));
        EDV_TRY(wsbuf("qkv", (size_t)MT * 3 * D, &qkv));
        EDV_TRY(wsbuf("att", (size_t)MT * D, &att));
        EDV_TRY(wsbuf("hid", (size_t)MT * 4 * D, &hid));
        for (int j = 0; j < 4; ++j) EDV_TRY(wsbuf("tap" + std::to_string(j), (size_t)F * P0 * D, &tap[j]));
        if (cfg.use_clstoken)
            for (int j = 0; j < 4; ++j) EDV_TRY(wsbuf("tapcls" + std::to_string(j), (size_t)F * D, &tapcls[j]));

        const float *pos;
        EDV_TRY(pos_table(&pos));
        // Frames are independent in the encoder: with two internal streams the two halves of the batch run as
        // concurrent kernels, so workgroups of different kernels (one half's attention, the other's GEMM) co-reside
        // on the CUs and fill each other's stalls and grid tails.  The head needs all T frames again (temporal attention).
        // Automatic = ONE stream since round 2.  Round 1 ran two frame groups on two streams while a block's GEMMs were short, so that one
        // group's attention filled the launch ramps and drains of the other's GEMMs (+4.8 % at T=8).  With the VALU-free GEMM loop and
        // the VALU-lean attention kernel of round 2 the two-stream form measures equal or slower (ViT-S T=8: 772.7 vs 792.3 frames/s, ViT-B
        // T=16: 280.9 vs 284.9; profiles/r02_notes.txt): co-resident kernels share a SIMD's matrix / vector ALUs, so one kernel's VALU
        // work comes out of the other's matrix time, and the attention kernel's 64 KB of LDS per workgroup leaves room for one GEMM
        // workgroup beside two of its own.  EDV_ENC_STREAMS=2..4 / edv_set_encoder_streams still select the forked form.
        int want = c->enc_streams;
        if (want <= 0) want = 1;
        int nstreams = (want > 1 && !c->capture && !c->train) ? (want > 4 ? 4 : want) : 1;
        enc_F = F;
        if (nstreams > F) nstreams = F;
        size_t attws_each = 0;  // the largest split workspace any stream's share of the frames needs
        for (int h = 0, f0 = 0; h < nstreams; ++h) {
            const int nf = (F - f0) / (nstreams - h);
            const size_t need = (std::max(attn_spatial_workspace(nf, ntok, heads), attn_spatial_workspace(nf, ntok, heads, true)) + 3) & ~(size_t)3;
            attws_each = need > attws_each ? need : attws_each;
            f0 += nf;
        }
        float *attws = nullptr;
        if (attws_each) EDV_TRY(wsbuf("attws", attws_each * nstreams, &attws));
        // Stream-K for the dense GEMMs (gemm_dma.hip): the last partial round of output tiles is split along K over the resident
        // workgroups and merged in-kernel by the last piece to arrive.  One workspace region per stream that launches GEMMs
        // concurrently: the encoder's frame-group streams, and the head's caller / internal stream pair (regions 0 and 1).
        // It applies to deep tiles only (K >= 768, grids under five rounds: gemm_dma.hip).  On by default: fc2 at T=8 138 -> 121 us,
        // ViT-B fc2 at T=8 472 -> 430 us; end to end +0.1 .. +0.7 % on ViT-S T=4/8/16, ViT-B T=8/16 and the fine-tune step
        // (profiles/r01_gemm_tile_sweep.txt).  EDV_GEMM_STREAMK=0 restores one workgroup per tile.
        static const bool gemm_streamk = env_flag("EDV_GEMM_STREAMK", true);
        const size_t skws_each = gemm_streamk ? gemm_workspace() : 0;
        const int skws_regions = nstreams > 2 ? nstreams : 2;
        float *skws_all = nullptr;
        if (skws_each) {
            EDV_TRY(wsbuf("skws", skws_each * skws_regions, &skws_all));
            if (c->skws_zeroed != skws_all) {  // fresh allocation: the arrival counters at the head of each region start at zero
                for (int h = 0; h < skws_regions; ++h) EDV_HIP(hipMemsetAsync(skws_all + (size_t)h * skws_each, 0, gemm_counter_bytes(), st));
                c->skws_zeroed = skws_all;
            }
        }
        EncBufs eb{cols, xt, xn, qkv, att, hid, {tap[0], tap[1], tap[2], tap[3]}, {tapcls[0], tapcls[1], tapcls[2], tapcls[3]}, pos, attws, attws_each};
        skws = skws_all;  // the head runs on the caller's stream with region 0 (the encoder streams have joined by then)
        skws_floats = skws_each;
        if (nstreams == 1) {
            EDV_TRY(encoder_range(eb, x, 0, F, H, W));
        } else {
            EDV_TRY(ensure_streams());
            EDV_HIP(hipEventRecord(c->ev_fork, st));
            static const bool stagger = env_flag("EDV_ENC_STAGGER", true);  // 0: the groups start together (A/B runs)
            for (int h = 0, f0 = 0; h < nstreams; ++h) {
                const int nf = (F - f0) / (nstreams - h);  // even split of the remaining frames
                EDV_HIP(hipStreamWaitEvent(c->sub[h], c->ev_fork, 0));
                // Group h starts when group h-1 has launched its first attention: the groups then run half a block apart, so
                // one group's attention (2 workgroups per CU, MFMA-bound) runs beside the other's GEMM ramps and drains
                // instead of beside its own kind.
                if (stagger && h > 0) EDV_HIP(hipStreamWaitEvent(c->sub[h], c->ev_x[5], 0));
                stagger_record = stagger && h + 1 < nstreams;
                {
                    OnStream group_(*this, c->sub[h], skws ? skws + (size_t)h * skws_each : nullptr);
                    EDV_TRY(encoder_range(eb, x, f0, nf, H, W, h));
                }
                EDV_HIP(hipEventRecord(c->ev_join[h], c->sub[h]));
                EDV_HIP(hipStreamWaitEvent(st, c->ev_join[h], 0));
                f0 += nf;
            }
        }
        for (int j = 0; j < 4; ++j) c->stages["tap" + std::to_string(j)] = {tap[j], (size_t)F * P0 * D};
        return 0;
    }

        // level j: tap -> 1x1 project -> resize -> (motion module on levels 3, 4) -> 3x3 layerN_rn  (dpt_pyramid.py:52-78)
    int level(int j) {
        const int *oc = cfg.out_channels;
        const long long MP = (long long)F * P0;
        const std::string pp = "head.projects." + std::to_string(j);
        const float *w, *b;
        const float *src = tap[j];
        if (cfg.use_clstoken) {
            // readout_projects[j] = GELU(Linear(2D -> D)) on cat(x, cls): W = [W1 | W2], so
            // y = GELU(W1 x + (W2 cls + b)); the bracket is one [F, D] vector per frame (dpt_pyramid.py:54-57)
            const std::string rp = "head.readout_projects." + std::to_string(j) + ".0";
            const float *rw, *rbias;
            EDV_TRY(param(rp + ".weight", &rw, 2));
            EDV_TRY(param(rp + ".bias", &rbias));
            GemmDesc g1;
            g1.A = tapcls[j]; g1.lda = D; g1.W = rw + D; g1.ldw = 2 * D; g1.C = fbias; g1.ldc = D; g1.M = F; g1.N = D; g1.K = D; g1.bias = rbias;
            EDV_TRY(gemm_ws(g1));
            GemmDesc g2;
            g2.A = tap[j]; g2.lda = D; g2.W = rw; g2.ldw = 2 * D; g2.C = readout; g2.ldc = D; g2.M = MP; g2.N = D; g2.K = D;
            g2.P1 = fbias; g2.ldp1 = D; g2.act = ACT_GELU;
            g2.p1_map = RowMap{P0, 1, 0, 0};  // inner 0: one bias row per frame
            if (c->train) {  // keep the pre-activation of every level; GELU from the stored fp32 value (same values as the fused epilogue)
                float *pre;
                EDV_TRY(wsbuf("ro" + std::to_string(j) + ".pre", (size_t)MP * D, &pre));
                g2.C = pre;
                g2.act = ACT_NONE;
                EDV_TRY(gemm_ws(g2));
                EDV_TRY(ew_bwd(pre, nullptr, nullptr, readout, MP * D, 3, st));
                c->launches++;
            } else {
                EDV_TRY(gemm_ws(g2));
            }
            c->launches += 2;
            src = readout;
            c->stages["tapcls" + std::to_string(j)] = {tapcls[j], (size_t)F * D};
            c->stages["fbias"] = {fbias, (size_t)F * D};       // last level only (buffers are reused)
            c->stages["readout"] = {readout, (size_t)MP * D};
        }
        EDV_TRY(param(pp + ".weight", &w, 4));
        EDV_TRY(param(pp + ".bias", &b));
        float *dst = (j == 2) ? lv[2] : pj[j];  // level 3 is not resized: project straight into l3
        EDV_TRY(linear(src, MP, D, w, oc[j], b, dst));
        if (j < 2) {
            const int s = j == 0 ? 4 : 2;
            const std::string rp = "head.resize_layers." + std::to_string(j);
            const float *wt, *bt;
            EDV_TRY(packedw(rp + ".weight", &wt));
            EDV_TRY(packedw(rp + ".bias", &bt));
            GemmDesc g;
            g.A = pj[j]; g.lda = oc[j]; g.W = wt; g.ldw = oc[j]; g.C = lv[j]; g.M = MP; g.N = s * s * oc[j]; g.K = oc[j];
            g.bias = bt; g.store = STORE_SHUFFLE; g.ps_s = s; g.ps_C = oc[j]; g.ps_h = ph; g.ps_w = pw; g.ldc = oc[j];
            EDV_TRY(gemm_ws(g));
            c->launches++;
        } else if (j == 3) {
            const float *wc, *bc;
            EDV_TRY(packedw("head.resize_layers.3.weight", &wc));
            EDV_TRY(param("head.resize_layers.3.bias", &bc));
            EDV_TRY(conv3(pj[3], ph, pw, oc[3], wc, bc, oc[3], 2, lv[3], false));
        }
        if (j == 2) EDV_TRY(motion_module(0, lv[2], h3 * w3, oc[2]));
        if (j == 3) EDV_TRY(motion_module(1, lv[3], h4 * w4, oc[3]));
        const int hs[4] = {h1, h2, h3, h4}, wsz[4] = {w1, w2, w3, w4};
        const float *wr;
        EDV_TRY(packedw("head.scratch.layer" + std::to_string(j + 1) + "_rn.weight", &wr));
        return conv3(lv[j], hs[j], wsz[j], oc[j], wr, nullptr, Fe, 1, rn[j], false);
    }

    int head_buffers() {
        const int *oc = cfg.out_channels;
        const int hs[5] = {h0, h1, h2, h3, h4}, wsz[5] = {w0, w1, w2, w3, w4};
        for (int j = 0; j < 4; ++j) EDV_TRY(wsbuf("l" + std::to_string(j + 1), (size_t)F * hs[j + 1] * wsz[j + 1] * oc[j], &lv[j]));
        // one projection buffer per level: the four level chains may run on two streams
        for (int j = 0; j < 4; ++j) EDV_TRY(wsbuf("pj" + std::to_string(j), (size_t)F * P0 * oc[j], &pj[j]));
        for (int j = 0; j < 4; ++j) EDV_TRY(wsbuf("r" + std::to_string(j + 1), (size_t)F * hs[j + 1] * wsz[j + 1] * Fe, &rn[j]));
        if (cfg.use_clstoken) {
            EDV_TRY(wsbuf("readout", (size_t)F * P0 * D, &readout));
            EDV_TRY(wsbuf("readout.fb", (size_t)F * D, &fbias));
        }
        for (int k = 4; k >= 1; --k) EDV_TRY(wsbuf("p" + std::to_string(k), (size_t)F * hs[k - 1] * wsz[k - 1] * Fe, &path[k]));
        return 0;
    }
        // The four level chains are independent until the fusion blocks and made of small kernels (7-80 us, a few hundred
        // workgroups each): level 4 -- the longest, with its stride-2 conv and the C = out_channels[3] motion module -- goes
        // to an internal stream, levels 3, 1, 2 stay on the caller's.  Not while training (saved activations are ordered by
        // the backward), with use_clstoken (shared readout scratch) or during a stage capture.
    bool head_on_two_streams() const {
        static const int head_streams = [] {
            const char *e = getenv("EDV_HEAD_STREAMS");  // 1 = everything on the caller's stream, 2 (default) = one internal stream beside it
            const int v = e ? atoi(e) : 2;
            return v < 1 ? 1 : (v > 2 ? 2 : v);
        }();
        // Measured (profiles/r01_gemm_tile_sweep.txt): +3 % at T = 8 and 16, -0.8 % at T = 32, where the head's kernels fill the
        // GPU on their own -- so only up to 16 frames per clip.
        return head_streams > 1 && T <= 16 && !c->train && !cfg.use_clstoken && !c->capture;
    }
    // internal stream: level 4, then the skip branches u3, u2, u1 of the fusion blocks (they need layerN_rn only);
    // caller's stream: levels 3, 1, 2, then the fusion chain, where whoever produces a block's x adds its u:
    // motion modules 2 and 3 in their proj_out epilogue, fusion block 2 in its upsample.
    int head_two_streams() {
        EDV_TRY(ensure_streams());
        float *u[4] = {nullptr, nullptr, nullptr, nullptr};
        EDV_TRY(wsbuf("fu.u1", (size_t)F * h1 * w1 * Fe, &u[1]));
        EDV_TRY(wsbuf("fu.u2", (size_t)F * h2 * w2 * Fe, &u[2]));
        EDV_TRY(wsbuf("fu.u3", (size_t)F * h3 * w3 * Fe, &u[3]));
        const hipStream_t user = st, side = c->sub[0];
        float *const ws_side = skws ? skws + skws_floats : nullptr;  // stream-K region 1 (the caller's stream keeps region 0)
        EDV_HIP(hipEventRecord(c->ev_fork, user));
        EDV_HIP(hipStreamWaitEvent(side, c->ev_fork, 0));
        {
            OnStream side_(*this, side, ws_side);
            EDV_TRY(level(3));
        }
        EDV_HIP(hipEventRecord(c->ev_join[0], side));  // r4 ready
        EDV_TRY(level(2));
        if (cfg.conv_head) {  // the four HeadDepth heads read path_4..path_1 themselves: no folding of u into them
            EDV_TRY(level(0));
            EDV_TRY(level(1));
            EDV_HIP(hipStreamWaitEvent(user, c->ev_join[0], 0));
            return fuse(nullptr);
        }
        EDV_HIP(hipEventRecord(c->ev_x[0], user));  // r3 ready
        EDV_HIP(hipStreamWaitEvent(side, c->ev_x[0], 0));
        {
            OnStream side_(*this, side, ws_side);
            EDV_TRY(skip_branch(3, rn[2], h3, w3, u[3]));
        }
        EDV_HIP(hipEventRecord(c->ev_x[2], side));  // u3 ready
        EDV_TRY(level(0));
        EDV_TRY(level(1));
        EDV_HIP(hipEventRecord(c->ev_x[1], user));  // r1, r2 ready
        EDV_HIP(hipStreamWaitEvent(side, c->ev_x[1], 0));
        {
            OnStream side_(*this, side, ws_side);
            EDV_TRY(skip_branch(2, rn[1], h2, w2, u[2]));
            EDV_HIP(hipEventRecord(c->ev_x[3], side));  // u2 ready
            EDV_TRY(skip_branch(1, rn[0], h1, w1, u[1]));
        }
        EDV_HIP(hipEventRecord(c->ev_x[4], side));  // u1 ready
        EDV_HIP(hipStreamWaitEvent(user, c->ev_join[0], 0));
        return fuse(u);
    }

    // ---- output heads ----
    // What the VDA head and a HeadDepth head share: conv3 -> bilinear to (oh, ow) -> conv3 + ReLU -> 1x1 to one channel with `act`.  tg names
    // the scratch set (the backward looks it up by these names), sized for cap_in / cap_out pixels at the input / output resolution.
    int depth_head(const std::string &tg, const std::string &c1, const std::string &c2, const std::string &c3, const float *x, int h, int w, int oh,
                   int ow, size_t cap_in, size_t cap_out, int act, float *out) {
        float *o1, *up, *o2;
        EDV_TRY(wsbuf(tg + "o1", cap_in * Fh, &o1));
        EDV_TRY(wsbuf(tg + "up", cap_out * Fh, &up));
        const float *wt, *b;
        EDV_TRY(packedw(c1 + ".weight", &wt));
        EDV_TRY(param(c1 + ".bias", &b));
        EDV_TRY(conv3(x, h, w, Fe, wt, b, Fh, 1, o1, false));
        {
            HbmScope b_(c, KC_BILINEAR, st, 4.0 * (double)F * Fh * ((double)h * w + (double)oh * ow));
            EDV_TRY(bilinear(o1, up, F, h, w, Fh, oh, ow, ACT_NONE, st));
        }
        // Inference: the 1x1 rides in the epilogue of the second convolution (conv_dma.hip, conv_dot) -- o2 is neither allocated nor written and the
        // dot_channels launch goes.  Training keeps the two steps: the backward reads o2.
        GemmDesc gd;
        gd.A = up; gd.ldw = 9 * Fh; gd.ldc = 32; gd.M = (long long)F * oh * ow; gd.N = 32; gd.K = 9 * Fh; gd.act = ACT_RELU; gd.act2 = act; gd.dot_out = out;
        gd.loader = LOAD_CONV3; gd.cH = oh; gd.cW = ow; gd.cC = Fh; gd.cOH = oh; gd.cOW = ow; gd.cS = 1;
        if (!c->train && conv_dot_enabled() && conv_dot_supported(gd)) {
            EDV_TRY(packedw(c2 + ".weight", &gd.W));
            EDV_TRY(param(c2 + ".bias", &gd.bias));
            EDV_TRY(param(c3 + ".weight", &gd.w2));
            EDV_TRY(param(c3 + ".bias", &gd.b2));
            c->launches += 2;  // the bilinear above and this one
            if (c->prof_mask & (1u << KC_CONV3)) {  // as conv3() counts a launch, with one float per pixel written
                c->prof_flops[KC_CONV3] += 2.0 * (double)gd.M * gd.N * gd.K;
                c->prof_bytes[KC_CONV3] += 4.0 * ((double)gd.M * Fh + (double)gd.N * gd.K + (double)gd.M);
            }
            Bracket b_(c, KC_CONV3, st);
            return conv_dot(gd, st);
        }
        EDV_TRY(wsbuf(tg + "o2", cap_out * 32, &o2));
        EDV_TRY(packedw(c2 + ".weight", &wt));
        EDV_TRY(param(c2 + ".bias", &b));
        EDV_TRY(conv3(up, oh, ow, Fh, wt, b, 32, 1, o2, false, ACT_RELU));
        EDV_TRY(param(c3 + ".weight", &wt));
        EDV_TRY(param(c3 + ".bias", &b));
        c->launches += 2;
        HbmScope b_(c, KC_DOT, st, 4.0 * (double)F * oh * ow * 33);
        return dot_channels(o2, wt, b, out, (long long)F * oh * ow, 32, act, st);
    }
    int vda_head(float *const disp[4]) {  // dpt.py:117-124 + dpt_pyramid.py:88-102
        const int ih = cfg.image_h, iw = cfg.image_w;
        const std::string oc = "head.scratch.output_conv";
        EDV_TRY(depth_head("hd.", oc + "1", oc + "2.0", oc + "2.2", path[1], h0, w0, ih, iw, (size_t)F * h0 * w0, (size_t)F * ih * iw, ACT_RELU, disp[0]));
        int sh = ih, sw = iw;
        for (int k = 1; k < 4; ++k) {  // F.interpolate(scale_factor=0.5): floor(in/2)
            const int nh = sh / 2, nw = sw / 2;
            HbmScope b_(c, KC_BILINEAR, st, 4.0 * (double)F * ((double)sh * sw + (double)nh * nw));
            EDV_TRY(bilinear(disp[k - 1], disp[k], F, sh, sw, 1, nh, nw, ACT_NONE, st));
            sh = nh; sw = nw;
        }
        c->launches += 3;
        if (cfg.out_sigmoid) {
            if (c->train) {  // the backward needs the ReLU mask of the raw map and every sigmoid output
                float *raw0;
                EDV_TRY(wsbuf("hd.raw0", (size_t)F * ih * iw, &raw0));
                EDV_TRY(copy_f32(disp[0], raw0, (long long)F * ih * iw, st));
            }
            sh = ih; sw = iw;
            for (int k = 0; k < 4; ++k) {
                EDV_TRY(sigmoid_inplace(disp[k], (long long)F * sh * sw, st));
                if (c->train) {
                    float *sg;
                    EDV_TRY(wsbuf("hd.sg" + std::to_string(k), (size_t)F * sh * sw, &sg));
                    EDV_TRY(copy_f32(disp[k], sg, (long long)F * sh * sw, st));
                }
                sh /= 2; sw /= 2;
            }
            c->launches += 4;
        }
        return 0;
    }
    int conv_heads(float *const disp[4]) {  // four HeadDepth heads: endodav/layers.py:206-221 + dpt_pyramid.py:103-109
        const int hs[4] = {h0, h1, h2, h3}, wsz[4] = {w0, w1, w2, w3};
        for (int k = 3; k >= 0; --k) {
            const std::string hp = "head.conv_depth_" + std::to_string(k + 1) + ".head.";
            // training keeps every head's intermediates (and its sigmoid output) for the backward; inference shares one scratch set
            const std::string tg = c->train ? "hd" + std::to_string(k) + "." : "hd.";
            const size_t px = (size_t)F * hs[k] * wsz[k], px0 = c->train ? px : (size_t)F * h0 * w0;
            EDV_TRY(depth_head(tg, hp + "0", hp + "2", hp + "4", path[k + 1], hs[k], wsz[k], 2 * hs[k], 2 * wsz[k], px0, px0 * 4,
                               cfg.inv_sigmoid ? ACT_SIGMOID_NEG : ACT_SIGMOID, disp[k]));
            if (c->train) {
                float *dk;
                EDV_TRY(wsbuf(tg + "disp", px * 4, &dk));
                EDV_TRY(copy_f32(disp[k], dk, (long long)px * 4, st));
            }
        }
        return 0;
    }

    int forward(const float *x, int B_, int T_, int H, int W, float *const disp[4]) {
        set_geometry(B_, T_);
        c->launches = 0;
        c->stages.clear();
        c->F = F; c->T = T; c->ph = ph; c->pw = pw; c->ntok = ntok;
        const int *oc = cfg.out_channels;
        EDV_TRY(encode(x, H, W));
        EDV_TRY(head_buffers());
        if (head_on_two_streams()) {
            EDV_TRY(head_two_streams());
        } else {
            for (int j = 0; j < 4; ++j) EDV_TRY(level(j));
            EDV_TRY(fuse(nullptr));
        }
        c->stages["mm0"] = {lv[2], (size_t)F * h3 * w3 * oc[2]};
        c->stages["mm1"] = {lv[3], (size_t)F * h4 * w4 * oc[3]};
        c->stages["path4"] = {path[4], (size_t)F * h3 * w3 * Fe};
        c->stages["path3"] = {path[3], (size_t)F * h2 * w2 * Fe};
        c->stages["path2"] = {path[2], (size_t)F * h1 * w1 * Fe};
        c->stages["path1"] = {path[1], (size_t)F * h0 * w0 * Fe};
        return cfg.conv_head ? conv_heads(disp) : vda_head(disp);
    }
};

}  // namespace

namespace edv {
int run_forward(edv_ctx *c, hipStream_t st, const float *x, int B, int T, int H, int W, float *const disp[4]) {
    return Forward(c, st).forward(x, B, T, H, W, disp);
}
}  // namespace edv
