"""Bias gradients of mark_only_part_as_trainable(bias="all") (endodav/layers.py:5-34; BitFit next to the LoRA factors) on MI355X,
against torch autograd through the CPU oracle on the same weights, inputs and upstream gradients, with the gates of
test_backward_gpu.py: 2e-4 scale-relative on the fp32 oracle for the micro cases, 1e-3 against the fp64 graph at full size.
Also: the batched column-sum kernel (bias_colsum.hip) against fp64 numpy, the head-only scope, determinism, the flat buffer and
the refresh path after a bias update."""
import ctypes as C

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, synth
from endodav_amd.endodav import grad_scope
from oracle import endodav_oracle as orc
from tests.helpers import build_model, case_input, oracle_config

pytestmark = pytest.mark.gpu

UNREACHED = "head.scratch.refinenet4.resConfUnit1."


def upstream(shapes, seed=5):
    # a gradient with a definite sign, as a loss has (see test_backward_gpu.upstream)
    return [1.0 + 0.5 * torch.from_numpy(synth.uniform(f"gout{k}", tuple(s), -1.0, 1.0, seed=seed)) for k, s in enumerate(shapes)]


def trainable(model):
    return [n for n, p in model.named_parameters() if p.requires_grad]


def oracle_grads(model, kwargs, x, names, gouts, dtype=torch.float32):
    sd = {k: (v.detach().cpu().clone().to(dtype) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    for n in names:
        sd[n].requires_grad_(True)
    out = orc.forward(sd, x.to(dtype), oracle_config(kwargs))
    loss = sum((out[("disp", s)] * gouts[s].to(dtype)).sum() for s in range(4))
    return dict(zip(names, torch.autograd.grad(loss, [sd[n] for n in names], allow_unused=True)))


def hip_grads(model, x, names, gouts, cuda):
    model.zero_grad(set_to_none=True)
    out = model(x.to(cuda))
    loss = sum((out[("disp", s)] * gouts[s].to(cuda)).sum() for s in range(4))
    loss.backward()
    sd = model.state_dict(keep_vars=True)
    return {n: sd[n].grad for n in names}


def check(hip, ref, tol):
    worst = 0.0
    for n, r in ref.items():
        g = hip[n]
        if r is None:  # not reached by the forward: no gradient in the reference, none here
            assert g is None, n
            continue
        assert g is not None and g.shape == r.shape, n
        err = (g.cpu().double() - r.double()).abs().max().item() / max(r.abs().max().item(), 1e-30)
        worst = max(worst, err)
        assert err <= tol, f"{n}: scale-relative gradient error {err:.2e} > {tol:.0e}"
    return worst


def bias_all(model):
    endodav_amd.mark_only_part_as_trainable(model, bias="all")
    names = trainable(model)
    assert any(n.startswith("pretrained.") and n.endswith(".bias") for n in names)
    return names


@pytest.mark.parametrize("case", ["micro_vda_dvlora", "micro_vda_lora_b2", "micro_t1", "micro_conv_dvlora", "micro_conv_invsig_ssb", "micro_vda_none_outsig",
                                  "micro_vda_temporal_lora", "micro_rope", "micro_clstoken", "micro_vitl"])
def test_bias_all_gradients_match_oracle_autograd(lib, cuda, case):
    model, kwargs, shape, kind, _ = build_model(case)
    x = case_input(case)
    names = bias_all(model)
    model = model.to(cuda).train()
    BT = shape[0] * shape[1]
    gouts = upstream([(BT, 1, h, w) for (h, w) in model.output_shapes()])
    ref = oracle_grads(model, kwargs, x, names, gouts)
    hip = hip_grads(model, x, names, gouts, cuda)
    assert all(ref[n] is None for n in names if n.startswith(UNREACHED))
    worst = check(hip, ref, 2e-4)
    print(f"\n[{case}] {len(names)} tensors, worst scale-relative gradient error {worst:.2e}")


@pytest.mark.parametrize("resblocks", [False, True], ids=["vda", "conv_head_resblocks"])
def test_bias_all_gradients_full_size(lib, cuda, resblocks):
    """ViT-S at the trainer's 256x320 -> (224, 280) geometry, T = 2, against the fp64 graph."""
    kwargs = dict(encoder="vits", features=64, out_channels=[48, 96, 192, 384], image_shape=(224, 280), lora_type="dvlora")
    if resblocks:
        kwargs["residual_block_indexes"] = [2, 5, 8, 11]
    else:
        kwargs["disable_conv_head"] = True
    model = endodav_amd.endodav(**kwargs, pretrained_path=None)
    synth.fill_module_(model)
    names = bias_all(model)
    x = torch.from_numpy(synth.synth_clip(1, 2, 256, 320, seed=3, kind="tissue"))
    model = model.to(cuda).train()
    gouts = upstream([(2, 1, h, w) for (h, w) in model.output_shapes()])
    ref64 = oracle_grads(model, kwargs, x, names, gouts, torch.float64)
    hip = hip_grads(model, x, names, gouts, cuda)
    worst = check(hip, ref64, 1e-3)
    print(f"\n[vits 224x280 T=2 bias=all{' resblocks' if resblocks else ''}] {len(names)} tensors, worst error vs the fp64 graph {worst:.2e}")


def test_head_bias_scope_stops_at_the_head(lib, cuda):
    model, kwargs, shape, kind, _ = build_model("micro_clstoken")
    x = case_input("micro_clstoken")
    model = model.to(cuda).train()
    gouts = upstream([(shape[0] * shape[1], 1, h, w) for (h, w) in model.output_shapes()])
    names = bias_all(model)
    full = {n: (g.clone() if g is not None else None) for n, g in hip_grads(model, x, names, gouts, cuda).items()}
    n_full = model.launch_count()
    h_names = [n for n in names if n.startswith("head.") and n.endswith(".bias")]
    for n, p in model.named_parameters():
        p.requires_grad = n in h_names
    assert grad_scope(model._trainable_names())[4:] == (0, 1)
    part = hip_grads(model, x, h_names, gouts, cuda)
    assert model.launch_count() < n_full  # the encoder backward did not run
    for n in h_names:
        if n.startswith(UNREACHED):
            assert part[n] is None and full[n] is None
        else:
            assert torch.equal(part[n], full[n]), n


def test_bias_scope_leaves_factor_gradients_bit_identical(lib, cuda):
    model, kwargs, shape, kind, _ = build_model("micro_conv_dvlora")
    x = case_input("micro_conv_dvlora")
    model = model.to(cuda).train()
    gouts = upstream([(shape[0] * shape[1], 1, h, w) for (h, w) in model.output_shapes()])
    endodav_amd.mark_only_part_as_trainable(model)
    base_names = trainable(model)
    base = {n: g.clone() for n, g in hip_grads(model, x, base_names, gouts, cuda).items()}
    names = bias_all(model)
    a = {n: (g.clone() if g is not None else None) for n, g in hip_grads(model, x, names, gouts, cuda).items()}
    b = hip_grads(model, x, names, gouts, cuda)
    for n in base_names:
        assert torch.equal(a[n], base[n]), n
    for n in names:
        if n.startswith(UNREACHED):
            assert a[n] is None and b[n] is None, n
        else:
            assert torch.equal(a[n], b[n]), n


def test_bias_gradients_live_in_the_flat_buffer_and_accumulate(lib, cuda):
    model, kwargs, shape, kind, _ = build_model("micro_vda_dvlora")
    x = case_input("micro_vda_dvlora").to(cuda)
    x2 = torch.flip(x, dims=[1]).contiguous()
    model = model.to(cuda).train()
    names = bias_all(model)
    params = [p for p in model.parameters() if p.requires_grad]

    def run(clip):
        out = model(clip)
        sum((o * o).mean() for o in out.values()).backward()

    model.zero_grad(set_to_none=True)
    run(x)
    flat = model.flat_gradients(params)
    assert flat is not None  # every reached .grad is a view of its slice
    sd = model.state_dict(keep_vars=True)
    assert all(sd[n].grad is None for n in names if n.startswith(UNREACHED))
    g1 = {n: sd[n].grad.clone() for n in names if not n.startswith(UNREACHED)}
    model.zero_grad(set_to_none=True)
    run(x2)
    g2 = {n: sd[n].grad.clone() for n in g1}
    model.zero_grad(set_to_none=True)
    run(x)
    run(x2)
    for n in g1:
        torch.testing.assert_close(sd[n].grad, g1[n] + g2[n], rtol=0, atol=1e-6 * max(1.0, (g1[n].abs().max() + g2[n].abs().max()).item()))


@pytest.mark.parametrize("products", ["f32", "bf16x6"])
def test_adam_step_on_biases_then_forward_equals_a_fresh_prepare(lib, cuda, products):
    model, kwargs, shape, kind, _ = build_model("micro_vda_temporal_lora")
    x = case_input("micro_vda_temporal_lora").to(cuda)
    model = model.to(cuda).train()
    model.products = products
    bias_all(model)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        sum((o * o).mean() for o in model(x).values()).backward()
        opt.step()
    with torch.no_grad():
        a = [o.clone() for o in model(x).values()]  # refresh path (edv_refresh_lora)
        model._native.clear()
        b = list(model(x).values())                 # bind + prepare from scratch
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_use_bn_bias_edits_reach_the_next_inference(lib, cuda):
    model, kwargs, shape, kind, _ = build_model("micro_bn")
    x = case_input("micro_bn").to(cuda)
    model = model.to(cuda).eval()
    with torch.no_grad():
        model(x)
        for n, p in model.named_parameters():
            if n.endswith(".bias") and n.startswith("head."):
                p.add_(0.01)
        a = [o.clone() for o in model(x).values()]
        model._native.clear()
        b = list(model(x).values())
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_batched_colsum_kernel(lib, cuda):
    rng = np.random.default_rng(7)
    Ns = [1, 3, 48, 384, 1152, 1536, 2048]
    jobs = []
    for k, N in enumerate(Ns):
        M = int(rng.integers(1, 3000)) if k % 2 else 10960 // (1 + k)  # ragged row counts
        jobs.append(dict(N=N, M=M, ld=N + (k % 3), patch=(k == 4), scale=(k % 3 == 1), acc=(k % 2 == 0)))
    srcs, refs, dsts, guards = [], [], [], []
    G = 16
    for j in jobs:
        N, M, ld = j["N"], j["M"], j["ld"]
        if j["patch"]:  # patch rows of ntok-row frames: P0 = 20 patch rows after one cls row
            P0, ntok = 20, 21
            frames = (M + P0 - 1) // P0
            j["M"] = M = frames * P0
            P = rng.standard_normal((frames * ntok, ld)).astype(np.float32)
            rows = np.concatenate([np.arange(f * ntok + 1, f * ntok + 1 + P0) for f in range(frames)])
            j["map"] = (P0, ntok, 1)
        else:
            P = rng.standard_normal((M, ld)).astype(np.float32)
            rows = np.arange(M)
            j["map"] = (0, 0, 0)
        sel = P[rows, :N].astype(np.float64)
        sc = rng.uniform(0.5, 2.0, N).astype(np.float32) if j["scale"] else None
        init = rng.standard_normal(N).astype(np.float32) if j["acc"] else np.zeros(N, np.float32)
        ref = sel.sum(0) * (sc.astype(np.float64) if sc is not None else 1.0) + (init.astype(np.float64) if j["acc"] else 0.0)
        bound = np.abs(sel).sum(0) * (sc if sc is not None else 1.0) * 1e-5 + 1e-6
        buf = torch.full((N + 2 * G,), float("nan"), device=cuda)
        buf[G:G + N] = torch.from_numpy(init).to(cuda)
        srcs.append(torch.from_numpy(P).to(cuda))
        j["sc"] = torch.from_numpy(sc).to(cuda) if sc is not None else None
        refs.append((ref, bound, init))
        dsts.append(buf)
    n = len(jobs)
    src_p = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    lds = (C.c_int64 * n)(*[j["ld"] for j in jobs])
    rows_ = (C.c_int64 * n)(*[j["M"] for j in jobs])
    maps = (C.c_int32 * (3 * n))(*[v for j in jobs for v in j["map"]])
    cols = (C.c_int32 * n)(*[j["N"] for j in jobs])
    scl = (C.c_void_p * n)(*[(j["sc"].data_ptr() if j["sc"] is not None else None) for j in jobs])
    dst_p = (C.c_void_p * n)(*[d.data_ptr() + 4 * G for d in dsts])
    acc = (C.c_int32 * n)(*[int(j["acc"]) for j in jobs])
    nbytes = lib.edv_colsum_batch_workspace(n, rows_, cols)
    ws = torch.empty(nbytes // 4 + 1, device=cuda)
    results = []
    for rep in range(2):
        for d, (_, _, init) in zip(dsts, refs):
            d[G:G + d.numel() - 2 * G] = torch.from_numpy(init).to(cuda)
        _lib.check(lib.edv_colsum_batch(n, src_p, lds, rows_, maps, cols, scl, dst_p, acc, ws.data_ptr(), nbytes, _lib.stream_ptr(cuda)), "edv_colsum_batch")
        torch.cuda.synchronize()
        results.append([d.clone() for d in dsts])
    for k, (d, (ref, bound, _)) in enumerate(zip(results[0], refs)):
        N = jobs[k]["N"]
        assert torch.isnan(d[:G]).all() and torch.isnan(d[G + N:]).all(), f"job {k}: write outside its slice"
        got = d[G:G + N].cpu().double().numpy()
        err = np.abs(got - ref)
        assert (err <= bound).all(), f"job {k} (N={N}): max err {err.max():.3e}"
        assert torch.equal(d[G:G + N], results[1][k][G:G + N]), f"job {k}: not bit-identical run to run"
