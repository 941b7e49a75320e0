"""CPU: host-side logic and the drop-in boundary (no GPU compute calls)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, synth, video
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI ---------------------------------------------------------------------------------------
def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "endodav_hip.h")).read()
    declared = set(re.findall(r"\b(edv_[a-z0-9_]+)\s*\(", header))
    declared -= {"edv_lora_type"}
    assert len(declared) >= 25
    lib = C.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/endodav_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)


def test_abi_version_and_config_layout():
    lib = _lib.load()
    assert lib.edv_abi_version() == _lib.ABI_VERSION
    assert C.sizeof(_lib.EdvConfig) == 4 * 29  # 29 32-bit slots incl. the two int[4] arrays


def test_create_validates_config_without_gpu():
    lib = _lib.load()
    cfg = _lib.EdvConfig()
    h = C.c_void_p()
    assert lib.edv_create(C.byref(cfg), C.byref(h)) != 0
    assert b"ABI" in lib.edv_last_error()
    m = endodav_amd.endodav(encoder="vits", features=64, out_channels=[48, 96, 192, 384], image_shape=(518, 518), disable_conv_head=True)
    cfg = m._config()
    assert lib.edv_create(C.byref(cfg), C.byref(h)) == 0
    oh, ow = C.c_int32(), C.c_int32()
    for s, want in enumerate([(518, 518), (259, 259), (129, 129), (64, 64)]):
        assert lib.edv_output_shape(h, s, C.byref(oh), C.byref(ow)) == 0 and (oh.value, ow.value) == want
    cfg.image_h = 500  # not a multiple of 14 (patch_embed.py:72)
    h2 = C.c_void_p()
    assert lib.edv_create(C.byref(cfg), C.byref(h2)) != 0 and b"14" in lib.edv_last_error()


def test_create_rejects_bad_products_variable_before_allocating(monkeypatch):
    """A bad EDV_PRODUCTS is a configuration error like the others: non-zero, the handle stays null (nothing allocated, nothing to leak), and
    the message names the variable."""
    lib = _lib.load()
    m = endodav_amd.endodav(encoder="vits", features=64, out_channels=[48, 96, 192, 384], image_shape=(518, 518), disable_conv_head=True)
    cfg = m._config()
    monkeypatch.setenv("EDV_PRODUCTS", "fp8")
    h = C.c_void_p()
    assert lib.edv_create(C.byref(cfg), C.byref(h)) != 0
    assert not h.value
    assert b"EDV_PRODUCTS" in lib.edv_last_error()
    for good in ("f32", "bf16x6"):
        monkeypatch.setenv("EDV_PRODUCTS", good)
        assert lib.edv_create(C.byref(cfg), C.byref(h)) == 0 and h.value
        assert lib.edv_get_products(h) == {"f32": 0, "bf16x6": 1}[good]  # EDV_PRODUCTS_* of include/endodav_hip.h
        assert lib.edv_destroy(h) == 0
        h = C.c_void_p()


# ---- drop-in surface --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(H.GOLDEN, "state_keys.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("combo", ["vits_dvlora_vda", "vits_lora_conv", "vits_ssb_vda_tlora", "vits_dash_conv", "vits_none_vda", "vitl_dvlora_vda",
                                   "vits_clstoken_resblocks", "vits_bn_rope"])
def test_state_dict_keys_shapes_and_trainable_set_match_reference(ref_keys, combo):
    entry = ref_keys[combo]
    m = endodav_amd.endodav(**entry["kwargs"], pretrained_path=None)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert sorted(map(tuple, map(lambda kv: (kv[0], tuple(kv[1])), got))) == sorted((k, tuple(s)) for k, s in entry["keys"])
    assert [k for k, _ in got] == [k for k, _ in entry["keys"]], "key ORDER differs from the reference"
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == entry["trainable"]


def test_constructor_errors_follow_the_reference():
    with pytest.raises(KeyError):
        endodav_amd.endodav(encoder="vitg")
    with pytest.raises(AssertionError):
        endodav_amd.endodav(encoder="vits", features=64, out_channels=[48, 96, 192, 384], num_frames=0)
    with pytest.raises(FileNotFoundError):
        endodav_amd.endodav(encoder="vits", features=64, out_channels=[48, 96, 192, 384], pretrained_path="/nonexistent")
    m = endodav_amd.endodav(encoder="vitb", features=128, out_channels=[96, 192, 384, 768])  # extension, SURVEY.md §0.5
    assert m.pretrained.embed_dim == 768 and len(m.pretrained.blocks) == 12


def test_forward_refuses_cpu_tensors():
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(42, 56), disable_conv_head=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 2, 3, 42, 56))


def test_mark_only_part_as_trainable_phases():
    m = endodav_amd.endodav(encoder="vits", features=64, out_channels=[48, 96, 192, 384], lora_type="dvlora")
    names = lambda: {n for n, p in m.named_parameters() if p.requires_grad}
    warm = names()
    assert any("lora_A" in n for n in warm) and any("conv_depth_" in n for n in warm) and not any("lora_U" in n for n in warm)
    assert not any("motion_modules" in n for n in warm)
    endodav_amd.mark_only_part_as_trainable(m.pretrained, warm_up=False)
    after = names()
    assert any("lora_U" in n for n in after) and not any("lora_A" in n for n in after)
    endodav_amd.mark_only_part_as_trainable(m.head, train_output_conv=True)
    with pytest.raises(NotImplementedError):
        endodav_amd.mark_only_part_as_trainable(m, bias="nope")


def test_synth_is_portable_and_stable():
    # known answers: any host must regenerate bit-identical weights
    a = synth.uniform01("w:pretrained.cls_token", 4)
    assert a.dtype == np.float32 and np.all((a >= 0) & (a < 1))
    assert synth.fnv1a64("abc") == 0xE71FA2190541574B
    b = synth.uniform01("w:pretrained.cls_token", 4)
    assert np.array_equal(a, b) and not np.array_equal(a, synth.uniform01("w:pretrained.pos_embed", 4))
    sd = synth.synth_state({"head.motion_modules.0.temporal_transformer.proj_out.weight": (8, 8), "x.ls1.gamma": (4,), "a.pos_encoder.pe": (1, 2, 2)})
    assert "a.pos_encoder.pe" not in sd and np.abs(sd["head.motion_modules.0.temporal_transformer.proj_out.weight"]).max() > 0
    assert sd["x.ls1.gamma"].min() >= 0.2


# ---- whole-video host logic ------------------------------------------------------------------------
def test_window_plan_and_resize_rule():
    assert video.window_plan(60) == (76, [0, 22, 44])  # endodav.py:188-189: pad to k*22 + 10
    assert video.window_plan(22) == (32, [0])
    assert video.window_plan(23) == (54, [0, 22])
    assert video.window_plan(1) == (32, [0])
    assert video.lower_bound_size(1280, 1024, 280, 224) == (280, 224)
    assert video.lower_bound_size(518, 518, 518, 518) == (518, 518)
    w, h = video.lower_bound_size(640, 480, 518, 518)
    assert (w, h) == (686, 518) and w % 14 == 0 and h % 14 == 0


def test_lower_bound_size_follows_the_reference_rule():
    """video.lower_bound_size against the arithmetic of the reference's Resize.get_size (util/transform.py:51-107: keep_aspect_ratio,
    resize_method='lower_bound', ensure_multiple_of=14) at the frame sizes the resize kernel is tested
    with (tests/test_kernels_gpu.py) and a few more."""
    def rule(width, height, tw, th, m=14):
        sh, sw = th / height, tw / width
        if sw > sh:
            sh = sw
        else:
            sw = sh

        def constrain(x, min_val):
            y = int(np.round(x / m) * m)
            if y < min_val:
                y = int(np.ceil(x / m) * m)
            return y

        return constrain(sw * width, tw), constrain(sh * height, th)

    for (w, h, tw, th), want in [((1920, 1080, 518, 518), (924, 518)), ((1280, 1024, 280, 224), (280, 224)), ((280, 224, 280, 224), (280, 224)),
                                 ((83, 61, 56, 42), (56, 42)), ((80, 60, 56, 42), (56, 42)), ((100, 70, 280, 224), (322, 224)),
                                 ((640, 480, 518, 518), (686, 518)), ((720, 576, 280, 224), (280, 224))]:
        assert rule(w, h, tw, th) == want, (w, h, tw, th, rule(w, h, tw, th))
        assert video.lower_bound_size(w, h, tw, th) == want, (w, h, tw, th)


def test_stitching_matches_reference_golden():
    from tests.golden.make_golden import VIDEO_CASE, fake_window_disp

    g = H.load_golden("video_stitch")
    n, h, w = VIDEO_CASE["n_frames"], VIDEO_CASE["h"], VIDEO_CASE["w"]
    total, starts = video.window_plan(n)
    assert len(starts) == g["window_input_means"].shape[0]
    wins = [fake_window_disp(i, h, w)[:, 0] for i in range(len(starts))]
    out = video.stitch_windows(wins, n)
    assert out.shape == g["out"].shape and out.dtype == np.float32
    assert np.abs(out - g["out"]).max() <= 1e-6 * np.abs(g["out"]).max()


def test_long_video_matches_reference_golden():
    """120 frames = 6 windows (tests/golden/video_stitch_long.npz, the reference's own infer_video_depth): the key-frame chain over more than two
    windows (slot 0 of window k is slot 6 of k-1, which is slot 26 of k-2), alignment to an already re-scaled predecessor, and a last window
    that is mostly padding.  The frames' means are pairwise >= 1e-3 apart, so a wrong source index cannot hide behind the 1e-6."""
    from tests.golden.make_golden import VIDEO_LONG_CASE, fake_window_disp, long_video_frames

    g = H.load_golden("video_stitch_long")
    n, h, w = VIDEO_LONG_CASE["n_frames"], VIDEO_LONG_CASE["h"], VIDEO_LONG_CASE["w"]
    frames = long_video_frames(n, h, w)
    per_frame = (frames.astype(np.float32) / 255.0).mean(axis=(1, 2, 3), dtype=np.float64)
    assert np.diff(np.sort(per_frame)).min() >= 1e-3
    sources = video.window_sources(n)
    assert len(sources) == 6 and g["window_input_means"].shape == (6, 32)
    got = np.stack([per_frame[src] for src in sources])
    err = np.abs(got - g["window_input_means"]).max()
    print(f"\n[video_stitch_long] window-input means: {err:.2e}")
    assert err < 1e-6
    out = video.stitch_windows([fake_window_disp(k, h, w)[:, 0] for k in range(6)], n)
    assert out.shape == g["out"].shape == (n, h, w) and out.dtype == np.float32
    serr = np.abs(out - g["out"]).max()
    print(f"[video_stitch_long] stitched output: {serr:.2e} (scale {np.abs(g['out']).max():.3f})")
    assert serr <= 2e-6 * np.abs(g["out"]).max()


@pytest.mark.parametrize("n", [1, 21, 22, 23, 44, 45, 120])
def test_window_boundaries_follow_the_reference_loop(n):
    """window_plan / window_sources against the reference's loop run on frame INDICES (endodav.py:186-199): pad with copies of the last frame by
    its formula, one window every 22 frames below the original length, the first 10 slots refilled from the previous window's input."""
    step = video.INFER_LEN - video.OVERLAP
    pad = (step - (n % step)) % step + (video.INFER_LEN - step)  # endodav.py:188
    padded = list(range(n)) + [n - 1] * pad                      # :189
    want, pre = [], None
    for s0 in range(0, n, step):                                 # :193
        cur = np.array(padded[s0:s0 + video.INFER_LEN])          # :195-197 (in range for every window: that is what the padding is for)
        assert len(cur) == video.INFER_LEN
        if pre is not None:
            cur[:video.OVERLAP] = pre[video.KEYFRAMES]           # :199
        want.append(cur)
        pre = cur
    total, starts = video.window_plan(n)
    sources = video.window_sources(n)
    assert total == len(padded) and starts == list(range(0, n, step))
    assert len(sources) == len(want) == -(-n // step)
    for k, (a, b) in enumerate(zip(sources, want)):
        assert a.shape == (video.INFER_LEN,) and np.array_equal(a, b), k
        assert a.min() >= 0 and a.max() <= n - 1
        if k > 0:
            assert np.array_equal(a[:video.OVERLAP], sources[k - 1][video.KEYFRAMES])
