"""CPU: notebooks/11_just_conv_and_conv_over_time.ipynb's LitAutoEncoder.  tests/nb11_reference.py (torch.nn.functional, P taken
from the input's sides) is pinned to the golden fixture (tests/golden/make_nb11_golden.py) and, in float32, to the notebook's
forward written out on the model file's own nn.Sequential holders; then the model's output-size rule, its refusals, the config
with notebook 10's fake datamodule, the entry points' argument checks, what the new wrappers hand to the C ABI, and the
chain builder's layer table with its ReLU-gating flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nb11_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT, _rel
from test_conv2d_glue_cpu import T, check_glue_case, check_new_symbols, f64, run

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb11_small.npz")
KEYS = ([f"conv.{i}.{w}" for i in (0, 2, 4, 6) for w in ("weight", "bias")]
        + [f"temporal_conv.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")])
N_PARAMS = 15090


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_golden(tag):
    gold = np.load(GOLDEN)
    batch, p = R.G.draw_batch(tag), R.params64(R.G.draw_parameters())
    y_hat = R.forward64(p, batch)
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape) == {"a": (2, 1, 6, 6), "b": (2, 1, 11, 11)}[tag]
    assert _rel(y_hat.detach(), gold[f"{tag}/y_hat"]) <= 1e-5
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    assert sorted(p) == sorted(KEYS)
    for k, v in p.items():
        assert _rel(v.grad, gold[f"{tag}/grad/{k}"]) <= NORM_TOL, k
    assert all(np.abs(gold[f"{tag}/grad/{k}"]).max() > 0 for k in KEYS)      # no layer is dead in the fixture


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_is_the_notebooks_forward_on_the_models_layers(tag):
    """The notebook's forward (11_...ipynb:1428-1451) written out on the model's own holders in float32 on the CPU, with P and
    the output's sides taken from the input where the notebook writes 4096 and 64: the restatement gives the same numbers."""
    from predict_pv_yield_amd.models.conv2d import nb11_conv_over_time as M
    model = M.LitAutoEncoder()
    model.load_state_dict(R.G.draw_parameters())
    batch = R.G.draw_batch(tag)
    hist = batch["HISTORICAL_SAT_IMAGES"]
    b, n_channels, h, w = hist.shape
    horizon_img = torch.zeros(b, 1, h, w)
    for i in range(b):
        start = int(batch["FORECAST_HORIZON"][i] * M.STRIPE_WIDTH)
        horizon_img[i, 0, :, start:start + M.STRIPE_WIDTH] = 1
    outs = []
    with torch.no_grad():
        for f in range(n_channels):
            out = model.conv(torch.cat((hist[:, f:f + 1], horizon_img), dim=1))
            sides = out.shape[2:]
            outs.append(out.view(b, 1, -1, 1))
        want = model.temporal_conv(torch.cat(outs, dim=3)).view(b, 1, *sides)
        got = R.forward({k: v for k, v in model.state_dict().items()}, batch, torch.float32)
    assert tuple(sides) == (M.output_side(h), M.output_side(w))
    assert torch.allclose(got, want, rtol=0, atol=1e-6) and _rel(got, want) <= 1e-6


def test_stripe_planes_and_frame_order_of_the_golden_cases():
    """Case a: inside, clipped at the right edge; case b: at column 0, empty.  Image 4 b + f is frame f of example b."""
    for tag, sums in (("a", [5, 2]), ("b", [5, 0])):
        batch = R.G.draw_batch(tag)
        x = R.input_frames(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"])
        assert [int(v) for v in x[::4, 1, 0].sum(1)] == sums
        for b in range(2):
            for f in range(4):
                assert torch.equal(x[4 * b + f, 0], batch["HISTORICAL_SAT_IMAGES"][b, f].double())
                assert torch.equal(x[4 * b + f, 1], x[4 * b, 1])


def test_output_side_and_refusals():
    from predict_pv_yield_amd.models.conv2d import nb11_conv_over_time as M
    assert [M.output_side(s) for s in (128, 47, 21, 12, 5)] == [64, 24, 11, 6, 3] and M.MIN_IMAGE_SIDE == 5
    with pytest.raises(ValueError, match="at least 5"):
        M.output_side(4)
    M.check_target_side((128, 128), (7, 64, 64))
    M.check_target_side((12, 21), (2, 6, 11))
    for bad in ((7, 65, 65), (7, 63, 64), (7, 1, 64, 64)):
        with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
            M.check_target_side((128, 128), bad)
    model = M.LitAutoEncoder()
    assert model.name == "nb11_conv_over_time"
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS
    assert sum(p.numel() for p in model.temporal_conv.parameters()) == 609
    assert list(model.state_dict()) == KEYS
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.G.PARAM_SHAPES
    batch = {"HISTORICAL_SAT_IMAGES": torch.zeros(2, 4, 16, 16), "FORECAST_HORIZON": torch.tensor([1, 2]),
             "TARGET_SAT_IMAGE": torch.zeros(2, 8, 8)}
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.training_step(batch, 0)
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        model.training_step({**batch, "TARGET_SAT_IMAGE": torch.zeros(2, 9, 9)}, 0)
    z = torch.zeros
    for hist in (z(2, 3, 16, 16), z(2, 5, 16, 16), z(2, 1, 4, 16, 16), z(4, 16, 16)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({"HISTORICAL_SAT_IMAGES": hist, "FORECAST_HORIZON": z(2)})
    with pytest.raises(ValueError, match="FORECAST_HORIZON"):
        model({"HISTORICAL_SAT_IMAGES": z(2, 4, 16, 16), "FORECAST_HORIZON": z(3)})
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 1e-4
    assert M.LitAutoEncoder(lr=1e-3).configure_optimizers().param_groups[0]["lr"] == 1e-3


def test_config_composes_and_instantiates():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb11_conv_over_time", "datamodule=nb10_fake",
                                                              "callbacks=none", "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb11_conv_over_time.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb10_datamodule.Nb10DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS and dm.image_size_pixels == 128
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-4
    assert model.output_side(dm.image_size_pixels) == 64      # the fake datamodule's 64-pixel targets are this model's


def test_the_new_entry_points_are_declared_bound_and_exported():
    check_new_symbols({"pv_conv2d_ae_frame_stripe_fwd_f32": 12, "pv_conv2d_ae_frame_stripe_bwd_weight_workspace_bytes": 5,
                       "pv_conv2d_ae_frame_stripe_bwd_weight_f32": 14, "pv_conv2d_ae_p2_fwd_f32": 11,
                       "pv_conv2d_ae_p2_bwd_data_f32": 11, "pv_conv2d_ae_p2_bwd_weight_workspace_bytes": 6,
                       "pv_conv2d_ae_p2_bwd_weight_f32": 13, "pv_conv_time_fwd_f32": 13, "pv_conv_time_bwd_workspace_bytes": 5,
                       "pv_conv_time_bwd_f32": 22}, notebook="11_just_conv_and_conv_over_time")


def test_entry_points_refuse_bad_arguments_without_launching():
    """A wrong channel pair, a too-wide plane, a wrong frame count, a null pointer and a short workspace: the ABI's error code
    and a message, from pointers that are never dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    # the per-frame stripe first layer: (n, frames, h, w, c_out, stripe_width)
    fwd, wg = lib.pv_conv2d_ae_frame_stripe_fwd_f32, lib.pv_conv2d_ae_frame_stripe_bwd_weight_f32
    assert fwd(p, p, p, p, p, 2, 4, 20, 130, 16, 5, None) == ESIZE and "130" in err()
    assert fwd(p, p, p, p, p, 2, 8, 20, 20, 16, 5, None) == ESIZE and "frame" in err()
    assert fwd(p, p, p, p, p, 2, 0, 20, 20, 16, 5, None) == ESIZE
    assert fwd(p, p, p, p, p, 2, 4, 20, 20, 32, 5, None) == ESIZE and "c_out" in err()
    assert fwd(p, p, p, p, p, 2, 4, 2, 20, 16, 5, None) == ESIZE and "3x3" in err()
    assert fwd(p, p, p, p, p, 1 << 13, 4, 128, 128, 16, 5, None) == ESIZE and "2^31" in err()
    assert fwd(p, p, p, p, p, 2, 4, 20, 20, 16, -1, None) == EINVAL
    assert fwd(p, p, p, p, p, 0, 4, 20, 20, 16, 5, None) == EINVAL
    assert fwd(p, None, p, p, p, 2, 4, 20, 20, 16, 5, None) == EINVAL and "null" in err()
    query = lib.pv_conv2d_ae_frame_stripe_bwd_weight_workspace_bytes
    assert query(2, 4, 20, 130, ctypes.byref(need)) == ESIZE and query(2, 4, 20, 20, None) == EINVAL
    assert query(2, 4, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert wg(p, p, p, p, p, 2, 4, 20, 20, 16, 5, p, need.value - 1, None) == EINVAL and "workspace" in err()
    assert wg(p, p, p, p, p, 2, 4, 20, 20, 16, 5, None, need.value, None) == EINVAL
    assert wg(p, p, None, p, p, 2, 4, 20, 20, 16, 5, p, need.value, None) == EINVAL
    assert wg(p, p, p, p, p, 2, 4, 20, 130, 16, 5, p, 1 << 30, None) == ESIZE
    # the padded 32 -> 32 layer
    for c_in, c_out in ((16, 32), (32, 16), (64, 64), (32, 1)):
        assert lib.pv_conv2d_ae_p2_fwd_f32(p, p, p, p, 2, c_in, c_out, 20, 20, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv2d_ae_p2_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 20, 20, None) == ESIZE
        assert lib.pv_conv2d_ae_p2_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 20, 20, p, 1 << 30, None) == ESIZE
        assert lib.pv_conv2d_ae_p2_bwd_weight_workspace_bytes(2, c_in, c_out, 20, 20, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_ae_p2_fwd_f32(p, p, p, p, 2, 32, 32, 20, 128, 1, None) == ESIZE and "130" in err()
    assert lib.pv_conv2d_ae_p2_bwd_data_f32(p, None, p, p, None, 2, 32, 32, 20, 127, None) == ESIZE
    assert lib.pv_conv2d_ae_p2_fwd_f32(p, p, p, p, 2, 32, 32, 0, 20, 1, None) == EINVAL
    assert lib.pv_conv2d_ae_p2_fwd_f32(p, None, p, p, 2, 32, 32, 20, 20, 1, None) == EINVAL and "null" in err()
    assert lib.pv_conv2d_ae_p2_bwd_data_f32(p, None, p, None, None, 2, 32, 32, 20, 20, None) == EINVAL
    assert lib.pv_conv2d_ae_p2_bwd_weight_workspace_bytes(2, 32, 32, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_ae_p2_bwd_weight_f32(p, p, None, p, p, 2, 32, 32, 20, 20, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    # the convolution over time: (n, frames, c_mid, p)
    assert lib.pv_conv_time_fwd_f32(p, p, p, p, p, p, p, p, 2, 3, 16, 100, None) == ESIZE and "channel" in err()
    assert lib.pv_conv_time_fwd_f32(p, p, p, p, p, p, p, p, 2, 4, 32, 100, None) == ESIZE
    assert lib.pv_conv_time_fwd_f32(p, p, p, p, p, p, p, p, 1 << 15, 4, 16, 1 << 14, None) == ESIZE and "2^31" in err()
    assert lib.pv_conv_time_fwd_f32(p, p, p, p, p, p, p, p, 2, 4, 16, 0, None) == EINVAL
    assert lib.pv_conv_time_fwd_f32(p, p, p, p, p, p, None, p, 2, 4, 16, 100, None) == EINVAL and "null" in err()
    assert lib.pv_conv_time_bwd_workspace_bytes(2, 5, 16, 100, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv_time_bwd_workspace_bytes(2, 4, 16, 100, None) == EINVAL
    assert lib.pv_conv_time_bwd_workspace_bytes(2, 4, 16, 100, ctypes.byref(need)) == 0 and need.value == 609 * 4
    assert lib.pv_conv_time_bwd_workspace_bytes(3, 4, 16, 256, ctypes.byref(need)) == 0 and need.value == 3 * 609 * 4
    assert lib.pv_conv_time_bwd_workspace_bytes(1, 4, 16, 514 * 256, ctypes.byref(need)) == 0 and need.value == 257 * 609 * 4
    bwd = lib.pv_conv_time_bwd_f32
    assert bwd(*[p] * 14, 2, 4, 16, 100, 0, p, 609 * 4 - 1, None) == EINVAL and "workspace" in err()
    assert bwd(*[p] * 14, 2, 4, 16, 100, 1, None, 609 * 4, None) == EINVAL
    assert bwd(*[p] * 7, None, *[p] * 6, 2, 4, 16, 100, 0, p, 609 * 4, None) == EINVAL and "null" in err()
    assert bwd(*[p] * 14, 2, 3, 16, 100, 0, p, 1 << 30, None) == ESIZE


# ---- what the new wrappers hand to the C ABI (the harness of tests/test_conv2d_glue_cpu.py) --------------------------------
X32, Y32, W32 = (2, 32, 10, 12), (2, 32, 12, 14), (32, 32, 3, 3)
STRIPE = dict(history=T(2, 4, 10, 12), stripe_start=T(2, dtype=torch.int32))
TIME = dict(w1=T(16, 1, 1, 2), b1=T(16), w2=T(16, 16, 1, 2), b2=T(16), w3=T(1, 16, 1, 2))
TIME_RESULTS = ["(8, 1, 3, 5) float32", "(16, 1, 1, 2) float32", "(16,) float32", "(16, 16, 1, 2) float32", "(16,) float32",
                "(1, 16, 1, 2) float32", "(1,) float32"]
GLUE = {
    "frame_stripe_fwd": (
        "conv2d_ae_frame_stripe_fwd_f32", dict(**STRIPE, weight=T(16, 2, 3, 3), bias=T(16), stripe_width=5),
        ["require_cuda", "require_cuda",
         "pv_conv2d_ae_frame_stripe_fwd_f32 history stripe_start weight bias out0 2 4 10 12 16 5 stream"],
        ["(8, 16, 8, 10) float32"], []),
    "frame_stripe_fwd/one frame": (
        "conv2d_ae_frame_stripe_fwd_f32", dict(history=T(3, 1, 5, 7), stripe_start=T(3, dtype=torch.int32), weight=T(16, 2, 3, 3),
                                               bias=T(16), stripe_width=0),
        ["require_cuda", "require_cuda",
         "pv_conv2d_ae_frame_stripe_fwd_f32 history stripe_start weight bias out0 3 1 5 7 16 0 stream"],
        ["(3, 16, 3, 5) float32"], []),
    "frame_stripe_bwd_weight": (
        "conv2d_ae_frame_stripe_bwd_weight_f32", dict(**STRIPE, dy=T(8, 16, 8, 10), weight_shape=(16, 2, 3, 3), stripe_width=5),
        ["require_cuda", "require_cuda", "pv_conv2d_ae_frame_stripe_bwd_weight_workspace_bytes 2 4 10 12 &bytes",
         "pv_conv2d_ae_frame_stripe_bwd_weight_f32 history stripe_start dy out0 out1 2 4 10 12 16 5 "
         "ws:conv2d_ae_frame_stripe_wgrad 4096 stream"],
        ["(16, 2, 3, 3) float32", "(16,) float32"], ["conv2d_ae_frame_stripe_wgrad"]),
    "p2_fwd": (
        "conv2d_ae_fwd_f32", dict(x=T(*X32), weight=T(*W32), bias=T(32), relu=True, padding=2),
        ["require_cuda", "pv_conv2d_ae_p2_fwd_f32 x weight bias out0 2 32 32 10 12 1 stream"], ["(2, 32, 12, 14) float32"], []),
    "p2_fwd/none": (
        "conv2d_ae_fwd_f32", dict(x=T(*X32), weight=T(*W32), bias=None, relu=False, padding=2),
        ["require_cuda", "pv_conv2d_ae_p2_fwd_f32 x weight NULL out0 2 32 32 10 12 0 stream"], ["(2, 32, 12, 14) float32"], []),
    "p2_bwd_data": (
        "conv2d_ae_bwd_data_f32", dict(dy=T(*Y32), dy_gate=T(*Y32), weight=T(*W32), x_gate=T(*X32), x_shape=X32, padding=2),
        ["require_cuda", "pv_conv2d_ae_p2_bwd_data_f32 dy dy_gate weight out0 x_gate 2 32 32 10 12 stream"],
        ["(2, 32, 10, 12) float32"], []),
    "p2_bwd_weight": (
        "conv2d_ae_bwd_weight_f32", dict(x=T(*X32), dy=T(*Y32), dy_gate=None, weight_shape=W32, padding=2),
        ["require_cuda", "pv_conv2d_ae_p2_bwd_weight_workspace_bytes 2 32 32 10 12 &bytes",
         "pv_conv2d_ae_p2_bwd_weight_f32 x dy NULL out0 out1 2 32 32 10 12 ws:conv2d_ae_p2_wgrad 4096 stream"],
        ["(32, 32, 3, 3) float32", "(32,) float32"], ["conv2d_ae_p2_wgrad"]),
    # padding=0, spelled out, is the call without the keyword (tests/test_conv2d_glue_cpu.py pins that one)
    "p0_fwd": (
        "conv2d_ae_fwd_f32", dict(x=T(*X32), weight=T(*W32), bias=T(32), relu=True, padding=0),
        ["require_cuda", "pv_conv2d_ae_fwd_f32 x weight bias out0 2 32 32 10 12 1 stream"], ["(2, 32, 8, 10) float32"], []),
    "p0_bwd_data": (
        "conv2d_ae_bwd_data_f32", dict(dy=T(2, 32, 8, 10), dy_gate=None, weight=T(*W32), x_gate=None, x_shape=X32, padding=0),
        ["require_cuda", "pv_conv2d_ae_bwd_data_f32 dy NULL weight out0 NULL 2 32 32 10 12 stream"],
        ["(2, 32, 10, 12) float32"], []),
    "p0_bwd_weight": (
        "conv2d_ae_bwd_weight_f32", dict(x=T(*X32), dy=T(2, 32, 8, 10), dy_gate=None, weight_shape=W32, padding=0),
        ["require_cuda", "pv_conv2d_ae_bwd_weight_workspace_bytes 2 32 32 10 12 0 &bytes",
         "pv_conv2d_ae_bwd_weight_f32 x dy NULL out0 out1 2 32 32 10 12 ws:conv2d_ae_wgrad 4096 stream"],
        ["(32, 32, 3, 3) float32", "(32,) float32"], ["conv2d_ae_wgrad"]),
    "conv_time_fwd": (
        "conv_time_fwd_f32", dict(u=T(8, 1, 3, 5), **TIME, b3=T(1)),
        ["require_cuda", "pv_conv_time_fwd_f32 u w1 b1 w2 b2 w3 b3 out0 2 4 16 15 stream"], ["(2, 1, 3, 5) float32"], []),
    "conv_time_bwd": (
        "conv_time_bwd_f32", dict(u=T(8, 1, 3, 5), dy=T(2, 1, 3, 5), **TIME),
        ["require_cuda", "require_cuda", "pv_conv_time_bwd_workspace_bytes 2 4 16 15 &bytes",
         "pv_conv_time_bwd_f32 u dy w1 b1 w2 b2 w3 out0 out1 out2 out3 out4 out5 out6 2 4 16 15 0 ws:conv_time_bwd 4096 stream"],
        TIME_RESULTS, ["conv_time_bwd"]),
    "conv_time_bwd/gated": (
        "conv_time_bwd_f32", dict(u=T(8, 1, 3, 5), dy=T(2, 1, 3, 5), **TIME, u_is_relu_output=True),
        ["require_cuda", "require_cuda", "pv_conv_time_bwd_workspace_bytes 2 4 16 15 &bytes",
         "pv_conv_time_bwd_f32 u dy w1 b1 w2 b2 w3 out0 out1 out2 out3 out4 out5 out6 2 4 16 15 1 ws:conv_time_bwd 4096 stream"],
        TIME_RESULTS, ["conv_time_bwd"]),
}
P2 = dict(weight=T(*W32), bias=None, relu=True, padding=2)
GLUE_ERRORS = {
    "p2 pair": ("conv2d_ae_fwd_f32", dict(x=T(2, 16, 10, 12), weight=T(32, 16, 3, 3), bias=None, relu=True, padding=2),
                ValueError, "C_in, C_out"),
    "p2 wide": ("conv2d_ae_fwd_f32", dict(x=T(1, 32, 8, 127), **P2), ValueError, "128 columns"),
    "padding": ("conv2d_ae_fwd_f32", dict(x=T(*X32), **{**P2, "padding": 1}), ValueError, "padding 0 or 2"),
    "p2 dy": ("conv2d_ae_bwd_weight_f32", dict(x=T(*X32), dy=T(2, 32, 8, 10), dy_gate=None, weight_shape=W32, padding=2),
              ValueError, "dy / dy_gate"),
    "p2 f64": ("conv2d_ae_fwd_f32", dict(x=T(*X32, dtype=f64), **P2), TypeError, "contiguous float32"),
    "stripe wide": ("conv2d_ae_frame_stripe_fwd_f32", dict(history=T(2, 4, 10, 130), stripe_start=T(2, dtype=torch.int32),
                                                           weight=T(16, 2, 3, 3), bias=T(16), stripe_width=5),
                    ValueError, "128 columns"),
    "stripe start": ("conv2d_ae_frame_stripe_fwd_f32", dict(history=T(2, 4, 10, 12), stripe_start=T(2), weight=T(16, 2, 3, 3),
                                                            bias=T(16), stripe_width=5), ValueError, "stripe_start"),
    "stripe length": ("conv2d_ae_frame_stripe_fwd_f32", dict(history=T(2, 4, 10, 12), stripe_start=T(3, dtype=torch.int32),
                                                             weight=T(16, 2, 3, 3), bias=T(16), stripe_width=5),
                      ValueError, "stripe_start int32 \\[2\\]"),
    "stripe frames": ("conv2d_ae_frame_stripe_fwd_f32", dict(history=T(2, 8, 10, 12), stripe_start=T(2, dtype=torch.int32),
                                                             weight=T(16, 2, 3, 3), bias=T(16), stripe_width=5),
                      ValueError, "history"),
    "stripe weight": ("conv2d_ae_frame_stripe_fwd_f32", dict(**STRIPE, weight=T(16, 5, 3, 3), bias=T(16), stripe_width=5),
                      ValueError, "weight \\[16, 2, 3, 3\\]"),
    "stripe bias": ("conv2d_ae_frame_stripe_fwd_f32", dict(**STRIPE, weight=T(16, 2, 3, 3), bias=None, stripe_width=5),
                    ValueError, "bias \\[16\\]"),
    "stripe f64": ("conv2d_ae_frame_stripe_fwd_f32", dict(history=T(2, 4, 10, 12, dtype=f64),
                                                          stripe_start=T(2, dtype=torch.int32), weight=T(16, 2, 3, 3),
                                                          bias=T(16), stripe_width=5), TypeError, "contiguous float32"),
    "stripe dy": ("conv2d_ae_frame_stripe_bwd_weight_f32", dict(**STRIPE, dy=T(2, 16, 8, 10), weight_shape=(16, 2, 3, 3),
                                                                stripe_width=5), ValueError, "dy \\(8, 16, 8, 10\\)"),
    "time frames": ("conv_time_fwd_f32", dict(u=T(6, 1, 3, 5), **TIME, b3=T(1)), ValueError, "u \\[4 N, 1, H, W\\]"),
    "time params": ("conv_time_fwd_f32", dict(u=T(8, 1, 3, 5), **{**TIME, "w2": T(16, 16, 1, 3)}, b3=T(1)), ValueError,
                    "parameters"),
    "time dy": ("conv_time_bwd_f32", dict(u=T(8, 1, 3, 5), dy=T(2, 1, 5, 3), **TIME), ValueError, "dy \\(2, 1, 3, 5\\)"),
    "time f64": ("conv_time_bwd_f32", dict(u=T(8, 1, 3, 5), dy=T(2, 1, 3, 5, dtype=f64), **TIME), TypeError, "contiguous float32"),
}


@pytest.mark.parametrize("case_id", sorted(GLUE))
def test_new_wrappers_hand_the_abi_what_the_table_pins(monkeypatch, case_id):
    check_glue_case(monkeypatch, GLUE[case_id])


@pytest.mark.parametrize("case_id", sorted(GLUE_ERRORS))
def test_new_wrappers_refuse_bad_arguments_before_the_library(monkeypatch, case_id):
    fn, args, exc_type, pattern = GLUE_ERRORS[case_id]
    text, _, keys, error = run(monkeypatch, fn, args, {})
    assert type(error) is exc_type, error
    assert not [t for t in text if t.startswith("pv_") and not t.endswith("&bytes")], text
    assert re.search(pattern, str(error)), str(error)


def test_padding_0_is_the_call_without_the_keyword(monkeypatch):
    """conv2d_ae_*(..., padding=0) hands the C ABI what the same call without the keyword does."""
    for case_id in ("p0_fwd", "p0_bwd_data", "p0_bwd_weight"):
        fn, args, *_ = GLUE[case_id]
        with_kw = run(monkeypatch, fn, args, {})[:3]
        monkeypatch.undo()
        without = run(monkeypatch, fn, {k: v for k, v in args.items() if k != "padding"}, {})[:3]
        monkeypatch.undo()
        assert with_kw == without and "pv_conv2d_ae_p2" not in " ".join(with_kw[0])


# ---- the chain builder ------------------------------------------------------------------------------------------------------
def test_functional_tuples_name_the_new_families(monkeypatch):
    from predict_pv_yield_amd import conv2d_functional as C
    from predict_pv_yield_amd import hip_ops as K
    assert C.FRAME_STRIPE_AE_OPS == (K.conv2d_ae_frame_stripe_fwd_f32, K.conv2d_ae_frame_stripe_bwd_weight_f32)
    assert len(C.CONV2D_AE_P2_OPS) == 3 and C.CONV2D_AE_P2_OPS not in C.POOL_OPS
    # each of the three is the conv2d_ae pass with padding=2 and nothing else
    calls = []
    for name in ("conv2d_ae_fwd_f32", "conv2d_ae_bwd_data_f32", "conv2d_ae_bwd_weight_f32"):
        monkeypatch.setattr(K, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)))
    C.CONV2D_AE_P2_OPS[0]("x", "w", "b", False)
    C.CONV2D_AE_P2_OPS[1]("dy", "gate", "w", "xg", (1, 2))
    C.CONV2D_AE_P2_OPS[2]("x", "dy", "gate", (3, 4))
    assert calls == [("conv2d_ae_fwd_f32", ("x", "w", "b", False), {"padding": 2}),
                     ("conv2d_ae_bwd_data_f32", ("dy", "gate", "w", "xg", (1, 2)), {"padding": 2}),
                     ("conv2d_ae_bwd_weight_f32", ("x", "dy", "gate", (3, 4)), {"padding": 2})]


def test_chain_builders_layer_table_and_gating_flags(monkeypatch):
    """nb11_conv_over_time_f32: the five layers' ops, inputs and scalars.  Every layer of the per-frame stack ends in a ReLU,
    the head included: each layer above the first gates its dx by its input, and each receives its dy already gated -- the
    head from the convolution over time, which is told that its input is a ReLU output and ends in no ReLU itself."""
    from predict_pv_yield_amd import conv2d_functional as C
    from predict_pv_yield_amd.models.conv2d.nb11_conv_over_time import LitAutoEncoder
    model = LitAutoEncoder()
    t = model.temporal_conv
    history, start = torch.zeros(2, 4, 12, 12), torch.zeros(2, dtype=torch.int32)
    layers = C.nb11_layers(history, start, model.conv, t)
    assert [layer[0] for layer in layers] == [C.FRAME_STRIPE_AE_OPS, C.CONV2D_AE_OPS, C.CONV2D_AE_P2_OPS, C.CONV2D_HEAD_S2_OPS,
                                              C.ConvOverTime]
    assert [layer[1] for layer in layers] == [model.conv[i] for i in (0, 2, 4, 6)] + [t[4]]
    assert layers[0][2][0] is history and layers[0][2][1] is start and layers[0][3] == {"stripe_width": 5}
    assert all(len(layer) == 2 for layer in layers[1:4])
    assert all(a is b for a, b in zip(layers[4][2], (t[0].weight, t[0].bias, t[2].weight, t[2].bias))) and len(layers[4]) == 3

    seen = []

    def synth(ops, inputs, weight, bias, scalars, dy_pregated):
        seen.append(("synth", ops, dy_pregated))
        return "y0"

    def conv(ops, x, weight, bias, relu, x_is_relu_output, dy_pregated):
        seen.append((x, ops, relu, x_is_relu_output, dy_pregated))
        return f"y{len(seen) - 1}"

    def head(u, *rest):
        *params, x_is_relu_output, dy_pregated = rest
        seen.append((u, [tuple(p.shape) for p in params], x_is_relu_output, dy_pregated))
        return "y_hat"

    monkeypatch.setattr(C.SynthConvReLU, "apply", staticmethod(synth))
    monkeypatch.setattr(C.ConvReLU, "apply", staticmethod(conv))
    monkeypatch.setattr(C.ConvOverTime, "apply", staticmethod(head))
    assert C.nb11_conv_over_time_f32(history, start, model.conv, t) == "y_hat"
    assert seen == [("synth", C.FRAME_STRIPE_AE_OPS, True),
                    ("y0", C.CONV2D_AE_OPS, True, True, True),
                    ("y1", C.CONV2D_AE_P2_OPS, True, True, True),
                    ("y2", C.CONV2D_HEAD_S2_OPS, True, True, True),
                    ("y3", [(16, 1, 1, 2), (16,), (16, 16, 1, 2), (16,), (1, 16, 1, 2), (1,)], True, False)]
