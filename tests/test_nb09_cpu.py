"""CPU: notebooks/09_horizon_represented_as_a_stripe.ipynb's LitAutoEncoder.  tests/nb09_reference.py (float64,
torch.nn.functional) is pinned to the golden fixture, which the notebook's own cell produced
(tests/golden/make_nb09_golden.py); then the model's output-size rule, its refusals, the config with notebook 10's fake
datamodule, the entry points' argument checks and what the new wrappers hand to the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nb09_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT
from test_conv2d_glue_cpu import T, check_glue_case, run

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb09_small.npz")
KEYS = [f"{m}.{i}.{w}" for m in ("encoder_conv", "decoder_conv") for i in (0, 2, 4) for w in ("weight", "bias")]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_golden(tag):
    gold = np.load(GOLDEN)
    batch, p = R.G.draw_batch(tag), R.params64(R.G.draw_parameters())
    y_hat = R.forward64(p, batch)
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape) == {"a": (3, 1, 25, 25), "b": (2, 1, 9, 25)}[tag]
    R.check_stored(gold, f"{tag}/y_hat", y_hat, 1e-5)
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    assert sorted(p) == sorted(KEYS)
    for k, v in p.items():
        R.check_stored(gold, f"{tag}/grad/{k}", v.grad, NORM_TOL)


def test_stripe_planes_of_the_golden_cases():
    """Case a: inside, clipped at the right edge, empty; case b: at column 0, clipped."""
    a = R.input64(R.G.draw_batch("a")["HISTORICAL_SAT_IMAGES"], R.G.draw_batch("a")["FORECAST_HORIZON"])[:, 4]
    assert [int(v) for v in a[:, 0].sum(1)] == [5, 2, 0]
    b = R.input64(R.G.draw_batch("b")["HISTORICAL_SAT_IMAGES"], R.G.draw_batch("b")["FORECAST_HORIZON"])[:, 4]
    assert [int(v) for v in b[:, 0].sum(1)] == [5, 4] and b[0, 0, :5].all() and b[1, 0, 50:].all()


def test_output_side_and_refusals():
    from predict_pv_yield_amd.models.conv2d import nb09_stripe_ae as M
    assert [M.output_side(s) for s in (128, 47, 54, 20, 15)] == [65, 25, 25, 9, 9]
    assert [M.target_side(s) for s in (128, 47)] == [64, 24] and M.MIN_IMAGE_SIDE == 15
    with pytest.raises(ValueError, match="at least 15"):
        M.output_side(14)
    M.check_target_side((128, 128), (7, 64, 64))
    M.check_target_side((20, 54), (2, 8, 24))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 65, 65))           # the output's own side: the loss crops the prediction
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 63, 64))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 1, 64, 64))
    model = M.LitAutoEncoder()
    assert model.name == "nb09_stripe_ae"
    assert sum(p.numel() for p in model.parameters()) == 520705
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
    # three or five history frames, a depth axis already there, no batch axis: refused before the device is looked at
    z = torch.zeros
    for hist in (z(2, 3, 16, 16), z(2, 5, 16, 16), z(2, 1, 4, 16, 16), z(4, 16, 16)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({"HISTORICAL_SAT_IMAGES": hist, "FORECAST_HORIZON": z(2)})
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 1e-3
    assert M.LitAutoEncoder(lr=1e-4).configure_optimizers().param_groups[0]["lr"] == 1e-4


def test_config_composes_and_instantiates():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb09_stripe_ae", "datamodule=nb10_fake", "callbacks=none",
                                                              "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb09_stripe_ae.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb10_datamodule.Nb10DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == 520705 and dm.batch_size == 64 and dm.image_size_pixels == 128
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-3
    # the fake datamodule's target is the side this model's loss takes for its history side
    from predict_pv_yield_amd.models.conv2d.nb09_stripe_ae import target_side
    assert target_side(dm.image_size_pixels) == 64


def test_entry_points_refuse_bad_arguments_without_launching():
    """A wrong channel pair, a too-wide plane, a null pointer, a short workspace, a window off y_hat and a dy_gate on the
    head: the ABI's error code and a message, from pointers that are never dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    # Conv2d, stride 2
    for c_in, c_out in ((32, 128), (128, 64), (64, 64), (16, 32)):
        assert lib.pv_conv2d_wide_s2_fwd_f32(p, p, p, p, 2, c_in, c_out, 20, 20, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv2d_wide_s2_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 20, 20, None) == ESIZE
        assert lib.pv_conv2d_wide_s2_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 20, 20, p, 1 << 30, None) == ESIZE
        assert lib.pv_conv2d_wide_s2_bwd_weight_workspace_bytes(2, c_in, c_out, 20, 20, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_wide_s2_fwd_f32(p, p, p, p, 2, 64, 128, 20, 129, 1, None) == ESIZE and "128" in err()
    assert lib.pv_conv2d_wide_s2_bwd_data_f32(p, None, p, p, None, 2, 64, 128, 20, 129, None) == ESIZE
    assert lib.pv_conv2d_wide_s2_fwd_f32(p, p, p, p, 2, 64, 128, 2, 20, 1, None) == ESIZE and "3x3" in err()
    assert lib.pv_conv2d_wide_s2_fwd_f32(p, p, p, p, 1 << 14, 128, 128, 128, 128, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_conv2d_wide_s2_fwd_f32(p, p, p, p, 0, 64, 128, 20, 20, 1, None) == EINVAL
    assert lib.pv_conv2d_wide_s2_fwd_f32(None, p, p, p, 2, 64, 128, 20, 20, 1, None) == EINVAL and "null" in err()
    assert lib.pv_conv2d_wide_s2_bwd_data_f32(p, None, p, None, None, 2, 64, 128, 20, 20, None) == EINVAL
    assert lib.pv_conv2d_wide_s2_bwd_weight_workspace_bytes(2, 64, 128, 20, 20, None) == EINVAL
    assert lib.pv_conv2d_wide_s2_bwd_weight_workspace_bytes(2, 64, 128, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_wide_s2_bwd_weight_f32(p, p, None, p, p, 2, 64, 128, 20, 20, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_conv2d_wide_s2_bwd_weight_f32(p, p, None, p, p, 2, 64, 128, 20, 20, None, need.value, None) == EINVAL
    # the stripe first layer
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, p, p, p, p, 2, 8, 20, 20, 64, 5, None) == ESIZE and "history" in err()
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, p, p, p, p, 2, 0, 20, 20, 64, 5, None) == ESIZE
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, p, p, p, p, 2, 4, 20, 20, 32, 5, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, p, p, p, p, 2, 4, 20, 129, 64, 5, None) == ESIZE
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, p, p, p, p, 2, 4, 2, 20, 64, 5, None) == ESIZE
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, p, p, p, p, 2, 4, 20, 20, 64, -1, None) == EINVAL
    assert lib.pv_conv2d_wide_s2_stripe_fwd_f32(p, None, p, p, p, 2, 4, 20, 20, 64, 5, None) == EINVAL
    assert lib.pv_conv2d_wide_s2_bwd_weight_workspace_bytes(2, 5, 64, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_wide_s2_stripe_bwd_weight_f32(p, p, p, p, p, 2, 4, 20, 20, 64, 5, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_conv2d_wide_s2_stripe_bwd_weight_f32(p, p, None, p, p, 2, 4, 20, 20, 64, 5, p, need.value, None) == EINVAL
    # ConvTranspose2d, stride 2
    for c_in, c_out in ((64, 128), (128, 64), (32, 32), (128, 1)):
        assert lib.pv_convt2d_wide_s2_fwd_f32(p, p, p, p, 2, c_in, c_out, 9, 9, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_convt2d_wide_s2_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 9, 9, None) == ESIZE
        assert lib.pv_convt2d_wide_s2_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 9, 9, p, 1 << 30, None) == ESIZE
        assert lib.pv_convt2d_wide_s2_bwd_weight_workspace_bytes(2, c_in, c_out, 9, 9, ctypes.byref(need)) == ESIZE
    assert lib.pv_convt2d_wide_s2_fwd_f32(p, p, p, p, 2, 128, 128, 9, 64, 1, None) == ESIZE and "129" in err()
    assert lib.pv_convt2d_wide_s2_bwd_data_f32(p, None, p, p, None, 2, 128, 128, 9, 64, None) == ESIZE
    assert lib.pv_convt2d_wide_s2_fwd_f32(p, p, p, p, 2, 128, 128, 0, 9, 1, None) == EINVAL
    assert lib.pv_convt2d_wide_s2_fwd_f32(p, None, p, p, 2, 128, 128, 9, 9, 1, None) == EINVAL and "null" in err()
    assert lib.pv_convt2d_wide_s2_bwd_weight_workspace_bytes(2, 128, 128, 9, 9, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_convt2d_wide_s2_bwd_weight_f32(p, p, None, p, p, 2, 128, 128, 9, 9, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    # the head
    assert lib.pv_convt2d_head_fwd_f32(p, p, p, p, 2, 128, 2, 20, 20, 0, None) == ESIZE and "c_out" in err()
    assert lib.pv_convt2d_head_fwd_f32(p, p, p, p, 2, 128, 1, 20, 129, 0, None) == ESIZE and "128" in err()
    assert lib.pv_convt2d_head_fwd_f32(p, None, p, p, 2, 128, 1, 20, 20, 0, None) == EINVAL
    assert lib.pv_convt2d_head_fwd_f32(p, p, p, p, 2, 0, 1, 20, 20, 0, None) == EINVAL
    assert lib.pv_convt2d_head_bwd_data_f32(p, p, p, p, None, 2, 128, 1, 20, 20, None) == EINVAL and "dy_gate" in err()
    assert lib.pv_convt2d_head_bwd_weight_f32(p, p, p, p, p, 2, 128, 1, 20, 20, p, 1 << 30, None) == EINVAL
    assert "dy_gate" in err()
    assert lib.pv_convt2d_head_bwd_weight_workspace_bytes(2, 128, 1, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_convt2d_head_bwd_weight_f32(p, p, None, p, p, 2, 128, 1, 20, 20, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    # the loss: y_hat 9 x 25, a window that leaves it by a row, by a column, by its origin
    assert lib.pv_mse_pred_window_f32(p, p, 2, 9, 25, 9, 24, 1, 0, p, p, p, 8, None) == ESIZE and "window" in err()
    assert lib.pv_mse_pred_window_f32(p, p, 2, 9, 25, 8, 24, 0, 2, p, p, p, 8, None) == ESIZE
    assert lib.pv_mse_pred_window_f32(p, p, 2, 9, 25, 8, 24, -1, 0, p, p, p, 8, None) == ESIZE
    assert lib.pv_mse_pred_window_f32(p, p, 2, 9, 25, 10, 26, 0, 0, p, p, p, 8, None) == ESIZE
    assert lib.pv_mse_pred_window_f32(p, None, 2, 9, 25, 8, 24, 0, 0, p, p, p, 8, None) == EINVAL and "null" in err()
    assert lib.pv_mse_pred_window_f32(p, p, 2, 9, 25, 8, 24, 0, 0, None, p, p, 8, None) == EINVAL
    assert lib.pv_mse_pred_window_f32(p, p, 2, 9, 25, 8, 24, 0, 0, p, p, p, 7, None) == EINVAL and "workspace" in err()


# ---- what the new wrappers hand to the C ABI (the harness of tests/test_conv2d_glue_cpu.py) --------------------------------
X64, X128 = (2, 64, 10, 12), (2, 128, 4, 5)
STRIPE = dict(history=T(2, 4, 10, 12), stripe_start=T(2, dtype=torch.int32))
GLUE = {
    "conv2d_wide_s2_fwd": (
        "conv2d_wide_s2_fwd_f32", dict(x=T(*X64), weight=T(128, 64, 3, 3), bias=T(128), relu=True),
        ["require_cuda", "pv_conv2d_wide_s2_fwd_f32 x weight bias out0 2 64 128 10 12 1 stream"], ["(2, 128, 4, 5) float32"], []),
    "conv2d_wide_s2_fwd/none": (
        "conv2d_wide_s2_fwd_f32", dict(x=T(*X64), weight=T(128, 64, 3, 3), bias=None, relu=False),
        ["require_cuda", "pv_conv2d_wide_s2_fwd_f32 x weight NULL out0 2 64 128 10 12 0 stream"], ["(2, 128, 4, 5) float32"], []),
    "conv2d_wide_s2_bwd_data": (
        "conv2d_wide_s2_bwd_data_f32", dict(dy=T(2, 128, 4, 5), dy_gate=T(2, 128, 4, 5), weight=T(128, 64, 3, 3), x_gate=T(*X64),
                                            x_shape=X64),
        ["require_cuda", "pv_conv2d_wide_s2_bwd_data_f32 dy dy_gate weight out0 x_gate 2 64 128 10 12 stream"],
        ["(2, 64, 10, 12) float32"], []),
    "conv2d_wide_s2_bwd_weight": (
        "conv2d_wide_s2_bwd_weight_f32", dict(x=T(*X64), dy=T(2, 128, 4, 5), dy_gate=None, weight_shape=(128, 64, 3, 3)),
        ["require_cuda", "pv_conv2d_wide_s2_bwd_weight_workspace_bytes 2 64 128 10 12 &bytes",
         "pv_conv2d_wide_s2_bwd_weight_f32 x dy NULL out0 out1 2 64 128 10 12 ws:conv2d_wide_s2_wgrad 4096 stream"],
        ["(128, 64, 3, 3) float32", "(128,) float32"], ["conv2d_wide_s2_wgrad"]),
    "conv2d_wide_s2_stripe_fwd": (
        "conv2d_wide_s2_stripe_fwd_f32", dict(**STRIPE, weight=T(64, 5, 3, 3), bias=T(64), stripe_width=5),
        ["require_cuda", "require_cuda", "pv_conv2d_wide_s2_stripe_fwd_f32 history stripe_start weight bias out0 2 4 10 12 64 5 stream"],
        ["(2, 64, 4, 5) float32"], []),
    "conv2d_wide_s2_stripe_bwd_weight": (
        "conv2d_wide_s2_stripe_bwd_weight_f32", dict(**STRIPE, dy=T(2, 64, 4, 5), weight_shape=(64, 5, 3, 3), stripe_width=5),
        ["require_cuda", "require_cuda", "pv_conv2d_wide_s2_bwd_weight_workspace_bytes 2 5 64 10 12 &bytes",
         "pv_conv2d_wide_s2_stripe_bwd_weight_f32 history stripe_start dy out0 out1 2 4 10 12 64 5 ws:conv2d_wide_s2_wgrad 4096 "
         "stream"],
        ["(64, 5, 3, 3) float32", "(64,) float32"], ["conv2d_wide_s2_wgrad"]),
    "convt2d_wide_s2_fwd": (
        "convt2d_wide_s2_fwd_f32", dict(x=T(*X128), weight=T(128, 128, 3, 3), bias=T(128), relu=True),
        ["require_cuda", "pv_convt2d_wide_s2_fwd_f32 x weight bias out0 2 128 128 4 5 1 stream"], ["(2, 128, 9, 11) float32"], []),
    "convt2d_wide_s2_bwd_data": (
        "convt2d_wide_s2_bwd_data_f32", dict(dy=T(2, 128, 9, 11), dy_gate=None, weight=T(128, 128, 3, 3), x_gate=None,
                                             x_shape=X128),
        ["require_cuda", "pv_convt2d_wide_s2_bwd_data_f32 dy NULL weight out0 NULL 2 128 128 4 5 stream"],
        ["(2, 128, 4, 5) float32"], []),
    "convt2d_wide_s2_bwd_weight": (
        "convt2d_wide_s2_bwd_weight_f32", dict(x=T(*X128), dy=T(2, 128, 9, 11), dy_gate=T(2, 128, 9, 11),
                                               weight_shape=(128, 128, 3, 3)),
        ["require_cuda", "pv_convt2d_wide_s2_bwd_weight_workspace_bytes 2 128 128 4 5 &bytes",
         "pv_convt2d_wide_s2_bwd_weight_f32 x dy dy_gate out0 out1 2 128 128 4 5 ws:convt2d_wide_s2_wgrad 4096 stream"],
        ["(128, 128, 3, 3) float32", "(128,) float32"], ["convt2d_wide_s2_wgrad"]),
    "convt2d_head_fwd": (
        "convt2d_head_fwd_f32", dict(x=T(2, 32, 4, 5), weight=T(32, 1, 3, 3), bias=T(1), relu=False),
        ["require_cuda", "pv_convt2d_head_fwd_f32 x weight bias out0 2 32 1 4 5 0 stream"], ["(2, 1, 6, 7) float32"], []),
    "convt2d_head_bwd_data": (
        "convt2d_head_bwd_data_f32", dict(dy=T(2, 1, 6, 7), dy_gate=None, weight=T(32, 1, 3, 3), x_gate=T(2, 32, 4, 5),
                                          x_shape=(2, 32, 4, 5)),
        ["require_cuda", "pv_convt2d_head_bwd_data_f32 dy NULL weight out0 x_gate 2 32 1 4 5 stream"], ["(2, 32, 4, 5) float32"], []),
    "convt2d_head_bwd_weight": (
        "convt2d_head_bwd_weight_f32", dict(x=T(2, 32, 4, 5), dy=T(2, 1, 6, 7), dy_gate=None, weight_shape=(32, 1, 3, 3)),
        ["require_cuda", "pv_convt2d_head_bwd_weight_workspace_bytes 2 32 1 4 5 &bytes",
         "pv_convt2d_head_bwd_weight_f32 x dy NULL out0 out1 2 32 1 4 5 ws:convt2d_head_wgrad 4096 stream"],
        ["(32, 1, 3, 3) float32", "(1,) float32"], ["convt2d_head_wgrad"]),
    "mse_pred_window": (
        "mse_pred_window_f32", dict(y_hat=T(2, 9, 25), target=T(2, 8, 24), row0=0, col0=1, need_grad=True),
        ["require_cuda", "pv_mse_pred_window_f32 y_hat target 2 9 25 8 24 0 1 out0 out1 ws:mse_pred_window 8 stream"],
        ["(1,) float32", "(2, 9, 25) float32"], ["mse_pred_window"]),
    "mse_pred_window/nograd": (
        "mse_pred_window_f32", dict(y_hat=T(2, 9, 25), target=T(2, 8, 24), row0=0, col0=0, need_grad=False),
        ["require_cuda", "pv_mse_pred_window_f32 y_hat target 2 9 25 8 24 0 0 out0 NULL ws:mse_pred_window 8 stream"],
        ["(1,) float32", "None"], ["mse_pred_window"]),
}
GLUE_ERRORS = {
    "pair": ("conv2d_wide_s2_fwd_f32", dict(x=T(2, 32, 10, 12), weight=T(128, 32, 3, 3), bias=None, relu=True), "C_in, C_out"),
    "wide": ("conv2d_wide_s2_fwd_f32", dict(x=T(1, 64, 8, 129), weight=T(128, 64, 3, 3), bias=None, relu=True), "128 columns"),
    "small": ("conv2d_wide_s2_fwd_f32", dict(x=T(1, 64, 2, 9), weight=T(128, 64, 3, 3), bias=None, relu=True), "3 x 3"),
    "dy": ("conv2d_wide_s2_bwd_weight_f32", dict(x=T(*X64), dy=T(2, 128, 8, 10), dy_gate=None, weight_shape=(128, 64, 3, 3)),
           "dy / dy_gate"),
    "convt pair": ("convt2d_wide_s2_fwd_f32", dict(x=T(2, 128, 4, 5), weight=T(128, 64, 3, 3), bias=None, relu=True),
                   "C_in, C_out"),
    "convt wide": ("convt2d_wide_s2_fwd_f32", dict(x=T(1, 128, 4, 64), weight=T(128, 128, 3, 3), bias=None, relu=True),
                   "128 columns"),
    "head weight": ("convt2d_head_fwd_f32", dict(x=T(1, 32, 8, 8), weight=T(32, 2, 3, 3), bias=None, relu=False), "weight"),
    "stripe start": ("conv2d_wide_s2_stripe_fwd_f32", dict(history=T(2, 4, 10, 12), stripe_start=T(2), weight=T(64, 5, 3, 3),
                                                           bias=T(64), stripe_width=5), "stripe_start"),
    "mse dims": ("mse_pred_window_f32", dict(y_hat=T(2, 9, 25), target=T(3, 8, 24), row0=0, col0=0, need_grad=True),
                 "y_hat \\[N, P, Q\\]"),
}


@pytest.mark.parametrize("case_id", sorted(GLUE))
def test_new_wrappers_hand_the_abi_what_the_table_pins(monkeypatch, case_id):
    check_glue_case(monkeypatch, GLUE[case_id])


@pytest.mark.parametrize("case_id", sorted(GLUE_ERRORS))
def test_new_wrappers_refuse_bad_shapes_before_the_library(monkeypatch, case_id):
    fn, args, pattern = GLUE_ERRORS[case_id]
    text, _, _, error = run(monkeypatch, fn, args, {})
    assert isinstance(error, ValueError), error
    assert not [t for t in text if t.startswith("pv_") and not t.endswith("&bytes")], text
    import re
    assert re.search(pattern, str(error)), str(error)


def test_functional_tuples_name_the_new_families():
    from predict_pv_yield_amd import conv2d_functional as C
    from predict_pv_yield_amd import hip_ops as K
    assert C.CONV2D_WIDE_S2_OPS == (K.conv2d_wide_s2_fwd_f32, K.conv2d_wide_s2_bwd_data_f32, K.conv2d_wide_s2_bwd_weight_f32)
    assert C.CONVT2D_WIDE_S2_OPS == (K.convt2d_wide_s2_fwd_f32, K.convt2d_wide_s2_bwd_data_f32,
                                     K.convt2d_wide_s2_bwd_weight_f32)
    assert C.CONVT2D_HEAD_OPS == (K.convt2d_head_fwd_f32, K.convt2d_head_bwd_data_f32, K.convt2d_head_bwd_weight_f32)
    assert C.STRIPE_WIDE_S2_OPS == (K.conv2d_wide_s2_stripe_fwd_f32, K.conv2d_wide_s2_stripe_bwd_weight_f32)
    assert C.STRIPE_WIDTH == 5
