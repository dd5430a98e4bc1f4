"""CPU: notebooks/07_multiple_historical_images.ipynb's LitAutoEncoder.  tests/nb07_reference.py (float64,
torch.nn.functional) is pinned to the golden fixture, which the notebook's own cell produced
(tests/golden/make_nb07_golden.py); then the model's names, count and output-size rule, its refusals, the config, the three
float64 identities the kernels are built on (the fold of the frames into the batch, the frame seam of the 128 -> 32
ConvTranspose2d, the horizon channel's equal taps), and the C ABI's glue and refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nb07_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT, _rel
from predict_pv_yield_amd.models.conv2d import nb07_multi_hist as M      # without the model the whole file fails at import
from notebook_model_checks import check_fit64
from test_conv2d_glue_cpu import T, check_glue_case, check_new_symbols

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb07_small.npz")
NEW_SYMBOLS = {"pv_conv2d_s2_frame_horizon_fwd_f32": 11, "pv_conv2d_s2_frame_horizon_bwd_weight_workspace_bytes": 5,
               "pv_conv2d_s2_frame_horizon_bwd_weight_f32": 13, "pv_convt2d_s2_frames_fwd_f32": 11,
               "pv_convt2d_s2_frames_bwd_data_f32": 11, "pv_convt2d_s2_frames_bwd_weight_workspace_bytes": 6,
               "pv_convt2d_s2_frames_bwd_weight_f32": 13}
N_PARAMS = 65537


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_golden(tag):
    gold = np.load(GOLDEN)
    batch, p = R.golden_case(gold, tag)
    p = R.params64(p)
    y_hat = R.forward64(p, batch)
    c = R.G.CASES[tag]
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape) == (len(c["timesteps"]), 1, R.G.out_side(c["h"]),
                                                                      R.G.out_side(c["w"]))
    assert _rel(y_hat.detach(), gold[f"{tag}/y_hat"]) <= 1e-5
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    for k, v in p.items():
        assert _rel(v.grad, gold[f"{tag}/grad/{k}"]) <= NORM_TOL, k
    check_fit64(R, gold, tag, batch, "TARGET_SAT_IMAGE")


def test_golden_cases_are_the_ones_the_issue_names():
    a, b = R.G.draw_batch("a"), R.G.draw_batch("b")
    assert tuple(a["HISTORICAL_SAT_IMAGES"].shape) == (3, 4, 31, 31) and tuple(a["TARGET_SAT_IMAGE"].shape) == (3, 16, 16)
    assert tuple(b["HISTORICAL_SAT_IMAGES"].shape) == (2, 4, 23, 39) and tuple(b["TARGET_SAT_IMAGE"].shape) == (2, 12, 20)
    seq = np.arange(1, 25, dtype=np.float32)
    for batch, steps in ((a, (1, 9, 23)), (b, (12, 24))):
        want = [(np.float32(t) - seq.mean()) / seq.std() for t in steps]
        assert batch["FORECAST_HORIZON"].tolist() == [float(v) for v in want]
    gold = np.load(GOLDEN)
    assert max(v.size for v in gold.values()) == 36864 and os.path.getsize(GOLDEN) < 1 << 20


# ---- the three identities the kernels are built on, in float64 ------------------------------------------------------------
def test_folded_encoder_is_the_loop_and_cat_in_float64():
    """The encoder over the [4 B, 2, H, W] fold (image 4 b + f), viewed [B, 128, e, f], is the notebook's loop over the
    frames and torch.cat along the channels: exactly."""
    g = torch.Generator().manual_seed(7)
    history = torch.randn(3, 4, 23, 31, generator=g, dtype=torch.float64)
    horizon = torch.tensor([0.0, -1.3, 0.7], dtype=torch.float64)
    p = R.params64(R.G.draw_parameters(), requires_grad=False)
    loop = torch.cat([R._encoder64(p, R.frame_input64(history, horizon, f), None) for f in range(4)], dim=1)
    folded = R._encoder64(p, R.folded_input64(history, horizon), None)
    assert tuple(folded.shape) == (12, 32, 2, 3) and folded.is_contiguous()
    assert torch.equal(folded.view(3, 128, 2, 3), loop)


def test_frame_seam_of_the_128_channel_conv_transpose_in_float64():
    """y = b + sum_f convT(x[:, 32 f : 32 f + 32], W[32 f : 32 f + 32]); dx and dW split along the same seam."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 128, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(128, 32, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(32, generator=g, dtype=torch.float64)
    whole = F.conv_transpose2d(x, w, b, stride=2)
    parts = b.view(1, -1, 1, 1) + sum(F.conv_transpose2d(x[:, 32 * f:32 * f + 32], w[32 * f:32 * f + 32], stride=2)
                                      for f in range(4))
    assert _rel(parts.detach(), whole.detach()) <= 1e-14
    dy = torch.randn(*whole.shape, generator=g, dtype=torch.float64)
    whole.backward(dy)
    for f in range(4):
        rows = slice(32 * f, 32 * f + 32)
        assert _rel(F.conv2d(dy, w.detach()[rows], stride=2), x.grad[:, rows]) <= 1e-14
        xs, ws = x.detach()[:, rows].clone().requires_grad_(True), w.detach()[rows].clone().requires_grad_(True)
        F.conv_transpose2d(xs, ws, stride=2).backward(dy)
        assert _rel(ws.grad, w.grad[rows]) <= 1e-14


def test_horizon_channel_taps_share_one_gradient_in_float64():
    """A valid conv of a constant plane sees every output position under every tap: the nine taps of dW[:, 1] are equal, and
    equal sum_i horizon[i / F] sum_pos dy[i]."""
    g = torch.Generator().manual_seed(9)
    history = torch.randn(3, 4, 9, 12, generator=g, dtype=torch.float64)
    horizon = torch.tensor([0.0, -1.3, 0.7], dtype=torch.float64)
    x = R.folded_input64(history, horizon)
    dy = torch.randn(12, 32, 4, 5, generator=g, dtype=torch.float64)
    dw = torch.nn.grad.conv2d_weight(x, (32, 2, 3, 3), dy, stride=2)
    want = (dy.sum((2, 3)) * horizon.repeat_interleave(4).view(-1, 1)).sum(0)
    for tap in range(9):
        assert _rel(dw[:, 1].reshape(32, 9)[:, tap], want) <= 1e-14, tap


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_names_shapes_count_and_size_rule():
    assert [M.output_side(s) for s in (128, 126, 41, 31, 30, 15)] == [65, 61, 21, 17, 13, 9]
    assert M.target_side(128) == 64 and M.MIN_IMAGE_SIDE == 15 and M.MAX_IMAGE_SIDE == 128
    for side in (14, 129, 0):
        with pytest.raises(ValueError, match="15 to 128"):
            M.output_side(side)
    M.check_target_side((128, 128), (7, 64, 64))
    M.check_target_side((23, 39), (2, 12, 20))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 65, 65))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 1, 64, 64))
    model = M.LitAutoEncoder()
    assert model.name == "nb07_multi_hist" and model.nb == "nb07"
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS
    assert list(model.state_dict()) == [f"{part}_conv.{i}.{w}" for part in ("encoder", "decoder") for i in (0, 2, 4)
                                        for w in ("weight", "bias")]
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.G.PARAM_SHAPES
    # the sides of the two nn.Sequential the model holds, on the CPU
    for h, w in ((15, 15), (31, 23), (128, 128)):
        enc = model.encoder_conv(torch.zeros(4, 2, h, w))
        assert enc.shape[:2] == (4, 32)
        dec = model.decoder_conv(enc.view(1, 128, *enc.shape[2:]))
        assert tuple(dec.shape) == (1, 1, M.output_side(h), M.output_side(w))
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 1e-3
    assert M.LitAutoEncoder(lr=1e-4).configure_optimizers().param_groups[0]["lr"] == 1e-4


def test_model_refusals_on_the_cpu():
    z = torch.zeros
    model = M.LitAutoEncoder()
    batch = {"HISTORICAL_SAT_IMAGES": z(2, 4, 31, 31), "FORECAST_HORIZON": torch.tensor([0.1, -0.2]),
             "TARGET_SAT_IMAGE": z(2, 16, 16)}
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        model.training_step({**batch, "TARGET_SAT_IMAGE": z(2, 17, 17)}, 0)
    for side in (14, 129):
        with pytest.raises(ValueError, match="15 to 128"):
            model.training_step({**batch, "HISTORICAL_SAT_IMAGES": z(2, 4, side, side)}, 0)
    # three or five history frames, a channel axis already there, no batch axis: refused before the device is looked at
    for hist in (z(2, 3, 31, 31), z(2, 5, 31, 31), z(2, 1, 4, 31, 31), z(4, 31, 31)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({"HISTORICAL_SAT_IMAGES": hist, "FORECAST_HORIZON": z(2)})
    # ... and so is a horizon of the wrong length, whatever its shape
    for horizon in (z(3), z(1), z(2, 2), z(())):
        with pytest.raises(ValueError, match="FORECAST_HORIZON"):
            model({**batch, "FORECAST_HORIZON": horizon})


def test_glue_refuses_bad_shapes_before_touching_a_device():
    from predict_pv_yield_amd import hip_ops as K
    z = torch.zeros
    first, frames = K.conv2d_s2_frame_horizon_fwd_f32, K.convt2d_s2_frames_fwd_f32
    with pytest.raises(ValueError, match="history \\[N, F"):
        first(z(2, 8, 8), z(2), z(32, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="horizon \\[2\\]"):
        first(z(2, 4, 8, 8), z(8), z(32, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="weight \\[32, 2, 3, 3\\]"):
        first(z(2, 4, 8, 8), z(2), z(16, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        first(z(2, 4, 8, 129), z(2), z(32, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        first(z(2, 4, 2, 8), z(2), z(32, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="bias"):
        first(z(2, 4, 8, 8), z(2), z(32, 2, 3, 3), z(8))
    with pytest.raises(ValueError, match="dy"):
        K.conv2d_s2_frame_horizon_bwd_weight_f32(z(2, 4, 9, 9), z(2), z(2, 32, 4, 4), (32, 2, 3, 3))
    for ci, co in ((32, 32), (64, 32), (128, 16), (128, 128), (96, 32)):      # every wrong channel pair
        with pytest.raises(ValueError, match="x \\[N, 128, H, W\\] and weight \\[128, 32, 3, 3\\]"):
            frames(z(2, ci, 4, 4), z(ci, co, 3, 3), z(co))
    with pytest.raises(ValueError, match="128 columns"):
        frames(z(2, 128, 4, 64), z(128, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="bias"):
        frames(z(2, 128, 4, 4), z(128, 32, 3, 3), z(8))
    with pytest.raises(ValueError, match="dy"):
        K.convt2d_s2_frames_bwd_data_f32(z(2, 32, 9, 8), None, z(128, 32, 3, 3), None, (2, 128, 4, 4))
    with pytest.raises(ValueError, match="dy"):
        K.convt2d_s2_frames_bwd_weight_f32(z(2, 128, 4, 4), z(2, 32, 8, 9), None, (128, 32, 3, 3))


def test_config_composes_and_instantiates():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb07_multi_hist", "datamodule=nb08_fake",
                                                              "callbacks=none", "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb07_multi_hist.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb08_datamodule.Nb08DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS and dm.batch_size == 64 and dm.image_size_pixels == 128
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-3


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound_with_matching_arity():
    check_new_symbols(NEW_SYMBOLS, "07_multiple_historical_images.ipynb")


def test_entry_points_refuse_bad_arguments_without_launching():
    """Every wrong channel pair, a plane over 128 wide, an output over 128 wide, n = 0, frames = 0, a tensor beyond 32-bit
    indexing, a null pointer, a workspace one byte short: the ABI's error code and a message, from pointers that are never
    dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    # the first layer
    first, first_ws, first_wg = (lib.pv_conv2d_s2_frame_horizon_fwd_f32, lib.pv_conv2d_s2_frame_horizon_bwd_weight_workspace_bytes,
                                 lib.pv_conv2d_s2_frame_horizon_bwd_weight_f32)
    assert first(p, p, p, p, p, 2, 4, 20, 129, 1, None) == ESIZE and "width 129" in err()
    assert first(p, p, p, p, p, 2, 4, 2, 20, 1, None) == ESIZE and "kernel" in err()
    assert first(p, p, p, p, p, 2, 4, 20, 2, 1, None) == ESIZE and "kernel" in err()
    assert first(p, p, p, p, p, 0, 4, 20, 20, 1, None) == EINVAL and "non-positive" in err()
    assert first(p, p, p, p, p, 2, 0, 20, 20, 1, None) == EINVAL and "non-positive" in err()
    assert first(p, p, p, p, p, 1 << 10, 4, 128, 128, 1, None) == ESIZE and "2^31" in err()
    assert first(p, p, p, p, p, 1 << 20, 1 << 20, 128, 128, 1, None) == ESIZE and "2^31" in err()
    for null in range(5):
        args = [None if i == null else p for i in range(5)]
        want = ESIZE if null == 3 else EINVAL                     # a null bias is allowed: the width is refused instead
        assert first(*args, 2, 4, 20, 129, 1, None) == want, null
    assert "null" in err()
    assert first_ws(2, 4, 20, 129, ctypes.byref(need)) == ESIZE
    assert first_ws(2, 0, 20, 20, ctypes.byref(need)) == EINVAL
    assert first_ws(2, 4, 20, 20, None) == EINVAL
    assert first_ws(2, 4, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert first_wg(p, p, p, None, p, p, 2, 4, 20, 20, p, need.value - 1, None) == EINVAL and "workspace" in err()
    assert first_wg(p, p, p, None, p, p, 2, 4, 20, 20, None, need.value, None) == EINVAL
    assert first_wg(p, None, p, None, p, p, 2, 4, 20, 20, p, need.value, None) == EINVAL and "null" in err()
    assert first_wg(p, p, p, None, p, p, 2, 4, 20, 129, p, need.value, None) == ESIZE
    # the 128 -> 32 ConvTranspose2d
    fwd, dgrad, ws_q, wgrad = (lib.pv_convt2d_s2_frames_fwd_f32, lib.pv_convt2d_s2_frames_bwd_data_f32,
                               lib.pv_convt2d_s2_frames_bwd_weight_workspace_bytes, lib.pv_convt2d_s2_frames_bwd_weight_f32)
    for c_in, c_out in ((32, 32), (32, 16), (16, 1), (64, 32), (128, 16), (128, 128), (96, 32), (160, 32), (32, 128)):
        assert fwd(p, p, p, p, 2, c_in, c_out, 7, 7, 1, None) == ESIZE and "channel" in err()
        assert dgrad(p, None, p, p, None, 2, c_in, c_out, 7, 7, None) == ESIZE and "channel" in err()
        assert wgrad(p, p, None, p, p, 2, c_in, c_out, 7, 7, p, 1 << 30, None) == ESIZE and "channel" in err()
        assert ws_q(2, c_in, c_out, 7, 7, ctypes.byref(need)) == ESIZE and "channel" in err()
    assert fwd(p, p, p, p, 2, 128, 32, 7, 64, 1, None) == ESIZE and "output width 129" in err()
    assert dgrad(p, None, p, p, None, 2, 128, 32, 7, 64, None) == ESIZE and "output width 129" in err()
    assert fwd(p, p, p, p, 0, 128, 32, 7, 7, 1, None) == EINVAL and "non-positive" in err()
    assert fwd(p, p, p, p, 2, 128, 32, 0, 7, 1, None) == EINVAL
    assert fwd(p, p, p, p, 1 << 12, 128, 32, 63, 63, 1, None) == ESIZE and "2^31" in err()
    assert fwd(None, p, p, p, 2, 128, 32, 7, 7, 1, None) == EINVAL and "null" in err()
    assert fwd(p, p, None, p, 2, 128, 32, 7, 64, 1, None) == ESIZE      # a null bias is allowed
    assert dgrad(p, None, p, None, None, 2, 128, 32, 7, 7, None) == EINVAL
    assert ws_q(2, 128, 32, 7, 7, None) == EINVAL
    assert ws_q(2, 128, 32, 7, 7, ctypes.byref(need)) == 0 and need.value > 0
    assert wgrad(p, p, None, p, p, 2, 128, 32, 7, 7, p, need.value - 1, None) == EINVAL and "workspace" in err()
    assert wgrad(p, p, None, p, p, 2, 128, 32, 7, 7, None, need.value, None) == EINVAL
    assert wgrad(p, None, None, p, p, 2, 128, 32, 7, 7, p, need.value, None) == EINVAL and "null" in err()


# ---- what the new wrappers hand to the C ABI (the harness of tests/test_conv2d_glue_cpu.py) --------------------------------
HIST, X128, Y32, W128 = (2, 4, 9, 11), (2, 128, 4, 5), (2, 32, 9, 11), (128, 32, 3, 3)
GLUE = {
    "frame_horizon_fwd": (
        "conv2d_s2_frame_horizon_fwd_f32", dict(history=T(*HIST), horizon=T(2), weight=T(32, 2, 3, 3), bias=T(32), relu=True),
        ["require_cuda", "pv_conv2d_s2_frame_horizon_fwd_f32 history horizon weight bias out0 2 4 9 11 1 stream"],
        ["(8, 32, 4, 5) float32"], []),
    "frame_horizon_fwd/one_frame": (
        "conv2d_s2_frame_horizon_fwd_f32", dict(history=T(3, 1, 10, 12), horizon=T(3), weight=T(32, 2, 3, 3), bias=None,
                                                relu=False),
        ["require_cuda", "pv_conv2d_s2_frame_horizon_fwd_f32 history horizon weight NULL out0 3 1 10 12 0 stream"],
        ["(3, 32, 4, 5) float32"], []),
    "frame_horizon_bwd_weight": (
        "conv2d_s2_frame_horizon_bwd_weight_f32", dict(history=T(*HIST), horizon=T(2), dy=T(8, 32, 4, 5),
                                                       weight_shape=(32, 2, 3, 3), dy_gate=T(8, 32, 4, 5)),
        ["require_cuda", "pv_conv2d_s2_frame_horizon_bwd_weight_workspace_bytes 2 4 9 11 &bytes",
         "pv_conv2d_s2_frame_horizon_bwd_weight_f32 history horizon dy dy_gate out0 out1 2 4 9 11 "
         "ws:conv2d_s2_frame_horizon_wgrad 4096 stream"],
        ["(32, 2, 3, 3) float32", "(32,) float32"], ["conv2d_s2_frame_horizon_wgrad"]),
    "frame_horizon_bwd_weight/ungated": (
        "conv2d_s2_frame_horizon_bwd_weight_f32", dict(history=T(*HIST), horizon=T(2), dy=T(8, 32, 4, 5),
                                                       weight_shape=(32, 2, 3, 3)),
        ["require_cuda", "pv_conv2d_s2_frame_horizon_bwd_weight_workspace_bytes 2 4 9 11 &bytes",
         "pv_conv2d_s2_frame_horizon_bwd_weight_f32 history horizon dy NULL out0 out1 2 4 9 11 "
         "ws:conv2d_s2_frame_horizon_wgrad 4096 stream"],
        ["(32, 2, 3, 3) float32", "(32,) float32"], ["conv2d_s2_frame_horizon_wgrad"]),
    "convt2d_s2_frames_fwd": (
        "convt2d_s2_frames_fwd_f32", dict(x=T(*X128), weight=T(*W128), bias=T(32), relu=True),
        ["require_cuda", "pv_convt2d_s2_frames_fwd_f32 x weight bias out0 2 128 32 4 5 1 stream"], ["(2, 32, 9, 11) float32"], []),
    "convt2d_s2_frames_bwd_data": (
        "convt2d_s2_frames_bwd_data_f32", dict(dy=T(*Y32), dy_gate=T(*Y32), weight=T(*W128), x_gate=T(*X128), x_shape=X128),
        ["require_cuda", "pv_convt2d_s2_frames_bwd_data_f32 dy dy_gate weight out0 x_gate 2 128 32 4 5 stream"],
        ["(2, 128, 4, 5) float32"], []),
    "convt2d_s2_frames_bwd_weight": (
        "convt2d_s2_frames_bwd_weight_f32", dict(x=T(*X128), dy=T(*Y32), dy_gate=None, weight_shape=W128),
        ["require_cuda", "pv_convt2d_s2_frames_bwd_weight_workspace_bytes 2 128 32 4 5 &bytes",
         "pv_convt2d_s2_frames_bwd_weight_f32 x dy NULL out0 out1 2 128 32 4 5 ws:convt2d_s2_frames_wgrad 4096 stream"],
        ["(128, 32, 3, 3) float32", "(32,) float32"], ["convt2d_s2_frames_wgrad"]),
}


@pytest.mark.parametrize("case_id", sorted(GLUE))
def test_new_wrappers_hand_the_abi_what_the_table_pins(monkeypatch, case_id):
    check_glue_case(monkeypatch, GLUE[case_id])


def test_functional_tuples_and_the_chain_name_the_new_families(monkeypatch):
    from predict_pv_yield_amd import conv2d_functional as C
    from predict_pv_yield_amd import hip_ops as K
    assert C.FRAME_HORIZON_S2_OPS == (K.conv2d_s2_frame_horizon_fwd_f32, K.conv2d_s2_frame_horizon_bwd_weight_f32)
    assert C.CONVT2D_S2_FRAMES_OPS == (K.convt2d_s2_frames_fwd_f32, K.convt2d_s2_frames_bwd_data_f32,
                                       K.convt2d_s2_frames_bwd_weight_f32)
    # the chain nb07_multi_hist_f32 hands to conv_chain: the first layer on (history, horizon), two stride-2 layers, the
    # view, then the three decoder layers, the last without a ReLU
    seen = {}
    monkeypatch.setattr(C, "conv_chain", lambda x, layers, last_relu: seen.update(x=x, layers=layers, last_relu=last_relu))
    enc, dec = list("abcdef"), list("ghijkl")
    history, horizon = torch.zeros(3, 4, 31, 31), torch.zeros(3)
    C.nb07_multi_hist_f32(history, horizon, enc, dec)
    layers = seen["layers"]
    assert seen["x"] is None and seen["last_relu"] is False and len(layers) == 7
    assert layers[0][:2] == (C.FRAME_HORIZON_S2_OPS, "a") and layers[0][2][0] is history and layers[0][2][1] is horizon
    assert layers[1] == (C.CONV2D_S2_OPS, "c") and layers[2] == (C.CONV2D_S2_OPS, "e")
    folded = torch.arange(12 * 32 * 2 * 2.0).view(12, 32, 2, 2)
    viewed = layers[3](folded)
    assert tuple(viewed.shape) == (3, 128, 2, 2) and viewed.data_ptr() == folded.data_ptr()
    assert layers[4:] == [(C.CONVT2D_S2_FRAMES_OPS, "g"), (C.CONVT2D_S2_OPS, "i"), (C.CONVT2D_HEAD_OPS, "k")]
