"""CPU: notebooks/08_multiple_historical_images_as_separate_channels.ipynb's LitAutoEncoder.  tests/nb08_reference.py (float64,
torch.nn.functional) is pinned to the golden fixture, which the notebook's own cell produced
(tests/golden/make_nb08_golden.py); then the model's names, count and output-size rule, its refusals, the configs, the fake
datamodule's draws against the notebook's sampler (the fixture notebook 10's identical cells produced) and its target side,
and the C ABI's glue and refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nb08_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT, _golden_module, _rel
from notebook_model_checks import check_fit64
from test_conv2d_glue_cpu import T, check_glue_case, check_new_symbols

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb08_small.npz")
SAMPLER = os.path.join(ROOT, "tests", "golden", "nb10_sampler.npz")
NEW_SYMBOLS = {"pv_conv3d_s2_fwd_f32": 12, "pv_conv3d_s2_bwd_data_f32": 12, "pv_conv3d_s2_bwd_weight_workspace_bytes": 7,
               "pv_conv3d_s2_bwd_weight_f32": 14, "pv_convt2d_s2_horizon_fwd_f32": 10,
               "pv_convt2d_s2_horizon_bwd_weight_workspace_bytes": 4, "pv_convt2d_s2_horizon_bwd_weight_f32": 12}
N_PARAMS = 42329


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


def test_depth_pair_identity_in_float64():
    """A depth-2 strided Conv3d on [n, c, d, h, w] is a stride-2 Conv2d with 2 c input channels per output depth: virtual
    channel 2 c + kd is the plane (c, z + kd), and the [m, c, 2, 3, 3] weight as it lies in memory is the [m, 2 c, 3, 3] one.
    The difference is exactly 0."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 8, 4, 9, 12, generator=g, dtype=torch.float64)
    w = torch.randn(32, 8, 2, 3, 3, generator=g, dtype=torch.float64)
    y = F.conv3d(x, w, stride=(1, 2, 2))
    for z in range(3):
        pair = x[:, :, z:z + 2].reshape(2, 16, 9, 12)
        assert torch.equal(y[:, :, z], F.conv2d(pair, w.view(32, 16, 3, 3), stride=2))


def test_names_shapes_count_and_size_rule():
    from predict_pv_yield_amd.models.conv3d import nb08_hist_depth as M
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
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS
    assert list(model.state_dict()) == [f"{part}_conv.{i}.{w}" for part in ("encoder", "decoder") for i in (0, 2, 4)
                                        for w in ("weight", "bias")]
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.G.PARAM_SHAPES
    # the depth chain 4 -> 3 -> 2 -> 1 and the sides of the two nn.Sequential the model holds, on the CPU
    for h, w in ((15, 15), (31, 23), (128, 128)):
        enc = model.encoder_conv(torch.zeros(1, 1, 4, h, w))
        assert enc.shape[:3] == (1, 32, 1)
        dec = model.decoder_conv(torch.cat((enc.squeeze(2), torch.zeros(1, 1, *enc.shape[3:])), dim=1))
        assert tuple(dec.shape) == (1, 1, M.output_side(h), M.output_side(w))
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 1e-3
    assert M.LitAutoEncoder(lr=1e-4).configure_optimizers().param_groups[0]["lr"] == 1e-4


def test_model_refusals_on_the_cpu():
    from predict_pv_yield_amd.models.conv3d import nb08_hist_depth as M
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
    # three or five history frames, a depth axis already there, no batch axis: refused before the device is looked at
    for hist in (z(2, 3, 31, 31), z(2, 5, 31, 31), z(2, 1, 4, 31, 31), z(4, 31, 31)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({"HISTORICAL_SAT_IMAGES": hist, "FORECAST_HORIZON": z(2)})


def test_glue_refuses_bad_shapes_before_touching_a_device():
    from predict_pv_yield_amd import hip_ops as K
    z = torch.zeros
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.conv3d_s2_fwd_f32(z(1, 16, 3, 8, 8), z(32, 16, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="2, 3, 3"):
        K.conv3d_s2_fwd_f32(z(1, 8, 3, 8, 8), z(32, 8, 3, 3, 3), z(32))
    with pytest.raises(ValueError, match="two slices"):
        K.conv3d_s2_fwd_f32(z(1, 8, 1, 8, 8), z(32, 8, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        K.conv3d_s2_fwd_f32(z(1, 8, 2, 8, 129), z(32, 8, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="bias"):
        K.conv3d_s2_fwd_f32(z(1, 8, 2, 8, 8), z(32, 8, 2, 3, 3), z(8))
    with pytest.raises(ValueError, match="dy"):
        K.conv3d_s2_bwd_data_f32(z(1, 32, 2, 4, 4), None, z(32, 8, 2, 3, 3), None, (1, 8, 3, 8, 8))
    with pytest.raises(ValueError, match="no data gradient"):
        K.conv3d_s2_bwd_data_f32(z(1, 8, 2, 3, 3), None, z(8, 1, 2, 3, 3), None, (1, 1, 3, 8, 8))
    with pytest.raises(ValueError, match="dy"):
        K.conv3d_s2_bwd_weight_f32(z(1, 8, 3, 8, 8), z(1, 32, 2, 3, 4), None, (32, 8, 2, 3, 3))
    with pytest.raises(ValueError, match="weight"):
        K.convt2d_s2_horizon_fwd_f32(z(2, 32, 4, 4), z(2), z(32, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="x \\[N, 32"):
        K.convt2d_s2_horizon_fwd_f32(z(2, 33, 4, 4), z(2), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="horizon"):
        K.convt2d_s2_horizon_fwd_f32(z(2, 32, 4, 4), z(3), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        K.convt2d_s2_horizon_fwd_f32(z(2, 32, 4, 64), z(2), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="dy"):
        K.convt2d_s2_horizon_bwd_weight_f32(z(2, 32, 4, 4), z(2), z(2, 32, 8, 9), None, (33, 32, 3, 3))


def test_config_composes_and_instantiates():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb08_hist_depth", "datamodule=nb08_fake",
                                                              "callbacks=none", "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv3d.nb08_hist_depth.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb08_datamodule.Nb08DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS and dm.batch_size == 64 and dm.image_size_pixels == 128
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-3


def test_datamodule_follows_the_sampler_and_this_models_target_side():
    from predict_pv_yield_amd.data import nb08_datamodule as D
    from predict_pv_yield_amd.data import nb12_datamodule as D12
    from predict_pv_yield_amd.models.conv3d import nb08_hist_depth as M
    from predict_pv_yield_amd.models.conv3d import nb12_just_3d_conv as M12
    g10 = _golden_module("nb10")
    want = np.load(SAMPLER)["draws"]
    # the crops are the ones the notebook's sampler draws name (frames whose pixels encode their own position)
    frames = g10.sampler_frames()
    rng = np.random.default_rng(g10.SAMPLER_SEED)
    batch = D.make_fake_nb08_batch(frames, 4, 128, rng, "cpu")
    seq = np.arange(1, 25, dtype=np.float32)
    for i, (hist_start, horizon, top, left) in enumerate(want[:4]):
        assert batch["FORECAST_HORIZON"][i].item() == (np.float32(horizon) - seq.mean()) / seq.std()
        assert batch["HISTORICAL_SAT_IMAGES"][i, 0, 0, 0] == hist_start * 1e6 + top * 1e3 + left
        assert batch["TARGET_SAT_IMAGE"][i, 0, 0] == (hist_start + 3 + horizon) * 1e6 + (top + 32) * 1e3 + left + 32
    assert tuple(batch["TARGET_SAT_IMAGE"].shape) == (4, 64, 64)
    # at 128 the two notebooks' rules agree, and the module's batches are notebook 12's ...
    kw = dict(batch_size=3, n_train_data=2, n_val_data=1, n_super_batches=1, n_timesteps=12, device="cpu")
    b08, b12 = next(iter(D.Nb08DataModule(**kw).train_dataloader())), next(iter(D12.Nb12DataModule(**kw).train_dataloader()))
    assert set(b08) == {"HISTORICAL_SAT_IMAGES", "FORECAST_HORIZON", "TARGET_SAT_IMAGE"}
    for k in b08:
        assert torch.equal(b08[k], b12[k]) and b08[k].dtype == torch.float32
    assert len(list(D.Nb08DataModule(**kw).val_dataloader())) == 1
    # ... but not at every size: 42 -> 20 here (border 11 a side), 21 by notebook 12's rule
    assert M.target_side(42) == 20 and M12.output_side(42) == 21
    small = next(iter(D.Nb08DataModule(**{**kw, "image_size_pixels": 42}).train_dataloader()))
    assert tuple(small["HISTORICAL_SAT_IMAGES"].shape) == (3, 4, 42, 42) and tuple(small["TARGET_SAT_IMAGE"].shape) == (3, 20, 20)
    M.check_target_side((42, 42), small["TARGET_SAT_IMAGE"].shape)
    # 41 -> 20 (notebook 12: 21): a border of 21 pixels cannot be centred
    with pytest.raises(ValueError, match="even border"):
        D.make_fake_nb08_batch(np.zeros((12, 176, 176), np.float32), 2, 41, np.random.default_rng(0), "cpu")


def test_new_symbols_are_declared_and_bound_with_matching_arity():
    check_new_symbols(NEW_SYMBOLS, "08_multiple_historical_images_as_separate_channels.ipynb")


def test_entry_points_refuse_bad_arguments_without_launching():
    """An unsupported channel pair, the first layer's data gradient, depth 1, a plane under 3 or over 128 wide, a tensor
    beyond 32-bit indexing, a null pointer, a short workspace: the ABI's error code and a message, from pointers that are
    never dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    for c_in, c_out in ((16, 32), (32, 8), (1, 32), (8, 8), (33, 32)):
        assert lib.pv_conv3d_s2_fwd_f32(p, p, p, p, 2, c_in, c_out, 3, 20, 20, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv3d_s2_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 3, 20, 20, None) == ESIZE
        assert lib.pv_conv3d_s2_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 3, 20, 20, p, 1 << 30, None) == ESIZE
        assert lib.pv_conv3d_s2_bwd_weight_workspace_bytes(2, c_in, c_out, 3, 20, 20, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv3d_s2_bwd_data_f32(p, None, p, p, None, 2, 1, 8, 3, 20, 20, None) == ESIZE and "no data gradient" in err()
    assert lib.pv_conv3d_s2_fwd_f32(p, p, p, p, 2, 8, 32, 1, 20, 20, 1, None) == ESIZE and "kernel" in err()
    assert lib.pv_conv3d_s2_fwd_f32(p, p, p, p, 2, 8, 32, 2, 2, 20, 1, None) == ESIZE and "kernel" in err()
    assert lib.pv_conv3d_s2_fwd_f32(p, p, p, p, 2, 8, 32, 2, 20, 129, 1, None) == ESIZE and "128" in err()
    assert lib.pv_conv3d_s2_fwd_f32(p, p, p, p, 1 << 14, 32, 32, 4, 128, 128, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_conv3d_s2_fwd_f32(p, p, p, p, 0, 8, 32, 2, 20, 20, 1, None) == EINVAL
    assert lib.pv_conv3d_s2_fwd_f32(None, p, p, p, 2, 8, 32, 2, 20, 20, 1, None) == EINVAL and "null" in err()
    assert lib.pv_conv3d_s2_fwd_f32(p, p, None, p, 2, 8, 32, 2, 20, 129, 1, None) == ESIZE      # a null bias is allowed
    assert lib.pv_conv3d_s2_bwd_data_f32(p, None, p, None, None, 2, 8, 32, 3, 20, 20, None) == EINVAL
    assert lib.pv_conv3d_s2_bwd_weight_workspace_bytes(2, 8, 32, 3, 20, 20, None) == EINVAL
    assert lib.pv_conv3d_s2_bwd_weight_workspace_bytes(2, 8, 32, 3, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv3d_s2_bwd_weight_f32(p, p, None, p, p, 2, 8, 32, 3, 20, 20, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_conv3d_s2_bwd_weight_f32(p, p, None, p, p, 2, 8, 32, 3, 20, 20, None, need.value, None) == EINVAL
    # the horizon ConvTranspose2d
    assert lib.pv_convt2d_s2_horizon_fwd_f32(p, p, p, p, p, 2, 15, 64, 1, None) == ESIZE and "width" in err()
    assert lib.pv_convt2d_s2_horizon_fwd_f32(p, p, p, p, p, 2, 0, 15, 1, None) == EINVAL
    assert lib.pv_convt2d_s2_horizon_fwd_f32(p, None, p, p, p, 2, 15, 15, 1, None) == EINVAL and "null" in err()
    assert lib.pv_convt2d_s2_horizon_fwd_f32(p, p, p, p, p, 1 << 20, 63, 63, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_convt2d_s2_horizon_bwd_weight_workspace_bytes(2, 15, 64, ctypes.byref(need)) == ESIZE
    assert lib.pv_convt2d_s2_horizon_bwd_weight_workspace_bytes(2, 15, 15, None) == EINVAL
    assert lib.pv_convt2d_s2_horizon_bwd_weight_workspace_bytes(2, 15, 15, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_convt2d_s2_horizon_bwd_weight_f32(p, p, p, None, p, p, 2, 15, 15, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_convt2d_s2_horizon_bwd_weight_f32(p, p, None, None, p, p, 2, 15, 15, p, need.value, None) == EINVAL


# ---- what the new wrappers hand to the C ABI (the harness of tests/test_conv2d_glue_cpu.py) --------------------------------
X8, Y32, W8 = (2, 8, 3, 10, 12), (2, 32, 2, 4, 5), (32, 8, 2, 3, 3)
GLUE = {
    "conv3d_s2_fwd": (
        "conv3d_s2_fwd_f32", dict(x=T(*X8), weight=T(*W8), bias=T(32), relu=True),
        ["require_cuda", "pv_conv3d_s2_fwd_f32 x weight bias out0 2 8 32 3 10 12 1 stream"], ["(2, 32, 2, 4, 5) float32"], []),
    "conv3d_s2_fwd/none": (
        "conv3d_s2_fwd_f32", dict(x=T(2, 1, 4, 9, 11), weight=T(8, 1, 2, 3, 3), bias=None, relu=False),
        ["require_cuda", "pv_conv3d_s2_fwd_f32 x weight NULL out0 2 1 8 4 9 11 0 stream"], ["(2, 8, 3, 4, 5) float32"], []),
    "conv3d_s2_bwd_data": (
        "conv3d_s2_bwd_data_f32", dict(dy=T(*Y32), dy_gate=None, weight=T(*W8), x_gate=T(*X8), x_shape=X8),
        ["require_cuda", "pv_conv3d_s2_bwd_data_f32 dy NULL weight out0 x_gate 2 8 32 3 10 12 stream"],
        ["(2, 8, 3, 10, 12) float32"], []),
    "conv3d_s2_bwd_weight": (
        "conv3d_s2_bwd_weight_f32", dict(x=T(*X8), dy=T(*Y32), dy_gate=T(*Y32), weight_shape=W8),
        ["require_cuda", "pv_conv3d_s2_bwd_weight_workspace_bytes 2 8 32 3 10 12 &bytes",
         "pv_conv3d_s2_bwd_weight_f32 x dy dy_gate out0 out1 2 8 32 3 10 12 ws:conv3d_s2_wgrad 4096 stream"],
        ["(32, 8, 2, 3, 3) float32", "(32,) float32"], ["conv3d_s2_wgrad"]),
    "convt2d_s2_horizon_fwd": (
        "convt2d_s2_horizon_fwd_f32", dict(x=T(2, 32, 4, 5), horizon=T(2), weight=T(33, 32, 3, 3), bias=T(32), relu=True),
        ["require_cuda", "pv_convt2d_s2_horizon_fwd_f32 x horizon weight bias out0 2 4 5 1 stream"],
        ["(2, 32, 9, 11) float32"], []),
    "convt2d_s2_horizon_bwd_weight": (
        "convt2d_s2_horizon_bwd_weight_f32", dict(x=T(2, 32, 4, 5), horizon=T(2), dy=T(2, 32, 9, 11), dy_gate=T(2, 32, 9, 11),
                                                  weight_shape=(33, 32, 3, 3)),
        ["require_cuda", "pv_convt2d_s2_horizon_bwd_weight_workspace_bytes 2 4 5 &bytes",
         "pv_convt2d_s2_horizon_bwd_weight_f32 x horizon dy dy_gate out0 out1 2 4 5 ws:convt2d_s2_horizon_wgrad 4096 stream"],
        ["(33, 32, 3, 3) float32", "(32,) float32"], ["convt2d_s2_horizon_wgrad"]),
}


@pytest.mark.parametrize("case_id", sorted(GLUE))
def test_new_wrappers_hand_the_abi_what_the_table_pins(monkeypatch, case_id):
    check_glue_case(monkeypatch, GLUE[case_id])


def test_functional_tuple_names_the_new_family():
    from predict_pv_yield_amd import conv3d_wide_functional as C
    from predict_pv_yield_amd import hip_ops as K
    assert C.CONV3D_S2_OPS == (K.conv3d_s2_fwd_f32, K.conv3d_s2_bwd_data_f32, K.conv3d_s2_bwd_weight_f32)
