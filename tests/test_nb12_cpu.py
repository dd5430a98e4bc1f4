"""CPU: notebooks/12_just_3d_conv.ipynb's LitAutoEncoder.  tests/nb12_reference.py (float64, torch.nn.functional) is pinned to
the golden fixture, which the notebook's own cell produced (tests/golden/make_nb12_golden.py); then the model's output-size
rule, its refusals, the config, the fake datamodule's draws against the notebook's sampler cells (the fixture notebook 10's
identical cells produced), its horizons against the notebook's formula, and the C ABI's glue and refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nb12_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT, _golden_module
from test_conv2d_glue_cpu import check_new_symbols

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb12_small.npz")
SAMPLER = os.path.join(ROOT, "tests", "golden", "nb10_sampler.npz")
NEW_SYMBOLS = {"pv_conv3d_wide_fwd_f32": 14, "pv_conv3d_wide_bwd_data_f32": 14, "pv_conv3d_wide_bwd_weight_workspace_bytes": 9,
               "pv_conv3d_wide_bwd_weight_f32": 16, "pv_conv3d_wide_horizon_fwd_f32": 11,
               "pv_conv3d_wide_horizon_bwd_weight_workspace_bytes": 6, "pv_conv3d_wide_horizon_bwd_weight_f32": 13,
               "pv_conv2d_head_s2p1_fwd_f32": 11, "pv_conv2d_head_s2p1_bwd_data_f32": 11,
               "pv_conv2d_head_s2p1_bwd_weight_workspace_bytes": 6, "pv_conv2d_head_s2p1_bwd_weight_f32": 13}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_golden(tag):
    gold = np.load(GOLDEN)
    batch, p = R.G.draw_batch(tag), R.params64(R.G.draw_parameters())
    y_hat = R.forward64(p, batch)
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape) and y_hat.shape[1:3] == (1, 1)
    R.check_stored(gold, f"{tag}/y_hat", y_hat, 1e-5)
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    for k, v in p.items():
        R.check_stored(gold, f"{tag}/grad/{k}", v.grad, NORM_TOL)


def test_reference_input_and_horizons():
    """The second channel is the example's horizon at every depth and pixel; the golden's horizons are the loader's formula."""
    x = R.input64(torch.arange(2 * 4 * 2 * 3, dtype=torch.float32).view(2, 4, 2, 3), torch.tensor([0.5, -1.25]))
    assert tuple(x.shape) == (2, 2, 4, 2, 3)
    assert (x[0, 1] == 0.5).all() and (x[1, 1] == -1.25).all() and x[1, 0, 3, 1, 2] == 47.0
    seq = np.arange(1, 25, dtype=np.float32)
    for tag, steps in (("a", (1, 9, 23)), ("b", (12, 24))):
        want = [(np.float32(t) - seq.mean()) / seq.std() for t in steps]
        assert R.G.draw_batch(tag)["FORECAST_HORIZON"].tolist() == [float(v) for v in want]


def test_output_side_and_refusals():
    from predict_pv_yield_amd.models.conv3d import nb12_just_3d_conv as M
    assert [M.output_side(s) for s in (128, 47, 46, 2, 1)] == [64, 24, 23, 1, 1]
    with pytest.raises(ValueError, match="at least 1"):
        M.output_side(0)
    M.check_target_side((128, 128), (7, 64, 64))
    M.check_target_side((47, 20), (2, 24, 10))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 63, 64))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 1, 64, 64))
    model = M.LitAutoEncoder()
    assert sum(p.numel() for p in model.parameters()) == 742337
    assert list(model.state_dict()) == [f"conv.{i}.{w}" for i in (0, 2, 4, 6, 8) for w in ("weight", "bias")]
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.G.PARAM_SHAPES
    # the depth chain 4 -> 3 -> 2 -> 3 -> 2 -> 1 and the sides of the nn.Sequential the model holds, on the CPU
    for h, w in ((1, 1), (2, 2), (47, 20)):
        assert tuple(model.conv(torch.zeros(1, 2, 4, h, w)).shape) == (1, 1, 1, M.output_side(h), M.output_side(w))
    batch = {"HISTORICAL_SAT_IMAGES": torch.zeros(2, 4, 16, 16), "FORECAST_HORIZON": torch.tensor([0.1, -0.2]),
             "TARGET_SAT_IMAGE": torch.zeros(2, 8, 8)}
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        model.training_step({**batch, "TARGET_SAT_IMAGE": torch.zeros(2, 16, 16)}, 0)
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 1e-4
    assert M.LitAutoEncoder(lr=1e-3).configure_optimizers().param_groups[0]["lr"] == 1e-3


def test_glue_refuses_bad_shapes_before_touching_a_device():
    """History that is not [B, 4, S, S] (the model), and the kernels' shape rules (hip_ops): all ValueError on CPU tensors,
    raised before the device check."""
    from predict_pv_yield_amd import hip_ops as K
    from predict_pv_yield_amd.conv3d_wide_functional import conv3d_wide_relu
    z = torch.zeros
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.conv3d_wide_fwd_f32(z(1, 32, 3, 8, 8), z(128, 32, 2, 3, 3), z(128))
    with pytest.raises(ValueError, match="2, 3, 3"):
        K.conv3d_wide_fwd_f32(z(1, 64, 3, 8, 8), z(128, 64, 3, 3, 3), z(128))
    with pytest.raises(ValueError, match="padding"):
        K.conv3d_wide_fwd_f32(z(1, 64, 3, 8, 8), z(128, 64, 2, 3, 3), z(128), padding=(2, 1, 1))
    with pytest.raises(ValueError, match="padding"):
        K.conv3d_wide_bwd_weight_f32(z(1, 64, 3, 8, 8), z(1, 128, 2, 8, 8), None, (128, 64, 2, 3, 3), padding=(0, 2, 2))
    with pytest.raises(ValueError, match="padding"):
        conv3d_wide_relu(z(1, 64, 3, 8, 8), z(128, 64, 2, 3, 3), z(128), padding=(0, 0, 1))
    with pytest.raises(ValueError, match="one slice"):
        K.conv3d_wide_fwd_f32(z(1, 64, 1, 8, 8), z(128, 64, 2, 3, 3), z(128))
    with pytest.raises(ValueError, match="128 columns"):
        K.conv3d_wide_fwd_f32(z(1, 64, 2, 8, 129), z(128, 64, 2, 3, 3), z(128))
    with pytest.raises(ValueError, match="dy"):
        K.conv3d_wide_bwd_data_f32(z(1, 128, 3, 8, 8), None, z(128, 64, 2, 3, 3), None, (1, 64, 3, 8, 8))
    with pytest.raises(ValueError, match="history"):
        K.conv3d_wide_horizon_fwd_f32(z(2, 1, 8, 8), z(2), z(64, 2, 2, 3, 3), z(64))
    with pytest.raises(ValueError, match="weight"):
        K.conv3d_wide_horizon_fwd_f32(z(2, 4, 8, 8), z(2), z(64, 2, 3, 3, 3), z(64))
    with pytest.raises(ValueError, match="depth 2"):
        K.conv3d_head_d2_fwd_f32(z(1, 128, 3, 8, 8), z(1, 128, 2, 3, 3), z(1))
    with pytest.raises(ValueError, match="depth 2"):
        K.conv3d_head_d2_bwd_data_f32(z(1, 1, 1, 4, 4), None, z(1, 128, 2, 3, 3), None, (1, 128, 1, 8, 8))
    assert [K.head_s2p1_out(s) for s in (1, 2, 3, 128)] == [1, 1, 2, 64]
    # the model refuses a history that is not [B, 4, S, S] before it looks at the device
    from predict_pv_yield_amd.models.conv3d import nb12_just_3d_conv as M
    model = M.LitAutoEncoder()
    for hist in (z(2, 3, 16, 16), z(2, 5, 16, 16), z(2, 1, 4, 16, 16), z(4, 16, 16)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({"HISTORICAL_SAT_IMAGES": hist, "FORECAST_HORIZON": z(2)})


def test_config_composes_and_instantiates():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb12_just_3d_conv", "datamodule=nb12_fake",
                                                              "callbacks=none", "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv3d.nb12_just_3d_conv.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb12_datamodule.Nb12DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == 742337 and dm.batch_size == 64 and dm.image_size_pixels == 128
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-4


def test_datamodule_draws_follow_the_notebooks_sampler():
    from predict_pv_yield_amd.data import nb12_datamodule as D
    g10 = _golden_module("nb10")
    want = np.load(SAMPLER)["draws"]
    t, h, w = g10.SAMPLER_SHAPE
    rng = np.random.default_rng(g10.SAMPLER_SEED)
    got = np.array([D.draw_example(t, h, w, rng) for _ in range(len(want))])
    assert np.array_equal(got, want)
    # ... the crops are the ones the draws name (frames whose pixels encode their own position), the horizon the notebook's
    # normalise_forecast_horizon of the drawn timesteps, in float32
    frames = g10.sampler_frames()
    rng = np.random.default_rng(g10.SAMPLER_SEED)
    seq = np.arange(1, 25, dtype=np.float32)
    for hist_start, horizon, top, left in want[:8]:
        ex = D.super_batch_to_example(frames, rng)
        assert ex["FORECAST_HORIZON"].dtype == np.float32
        assert ex["FORECAST_HORIZON"] == (np.float32(horizon) - seq.mean()) / seq.std()
        assert ex["FORECAST_HORIZON"] == R.G.normalise_forecast_horizon(int(horizon))
        assert ex["HISTORICAL_SAT_IMAGES"].shape == (4, 128, 128)
        assert ex["HISTORICAL_SAT_IMAGES"][0, 0, 0] == hist_start * 1e6 + top * 1e3 + left
        assert ex["HISTORICAL_SAT_IMAGES"][3, 127, 127] == (hist_start + 3) * 1e6 + (top + 127) * 1e3 + left + 127
        assert ex["TARGET_SAT_IMAGE"].shape == (64, 64)
        assert ex["TARGET_SAT_IMAGE"][0, 0] == (hist_start + 3 + horizon) * 1e6 + (top + 32) * 1e3 + left + 32
    assert abs(float(D.normalise_forecast_horizon(3)) - (-1.3724)) < 1e-4 and D.FCST_HORIZON_MEAN == 12.5


def test_datamodule_batches_on_the_cpu():
    from predict_pv_yield_amd.data import nb10_datamodule as D10
    from predict_pv_yield_amd.data import nb12_datamodule as D
    kw = dict(batch_size=3, n_train_data=2, n_val_data=1, n_super_batches=1, n_timesteps=12, device="cpu")
    dm = D.Nb12DataModule(**kw)
    batch = next(iter(dm.train_dataloader()))
    assert set(batch) == {"HISTORICAL_SAT_IMAGES", "FORECAST_HORIZON", "TARGET_SAT_IMAGE"}
    assert tuple(batch["HISTORICAL_SAT_IMAGES"].shape) == (3, 4, 128, 128) and batch["HISTORICAL_SAT_IMAGES"].dtype == torch.float32
    assert tuple(batch["TARGET_SAT_IMAGE"].shape) == (3, 64, 64) and batch["TARGET_SAT_IMAGE"].dtype == torch.float32
    assert batch["FORECAST_HORIZON"].dtype == torch.float32 and tuple(batch["FORECAST_HORIZON"].shape) == (3,)
    assert len(list(dm.val_dataloader())) == 1
    # the same draws as notebook 10's module: same images, and its integer horizons normalised
    b10 = next(iter(D10.Nb10DataModule(**kw).train_dataloader()))
    assert torch.equal(b10["HISTORICAL_SAT_IMAGES"], batch["HISTORICAL_SAT_IMAGES"])
    assert torch.equal(b10["TARGET_SAT_IMAGE"], batch["TARGET_SAT_IMAGE"])
    assert batch["FORECAST_HORIZON"].tolist() == [float(D.normalise_forecast_horizon(int(h))) for h in b10["FORECAST_HORIZON"]]
    with pytest.raises(ValueError, match="even border"):
        D.make_fake_nb12_batch(np.zeros((12, 176, 176), np.float32), 2, 127, np.random.default_rng(0), "cpu")


def test_new_symbols_are_declared_and_bound_with_matching_arity():
    check_new_symbols(NEW_SYMBOLS)


def test_entry_points_refuse_bad_arguments_without_launching():
    """An unsupported channel pair, depth padding 2, spatial padding other than 1, a plane 129 columns wide, depth 1 without
    depth padding, a null pointer, a short workspace: the ABI's error code and a message, from pointers that are never
    dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    for c_in, c_out in ((32, 128), (128, 64), (64, 64), (56, 128)):
        assert lib.pv_conv3d_wide_fwd_f32(p, p, p, p, 2, c_in, c_out, 3, 20, 20, 0, 1, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv3d_wide_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 3, 20, 20, 1, 1, None) == ESIZE
        assert lib.pv_conv3d_wide_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 3, 20, 20, 0, 1, p, 1 << 30, None) == ESIZE
    assert lib.pv_conv3d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 3, 20, 20, 2, 1, 1, None) == ESIZE and "depth padding" in err()
    assert lib.pv_conv3d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 3, 20, 20, 0, 0, 1, None) == ESIZE and "spatial padding" in err()
    assert lib.pv_conv3d_wide_bwd_data_f32(p, None, p, p, None, 2, 64, 128, 3, 20, 20, 0, 2, None) == ESIZE
    assert lib.pv_conv3d_wide_bwd_weight_workspace_bytes(2, 64, 128, 3, 20, 20, -1, 1, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv3d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 3, 20, 129, 0, 1, 1, None) == ESIZE and "128" in err()
    assert lib.pv_conv3d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 1, 20, 20, 0, 1, 1, None) == ESIZE and "depth" in err()
    assert lib.pv_conv3d_wide_fwd_f32(p, p, p, p, 1 << 13, 128, 128, 3, 128, 128, 0, 1, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_conv3d_wide_fwd_f32(None, p, p, p, 2, 64, 128, 3, 20, 20, 0, 1, 1, None) == EINVAL and "null" in err()
    assert lib.pv_conv3d_wide_bwd_data_f32(p, None, p, None, None, 2, 64, 128, 3, 20, 20, 0, 1, None) == EINVAL
    assert lib.pv_conv3d_wide_bwd_weight_workspace_bytes(2, 64, 128, 3, 20, 20, 0, 1, None) == EINVAL
    assert lib.pv_conv3d_wide_bwd_weight_workspace_bytes(2, 64, 128, 1, 20, 20, 1, 1, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv3d_wide_bwd_weight_f32(p, p, None, p, p, 2, 64, 128, 1, 20, 20, 1, 1, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    # the horizon first layer: 64 output channels, at least two slices, a horizon pointer
    assert lib.pv_conv3d_wide_horizon_fwd_f32(p, p, p, p, p, 2, 4, 20, 20, 128, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv3d_wide_horizon_fwd_f32(p, p, p, p, p, 2, 1, 20, 20, 64, None) == ESIZE and "depth" in err()
    assert lib.pv_conv3d_wide_horizon_fwd_f32(p, p, p, p, p, 2, 4, 20, 129, 64, None) == ESIZE
    assert lib.pv_conv3d_wide_horizon_fwd_f32(p, None, p, p, p, 2, 4, 20, 20, 64, None) == EINVAL
    assert lib.pv_conv3d_wide_horizon_bwd_weight_workspace_bytes(2, 4, 20, 20, 64, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv3d_wide_horizon_bwd_weight_f32(p, p, p, p, p, 2, 4, 20, 20, 64, p, need.value - 1, None) == EINVAL
    # the head: one output channel, no dy_gate
    assert lib.pv_conv2d_head_s2p1_fwd_f32(p, p, p, p, 2, 256, 2, 20, 20, 0, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv2d_head_s2p1_bwd_data_f32(p, p, p, p, None, 2, 256, 1, 20, 20, None) == EINVAL and "dy_gate" in err()
    assert lib.pv_conv2d_head_s2p1_bwd_weight_workspace_bytes(2, 256, 1, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_head_s2p1_bwd_weight_f32(p, p, None, p, p, 2, 256, 1, 20, 20, p, need.value - 1, None) == EINVAL
    # the existing padded Conv2d family keeps its refusals: padding 1 is still not one of its shapes
    assert lib.pv_conv2d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 20, 20, 1, 1, None) == ESIZE and "padding" in err()
