"""CPU: notebooks/10_just_conv.ipynb's LitAutoEncoder.  tests/nb10_reference.py (float64, torch.nn.functional) is pinned to
the golden fixture, which the notebook's own cell produced (tests/golden/make_nb10_golden.py); then the model's output-size
rule, its refusals, the config, the fake datamodule's draws against the notebook's sampler cells and its batch shapes."""
import os

import numpy as np
import pytest
import torch

import nb10_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb10_small.npz")
SAMPLER = os.path.join(ROOT, "tests", "golden", "nb10_sampler.npz")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_golden(tag):
    gold = np.load(GOLDEN)
    batch, p = R.G.draw_batch(tag), R.params64(R.G.draw_parameters())
    y_hat = R.forward64(p, batch)
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape)
    R.check_stored(gold, f"{tag}/y_hat", y_hat, 1e-5)
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    for k, v in p.items():
        R.check_stored(gold, f"{tag}/grad/{k}", v.grad, NORM_TOL)


def test_stripe_planes_of_the_golden_cases():
    """Case a: inside, clipped at the right edge, empty; case b: at column 0, clipped."""
    a = R.input64(R.G.draw_batch("a")["HISTORICAL_SAT_IMAGES"], R.G.draw_batch("a")["FORECAST_HORIZON"])[:, 4]
    assert [int(v) for v in a[:, 0].sum(1)] == [5, 2, 0] and a[0, 3, 5:10].all() and a[1, 0, 45:].all()
    b = R.input64(R.G.draw_batch("b")["HISTORICAL_SAT_IMAGES"], R.G.draw_batch("b")["FORECAST_HORIZON"])[:, 4]
    assert [int(v) for v in b[:, 0].sum(1)] == [5, 4] and b[0, 0, :5].all() and b[1, 0, 50:].all()
    # truncation toward zero, float horizons, the kernel rule for a negative start
    assert R.stripe_plane64(torch.tensor([-3]), 1, 8)[0, 0, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert R.input64(torch.zeros(1, 4, 1, 20), torch.tensor([1.9]))[0, 4, 0].nonzero().flatten().tolist() == [9, 10, 11, 12, 13]


def test_stripe_start_from_horizon_truncates_toward_zero():
    from predict_pv_yield_amd.conv2d_functional import stripe_start_from_horizon
    for h in (torch.tensor([1, 9, 23, 0]), torch.tensor([1.9, -0.3, 23.0, 0.0]), torch.tensor([3, 4], dtype=torch.int32),
              torch.tensor([2.5], dtype=torch.float64)):
        got = stripe_start_from_horizon(h)
        assert got.dtype == torch.int32 and got.tolist() == [int(float(v) * 5) for v in h]


def test_output_side_and_refusals():
    from predict_pv_yield_amd.models.conv2d import nb10_just_conv as M
    assert [M.output_side(s) for s in (128, 47, 46, 5)] == [64, 24, 23, 3]
    with pytest.raises(ValueError, match="at least 5"):
        M.output_side(4)
    M.check_target_side((128, 128), (7, 64, 64))
    M.check_target_side((20, 54), (2, 10, 27))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 63, 64))
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        M.check_target_side((128, 128), (7, 1, 64, 64))
    model = M.LitAutoEncoder()
    assert sum(p.numel() for p in model.parameters()) == 225537
    assert list(model.state_dict()) == [f"conv.{i}.{w}" for i in (0, 2, 4, 6) for w in ("weight", "bias")]
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.G.PARAM_SHAPES
    batch = {"HISTORICAL_SAT_IMAGES": torch.zeros(2, 4, 16, 16), "FORECAST_HORIZON": torch.tensor([1, 2]),
             "TARGET_SAT_IMAGE": torch.zeros(2, 8, 8)}
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        model.training_step({**batch, "TARGET_SAT_IMAGE": torch.zeros(2, 16, 16)}, 0)
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
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb10_just_conv", "datamodule=nb10_fake", "callbacks=none",
                                                              "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb10_just_conv.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb10_datamodule.Nb10DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == 225537 and dm.batch_size == 64 and dm.image_size_pixels == 128
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-3


def test_datamodule_draws_follow_the_notebooks_sampler():
    from predict_pv_yield_amd.data import nb10_datamodule as D
    want = np.load(SAMPLER)["draws"]
    t, h, w = R.G.SAMPLER_SHAPE
    rng = np.random.default_rng(R.G.SAMPLER_SEED)
    got = np.array([D.draw_example(t, h, w, rng) for _ in range(len(want))])
    assert np.array_equal(got, want)
    assert want[:, 1].min() >= 1 and want[:, 1].max() <= 23
    # ... and the crops are the ones the draws name: frames whose pixels encode their own position
    frames = R.G.sampler_frames()
    rng = np.random.default_rng(R.G.SAMPLER_SEED)
    for hist_start, horizon, top, left in want[:8]:
        ex = D.super_batch_to_example(frames, rng)
        assert ex["FORECAST_HORIZON"] == horizon and ex["HISTORICAL_SAT_IMAGES"].shape == (4, 128, 128)
        assert ex["HISTORICAL_SAT_IMAGES"][0, 0, 0] == hist_start * 1e6 + top * 1e3 + left
        assert ex["HISTORICAL_SAT_IMAGES"][3, 127, 127] == (hist_start + 3) * 1e6 + (top + 127) * 1e3 + left + 127
        assert ex["TARGET_SAT_IMAGE"].shape == (64, 64)
        assert ex["TARGET_SAT_IMAGE"][0, 0] == (hist_start + 3 + horizon) * 1e6 + (top + 32) * 1e3 + left + 32


def test_datamodule_batches_on_the_cpu():
    from predict_pv_yield_amd.data import nb10_datamodule as D
    dm = D.Nb10DataModule(batch_size=3, n_train_data=2, n_val_data=1, n_super_batches=1, n_timesteps=12, device="cpu")
    batch = next(iter(dm.train_dataloader()))
    assert set(batch) == {"HISTORICAL_SAT_IMAGES", "FORECAST_HORIZON", "TARGET_SAT_IMAGE"}
    assert tuple(batch["HISTORICAL_SAT_IMAGES"].shape) == (3, 4, 128, 128) and batch["HISTORICAL_SAT_IMAGES"].dtype == torch.float32
    assert tuple(batch["TARGET_SAT_IMAGE"].shape) == (3, 64, 64) and batch["TARGET_SAT_IMAGE"].dtype == torch.float32
    assert batch["FORECAST_HORIZON"].dtype == torch.int64 and 1 <= int(batch["FORECAST_HORIZON"].min())
    assert float(batch["HISTORICAL_SAT_IMAGES"].abs().max()) < 10.0           # normalised in the loader
    assert len(list(dm.val_dataloader())) == 1
    with pytest.raises(ValueError, match="even border"):
        D.make_fake_nb10_batch(np.zeros((12, 176, 176), np.float32), 2, 127, np.random.default_rng(0), "cpu")


def test_entry_points_refuse_bad_arguments_without_launching():
    """An unsupported channel pair, padding 1, a plane 129 columns wide, a null pointer, a short workspace: the ABI's error
    code and a message, from pointers that are never dereferenced."""
    import ctypes
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    for c_in, c_out in ((32, 128), (128, 64), (64, 64), (144, 144)):
        assert lib.pv_conv2d_wide_fwd_f32(p, p, p, p, 2, c_in, c_out, 20, 20, 0, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv2d_wide_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 20, 20, 2, None) == ESIZE
        assert lib.pv_conv2d_wide_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 20, 20, 0, p, 1 << 30, None) == ESIZE
    assert lib.pv_conv2d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 20, 20, 1, 1, None) == ESIZE and "padding" in err()
    assert lib.pv_conv2d_wide_bwd_data_f32(p, None, p, p, None, 2, 64, 128, 20, 20, 1, None) == ESIZE
    assert lib.pv_conv2d_wide_bwd_weight_workspace_bytes(2, 64, 128, 20, 20, 1, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 20, 129, 0, 1, None) == ESIZE and "128" in err()
    assert lib.pv_conv2d_wide_fwd_f32(p, p, p, p, 2, 64, 128, 2, 20, 0, 1, None) == ESIZE
    assert lib.pv_conv2d_wide_fwd_f32(p, p, p, p, 1 << 14, 128, 128, 128, 128, 0, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_conv2d_wide_fwd_f32(None, p, p, p, 2, 64, 128, 20, 20, 0, 1, None) == EINVAL and "null" in err()
    assert lib.pv_conv2d_wide_bwd_data_f32(p, None, p, None, None, 2, 64, 128, 20, 20, 0, None) == EINVAL
    assert lib.pv_conv2d_wide_bwd_weight_workspace_bytes(2, 64, 128, 20, 20, 0, None) == EINVAL
    assert lib.pv_conv2d_wide_bwd_weight_workspace_bytes(2, 64, 128, 20, 20, 2, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_wide_bwd_weight_f32(p, p, None, p, p, 2, 64, 128, 20, 20, 2, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_conv2d_wide_stripe_fwd_f32(p, p, p, p, p, 2, 8, 20, 20, 64, 5, None) == ESIZE and "history" in err()
    assert lib.pv_conv2d_wide_stripe_fwd_f32(p, p, p, p, p, 2, 4, 20, 20, 32, 5, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv2d_wide_stripe_fwd_f32(p, p, p, p, p, 2, 4, 20, 129, 64, 5, None) == ESIZE
    assert lib.pv_conv2d_wide_stripe_fwd_f32(p, None, p, p, p, 2, 4, 20, 20, 64, 5, None) == EINVAL
    assert lib.pv_conv2d_wide_stripe_bwd_weight_f32(p, p, p, p, p, 2, 4, 20, 20, 64, 5, p, 16, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_conv2d_head_s2_fwd_f32(p, p, p, p, 2, 128, 2, 20, 20, 0, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv2d_head_s2_fwd_f32(p, None, p, p, 2, 128, 1, 20, 20, 0, None) == EINVAL
    assert lib.pv_conv2d_head_s2_bwd_data_f32(p, p, p, p, None, 2, 128, 1, 20, 20, None) == EINVAL and "dy_gate" in err()
    assert lib.pv_conv2d_head_s2_bwd_weight_workspace_bytes(2, 128, 1, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_head_s2_bwd_weight_f32(p, p, None, p, p, 2, 128, 1, 20, 20, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
