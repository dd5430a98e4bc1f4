"""CPU: the stride-2 LitAutoEncoder of notebooks 14 / 15 -- the golden fixture (made by executing notebook 15's own cells,
tests/golden/make_nb15_golden.py) against the float64 restatement of tests/nb15_reference.py, the module surface, the
output-size rule, the refusals, the fake datamodule's border rule, the configs and the C ABI's refusals (argument checks
run before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nb15_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT, _rel

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb15_small.npz")


@pytest.mark.parametrize("tag, out_side", [("a", 23), ("b", 23)])
def test_float64_restatement_reproduces_the_golden(tag, out_side):
    """The golden is torch's float32 CPU arithmetic on the notebook's source; the restatement agrees to float32 rounding.
    There is no selection (pool) in this model, so every gradient is held to NORM_TOL."""
    gold = np.load(GOLDEN)
    batch, init = R.golden_case(gold, tag)
    p = R.params64(init)
    y_hat = R.forward64(p, batch)
    assert tuple(y_hat.shape) == (batch["FORECAST_HORIZON"].shape[0], 1, out_side, out_side)
    assert _rel(y_hat.detach(), gold[f"{tag}/y_hat"]) <= NORM_TOL
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= NORM_TOL * gold[f"{tag}/losses"][0]
    loss.backward()
    for k, v in p.items():
        assert _rel(v.grad, gold[f"{tag}/grad/{k}"]) <= NORM_TOL, (k, _rel(v.grad, gold[f"{tag}/grad/{k}"]))


def test_state_dict_names_shapes_and_parameter_count():
    from predict_pv_yield_amd.models.conv2d.nb15_strided_ae import LitAutoEncoder
    model = LitAutoEncoder()
    gold = np.load(GOLDEN)
    sd = model.state_dict()
    want = {k[len("init/"):]: gold[k].shape for k in gold.files if k.startswith("init/")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in want.items()}
    assert list(sd) == [f"conv.{i}.{w}" for i in R.ENC + R.DEC for w in ("weight", "bias")]
    assert tuple(sd["conv.10.weight"].shape) == (32, 16, 3, 3)       # ConvTranspose2d: [c_in][c_out][3][3]
    assert sum(p.numel() for p in model.parameters()) == 38033
    model.load_state_dict({k: torch.from_numpy(gold[f"init/{k}"]) for k in sd})
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 0.001
    assert LitAutoEncoder(lr=1e-4).configure_optimizers().param_groups[0]["lr"] == 1e-4


def test_output_size_rule_and_refusals():
    from predict_pv_yield_amd.models.conv2d import nb15_strided_ae as M
    sides = {31: 15, 32: 15, 47: 23, 50: 23, 54: 23, 62: 23, 128: 63}
    for s, out in sides.items():
        assert M.output_side(s) == out and M.target_side(s) == out + 1, s
    with pytest.raises(ValueError, match="at least 31"):
        M.output_side(30)
    model = M.LitAutoEncoder()
    batch = {M.HISTORICAL_SAT_IMAGES: torch.zeros(2, 4, 47, 47, dtype=torch.int16),
             M.OPTICAL_FLOW_PREDICTIONS: torch.zeros(2, 47, 47), M.FORECAST_HORIZON: torch.zeros(2),
             M.TARGET_SAT_IMAGE: torch.zeros(2, 23, 23, dtype=torch.int16)}    # the output's own side: [..., :-1, :-1] is 22
    with pytest.raises(ValueError, match=r"TARGET_SAT_IMAGE must be \[B, 24, 24\]"):
        model.training_step(batch, 0)
    M.check_target_side((47, 128), (2, 24, 64))                                 # each side by its own rule
    with pytest.raises(ValueError, match=r"TARGET_SAT_IMAGE must be \[B, 24, 64\]"):
        M.check_target_side((47, 128), (2, 24, 24))
    small = dict(batch, **{M.HISTORICAL_SAT_IMAGES: torch.zeros(2, 4, 30, 30, dtype=torch.int16),
                           M.OPTICAL_FLOW_PREDICTIONS: torch.zeros(2, 30, 30)})
    with pytest.raises(ValueError, match="at least 31"):
        model.training_step(small, 0)
    batch[M.TARGET_SAT_IMAGE] = torch.zeros(2, 24, 24, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.training_step(batch, 0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    # three or five history frames, a depth axis already there, no batch axis: refused before the device is looked at
    z = torch.zeros
    for hist in (z(2, 3, 47, 47), z(2, 5, 47, 47), z(2, 1, 4, 47, 47), z(4, 47, 47)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({**batch, M.HISTORICAL_SAT_IMAGES: hist})


def test_fake_datamodule_refuses_an_odd_border():
    from predict_pv_yield_amd.data import nb15_datamodule as D
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="even border"):
        D.make_fake_nb15_batch(None, 2, 47, rng)          # target 24: a border of 23 pixels cannot be centred
    with pytest.raises(ValueError, match="at least 31"):
        D.make_fake_nb15_batch(None, 2, 30, rng)
    dm = D.Nb15DataModule(batch_size=4)
    assert dm.make_batch is D.make_fake_nb15_batch and dm.image_size_pixels == 128


@pytest.mark.parametrize("name, lr", [("nb15_strided_ae", 1e-3), ("nb14_strided_ae", 1e-4)])
def test_configs_compose(name, lr):
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", [f"model={name}", "datamodule=nb15_fake", "callbacks=none",
                                                              "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb15_strided_ae.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb15_datamodule.Nb15DataModule"
    assert cfg.datamodule.batch_size == 64 and cfg.datamodule.image_size_pixels == 128
    model = H.instantiate(cfg.model)
    dm = H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == 38033 and dm.batch_size == 64
    assert model.configure_optimizers().param_groups[0]["lr"] == lr


def test_entry_points_refuse_bad_arguments_without_launching():
    """Widths beyond the limit, unsupported channel pairs, images too small for four stride-2 convolutions, a short
    workspace, a loss window that leaves the target: a negative status and a message, from pointers that are never
    dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    assert lib.pv_conv2d_s2_counts_fwd_f32(p, 1, p, 0, p, p, p, p, 2, 30, 47, 16, None) == ESIZE and "31 at least" in err()
    assert lib.pv_conv2d_s2_counts_fwd_f32(p, 1, p, 0, p, p, p, p, 2, 129, 129, 16, None) == ESIZE and "beyond 128" in err()
    assert lib.pv_conv2d_s2_counts_fwd_f32(p, 1, p, 0, p, p, p, p, 2, 47, 47, 32, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv2d_s2_counts_fwd_f32(None, 1, p, 0, p, p, p, p, 2, 47, 47, 16, None) == EINVAL
    assert lib.pv_conv2d_s2_counts_bwd_weight_f32(p, 1, p, 0, p, p, p, p, 2, 47, 47, 16, p, 16, None) == EINVAL
    assert "workspace" in err()
    for c_in, c_out in ((6, 32), (32, 16), (16, 16), (16, 1)):
        assert lib.pv_conv2d_s2_fwd_f32(p, p, p, p, 2, c_in, c_out, 36, 36, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv2d_s2_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 36, 36, None) == ESIZE
        assert lib.pv_conv2d_s2_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 36, 36, p, 1 << 30, None) == ESIZE
    assert lib.pv_conv2d_s2_fwd_f32(p, p, p, p, 2, 32, 32, 36, 129, 1, None) == ESIZE and "beyond 128" in err()
    assert lib.pv_conv2d_s2_fwd_f32(p, p, p, p, 2, 32, 32, 2, 36, 1, None) == ESIZE
    assert lib.pv_conv2d_s2_bwd_weight_workspace_bytes(2, 32, 32, 36, 36, None) == EINVAL
    assert lib.pv_conv2d_s2_bwd_weight_workspace_bytes(2, 32, 32, 36, 36, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_s2_bwd_weight_f32(p, p, None, p, p, 2, 32, 32, 36, 36, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    for c_in, c_out in ((16, 32), (16, 16), (32, 1), (6, 16)):
        assert lib.pv_convt2d_s2_fwd_f32(p, p, p, p, 2, c_in, c_out, 10, 10, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_convt2d_s2_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 10, 10, None) == ESIZE
        assert lib.pv_convt2d_s2_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 10, 10, p, 1 << 30, None) == ESIZE
        assert lib.pv_convt2d_s2_bwd_weight_workspace_bytes(2, c_in, c_out, 10, 10, ctypes.byref(need)) == ESIZE
    assert lib.pv_convt2d_s2_fwd_f32(p, p, p, p, 2, 32, 32, 10, 64, 1, None) == ESIZE and "beyond 128" in err()
    assert lib.pv_convt2d_s2_bwd_weight_workspace_bytes(2, 16, 1, 16, 16, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_convt2d_s2_bwd_weight_f32(p, p, None, p, p, 2, 16, 1, 16, 16, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_mse_window_norm_f32(p, p, 1, 2, 23, 23, 23, 24, 0, 2, p, p, p, 8, None) == ESIZE and "window" in err()
    assert lib.pv_mse_window_norm_f32(p, p, 1, 2, 23, 23, 24, 24, 2, 0, p, p, p, 8, None) == ESIZE
    assert lib.pv_mse_window_norm_f32(p, p, 1, 2, 23, 23, 24, 24, 0, 0, p, p, p, 4, None) == EINVAL and "workspace" in err()
    assert lib.pv_mse_window_norm_f32(p, None, 1, 2, 23, 23, 24, 24, 0, 0, p, p, p, 8, None) == EINVAL
