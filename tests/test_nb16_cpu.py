"""CPU: notebook 16's LitAutoEncoder -- the golden fixture (made by executing the notebook's own cells,
tests/golden/make_nb16_golden.py) against the float64 restatement of tests/nb16_reference.py, the module surface, the
output-size rule, the configs, the loader keyword and the C ABI's refusals (argument checks run before any launch)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import nb16_reference as R
from conv2d_f32_helpers import ROOT, _rel

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb16_small.npz")


@pytest.mark.parametrize("tag, out_side", [("a", 18), ("b", 17)])
def test_float64_restatement_reproduces_the_golden(tag, out_side):
    """The golden is torch's float32 CPU arithmetic on the notebook's source; the restatement must agree to float32
    rounding: y_hat and loss to 1e-5, decoder gradients to 1e-4; encoder gradients pass through the pool, where a
    near-tie may be picked differently in float64 (ROUTED_TOL)."""
    gold = np.load(GOLDEN)
    batch, init = R.golden_case(gold, tag)
    p = R.params64(init)
    y_hat = R.forward64(p, batch)
    assert tuple(y_hat.shape) == (batch["FORECAST_HORIZON"].shape[0], 1, out_side, out_side)
    assert _rel(y_hat.detach(), gold[f"{tag}/y_hat"]) <= 1e-5
    loss = R.loss64(y_hat, batch["TARGET_SAT_IMAGE"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    for k, v in p.items():
        tol = R.ROUTED_TOL if k.startswith("encoder") else 1e-4
        assert _rel(v.grad, gold[f"{tag}/grad/{k}"]) <= tol, (k, _rel(v.grad, gold[f"{tag}/grad/{k}"]))


def test_state_dict_names_shapes_and_parameter_count():
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder
    model = LitAutoEncoder()
    gold = np.load(GOLDEN)
    sd = model.state_dict()
    want = {k[len("init/"):]: gold[k].shape for k in gold.files if k.startswith("init/")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in want.items()}
    assert list(sd) == [f"{n}.{w}" for n in R.ENC + R.DEC for w in ("weight", "bias")]
    assert tuple(sd["decoder_conv2.weight"].shape) == (32, 16, 3, 3)       # ConvTranspose2d: [c_in][c_out][3][3]
    assert sum(p.numel() for p in model.parameters()) == 40353
    assert isinstance(model.maxpool, torch.nn.MaxPool2d) and isinstance(model.maxunpool, torch.nn.MaxUnpool2d)
    assert not list(model.maxpool.parameters()) and not list(model.maxunpool.parameters())
    model.load_state_dict({k: torch.from_numpy(gold[f"init/{k}"]) for k in sd})
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 0.001


def test_output_size_rule_and_refusals():
    from predict_pv_yield_amd.models.conv2d import nb16_maxpool as M
    assert M.output_side(128) == 48 and M.target_side(128) == 64
    assert M.output_side(38) == 18 and M.target_side(38) == 34
    assert M.output_side(36) == 17 and M.target_side(36) == 33
    assert M.output_side(11) == 9
    with pytest.raises(ValueError, match="at least 11"):
        M.output_side(10)
    model = M.LitAutoEncoder()
    batch = {M.HISTORICAL_SAT_IMAGES: torch.zeros(2, 4, 35, 35, dtype=torch.int16),
             M.OPTICAL_FLOW_PREDICTIONS: torch.zeros(2, 35, 35), M.FORECAST_HORIZON: torch.zeros(2),
             M.TARGET_SAT_IMAGE: torch.zeros(2, 17, 17, dtype=torch.int16)}    # S // 2: torch would broadcast a 1 x 1 crop
    with pytest.raises(ValueError, match=r"TARGET_SAT_IMAGE must be \[B, 33, 33\]"):
        model.training_step(batch, 0)
    M.check_target_side((38, 36), (2, 34, 33))                                  # each side by its own rule
    with pytest.raises(ValueError, match=r"TARGET_SAT_IMAGE must be \[B, 34, 33\]"):
        M.check_target_side((38, 36), (2, 34, 34))
    batch[M.TARGET_SAT_IMAGE] = torch.zeros(2, 33, 33, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.training_step(batch, 0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    # three or five history frames, a depth axis already there, no batch axis: refused before the device is looked at
    z = torch.zeros
    for hist in (z(2, 3, 35, 35), z(2, 5, 35, 35), z(2, 1, 4, 35, 35), z(4, 35, 35)):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({**batch, M.HISTORICAL_SAT_IMAGES: hist})


def test_configs_compose():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb16_maxpool_ae", "datamodule=nb16_fake",
                                                              "callbacks=none", "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb16_maxpool.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb16_datamodule.Nb16DataModule"
    assert cfg.datamodule.batch_size == 64 and cfg.datamodule.image_size_pixels == 128
    model = H.instantiate(cfg.model)
    dm = H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == 40353 and dm.batch_size == 64


def test_load_super_batch_keyword_and_unchanged_default():
    from predict_pv_yield_amd.data import flow_examples as fe
    sig = inspect.signature(fe.load_super_batch)
    assert list(sig.parameters) == ["raw_counts", "include_optical_flow", "normalise"]
    assert sig.parameters["normalise"].default is True and sig.parameters["include_optical_flow"].default is True
    for kw in ({}, {"normalise": False}, {"normalise": True}):      # accepted; the CPU refusal is the same either way
        with pytest.raises(RuntimeError, match="MI355X"):
            fe.load_super_batch(torch.zeros(3, 8, 8, dtype=torch.int16), **kw)


def test_entry_points_refuse_bad_arguments_without_launching():
    """Widths beyond 128, unsupported channel pairs, images too small for one pool window after four convolutions, a
    target side that does not match: a negative status and a message, from pointers that are never dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    assert lib.pv_conv2d_ae_counts_fwd_f32(p, 1, p, 0, p, p, p, p, 2, 10, 10, 16, None) == ESIZE and "pool window" in err()
    assert lib.pv_conv2d_ae_counts_fwd_f32(p, 1, p, 0, p, p, p, p, 2, 129, 129, 16, None) == ESIZE and "beyond 128" in err()
    assert lib.pv_conv2d_ae_counts_fwd_f32(p, 1, p, 0, p, p, p, p, 2, 38, 38, 32, None) == ESIZE and "c_out" in err()
    assert lib.pv_conv2d_ae_counts_fwd_f32(None, 1, p, 0, p, p, p, p, 2, 38, 38, 16, None) == EINVAL
    assert lib.pv_conv2d_ae_counts_bwd_weight_f32(p, 1, p, 0, p, p, p, p, 2, 10, 38, 16, p, 16, None) == ESIZE
    assert lib.pv_conv2d_ae_counts_bwd_weight_f32(p, 1, p, 0, p, p, p, p, 2, 38, 38, 16, p, 16, None) == EINVAL
    assert "workspace" in err()
    for c_in, c_out in ((6, 32), (32, 16), (16, 16), (144, 144)):
        assert lib.pv_conv2d_ae_fwd_f32(p, p, p, p, 2, c_in, c_out, 36, 36, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_conv2d_ae_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 36, 36, None) == ESIZE
        assert lib.pv_conv2d_ae_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 36, 36, p, 1 << 30, None) == ESIZE
    assert lib.pv_conv2d_ae_fwd_f32(p, p, p, p, 2, 32, 32, 36, 129, 1, None) == ESIZE and "beyond 128" in err()
    assert lib.pv_conv2d_ae_fwd_f32(p, p, p, p, 2, 32, 32, 2, 36, 1, None) == ESIZE
    assert lib.pv_conv2d_ae_bwd_weight_workspace_bytes(2, 32, 32, 36, 36, 0, None) == EINVAL
    assert lib.pv_conv2d_ae_bwd_weight_workspace_bytes(2, 32, 32, 36, 36, 0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_ae_bwd_weight_workspace_bytes(2, 16, 32, 36, 36, 1, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_ae_pool_fwd_f32(p, p, p, p, p, 2, 16, 32, 36, 36, None, 0, None) == ESIZE
    assert lib.pv_conv2d_ae_pool_fwd_f32(p, p, p, p, p, 2, 32, 32, 4, 36, None, 0, None) == ESIZE and "pool window" in err()
    assert lib.pv_conv2d_ae_pool_fwd_workspace_bytes(2, 32, 32, 36, 36, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.pv_conv2d_ae_pool_fwd_workspace_bytes(4, 32, 32, 128, 128, ctypes.byref(need)) == 0
    assert need.value >= 4 * 32 * 126 * 126 * 4                   # the general route: pre-activations in the workspace
    assert lib.pv_conv2d_ae_pool_fwd_f32(p, p, p, p, p, 4, 32, 32, 128, 128, None, 0, None) == EINVAL and "workspace" in err()
    assert lib.pv_conv2d_ae_pool_fwd_workspace_bytes(2, 16, 32, 36, 36, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_ae_pool_bwd_data_f32(p, p, p, p, None, 2, 32, 32, 36, 4, None) == ESIZE
    assert lib.pv_conv2d_ae_pool_bwd_weight_f32(p, p, p, p, p, 2, 32, 32, 36, 130, p, 1 << 30, None) == ESIZE
    for c_in, c_out in ((16, 32), (32, 1), (1, 16), (6, 16)):
        assert lib.pv_convt2d_ae_fwd_f32(p, p, p, p, 2, c_in, c_out, 10, 10, 1, None) == ESIZE and "channel" in err()
        assert lib.pv_convt2d_ae_bwd_data_f32(p, None, p, p, None, 2, c_in, c_out, 10, 10, None) == ESIZE
        assert lib.pv_convt2d_ae_bwd_weight_f32(p, p, None, p, p, 2, c_in, c_out, 10, 10, p, 1 << 30, None) == ESIZE
        assert lib.pv_convt2d_ae_bwd_weight_workspace_bytes(2, c_in, c_out, 10, 10, ctypes.byref(need)) == ESIZE
    assert lib.pv_convt2d_ae_fwd_f32(p, p, p, p, 2, 32, 32, 10, 127, 1, None) == ESIZE and "beyond 128" in err()
    assert lib.pv_convt2d_ae_bwd_weight_workspace_bytes(2, 16, 1, 16, 16, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_mse_crop_norm_f32(p, p, 1, 2, 18, 18, 33, 34, p, p, p, 8, None) == ESIZE and "target side" in err()
    assert lib.pv_mse_crop_norm_f32(p, p, 1, 2, 18, 18, 19, 19, p, p, p, 8, None) == ESIZE
    assert lib.pv_mse_crop_norm_f32(p, p, 1, 2, 18, 18, 34, 34, p, p, p, 4, None) == EINVAL and "workspace" in err()
    assert lib.pv_mse_crop_norm_f32(p, None, 1, 2, 18, 18, 34, 34, p, p, p, 8, None) == EINVAL
