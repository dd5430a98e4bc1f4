"""CPU: experiments/002's LitModel and its Conv2d entry points without a GPU -- argument errors of the C ABI (checked before
any launch), the state_dict contract against the golden fixture, the CPU-tensor error and the configs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from predict_pv_yield_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exp002_small.npz")


def test_conv2d_argument_errors_without_gpu():
    lib = _lib.get_lib()
    one = ctypes.c_float(0)
    p = ctypes.byref(one)
    nbytes = ctypes.c_size_t(0)
    assert lib.pv_conv2d_fwd_f32(None, p, p, p, 8, 32, 32, 30, 30, 1, None) == -1
    assert b"null pointer" in lib.pv_last_error()
    assert lib.pv_conv2d_fwd_f32(p, p, p, p, 8, 32, 32, 2, 30, 1, None) == -2
    assert b"smaller than the 3x3 kernel" in lib.pv_last_error()
    assert lib.pv_conv2d_fwd_f32(p, p, p, p, 8, 16, 32, 30, 30, 1, None) == -2
    assert b"unsupported channel counts" in lib.pv_last_error()
    assert lib.pv_conv2d_fwd_f32(p, p, p, p, 8, 32, 8, 30, 30, 1, None) == -2
    assert lib.pv_conv2d_fwd_f32(p, p, p, p, 0, 32, 32, 30, 30, 1, None) == -1
    assert lib.pv_conv2d_bwd_data_f32(p, None, None, p, None, 8, 32, 4, 28, 28, None) == -1
    assert b"null pointer" in lib.pv_last_error()
    assert lib.pv_conv2d_bwd_data_f32(p, None, p, p, None, 8, 32, 4, 28, 1, None) == -2
    assert lib.pv_conv2d_coords_fwd_f32(p, None, p, p, p, p, 38, 19, 32, 32, 32, None) == -1
    assert lib.pv_conv2d_coords_fwd_f32(p, p, p, p, p, p, 38, 19, 32, 32, 16, None) == -2
    assert b"unsupported channel count" in lib.pv_last_error()
    assert lib.pv_conv2d_coords_fwd_f32(p, p, p, p, p, p, 37, 19, 32, 32, 32, None) == -1
    assert b"multiple of t_per_example" in lib.pv_last_error()
    assert lib.pv_conv2d_coords_fwd_f32(p, p, p, p, p, p, 38, 19, 32, 200, 32, None) == -2
    # workspace: a size query, then a call with too little of it
    assert lib.pv_conv2d_bwd_weight_workspace_bytes(608, 32, 32, 30, 30, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    assert lib.pv_conv2d_bwd_weight_workspace_bytes(608, 17, 32, 32, 32, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    assert lib.pv_conv2d_bwd_weight_workspace_bytes(608, 17, 4, 32, 32, ctypes.byref(nbytes)) == -2
    assert lib.pv_conv2d_bwd_weight_workspace_bytes(608, 32, 32, 30, 30, None) == -1
    assert lib.pv_conv2d_bwd_weight_f32(p, p, None, p, p, 608, 32, 32, 30, 30, p, 4, None) == -1
    assert b"workspace too small" in lib.pv_last_error()
    assert lib.pv_conv2d_bwd_weight_f32(p, None, None, p, p, 608, 32, 32, 30, 30, p, 1 << 30, None) == -1
    assert lib.pv_conv2d_coords_bwd_weight_f32(p, p, p, p, p, p, 38, 19, 32, 32, 32, p, 4, None) == -1
    assert b"workspace too small" in lib.pv_last_error()


def test_state_dict_matches_the_reference_names_and_shapes():
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    gold = np.load(GOLDEN)
    sd = LitModel().state_dict()
    assert sorted(sd) == list(gold["param_names"])
    for k, v in sd.items():
        key = f"grad/{k}" if f"grad/{k}" in gold.files else None
        if key is not None:
            assert tuple(gold[key].shape) == tuple(v.shape), k
    assert tuple(sd["fc1.weight"].shape) == (256, 2704) and tuple(sd["sat_conv1.weight"].shape) == (32, 17, 3, 3)
    assert tuple(sd["pv_system_id_embedding.weight"].shape) == (940, 16)


def test_cpu_tensors_raise_a_clear_error():
    from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    batch = make_fake_exp002_batch(2, 32, torch.Generator().manual_seed(0))
    assert tuple(batch["sat_data"].shape) == (2, 19, 32, 32, 12) and tuple(batch["sat_x_coords"].shape) == (2, 32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        LitModel()(batch)


def test_configs_compose():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=exp002_cnn_rnn", "datamodule=exp002_fake",
                                                              "callbacks=none"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.exp002.LitModel"
    assert cfg.model.history_len == 6 and cfg.model.forecast_len == 12
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.exp002_datamodule.Exp002DataModule"
    assert cfg.datamodule.batch_size == 32 and cfg.datamodule.image_size_pixels == 32
    model = H.instantiate(cfg.model)
    dm = H.instantiate(cfg.datamodule)
    assert model.forecast_len == 12 and dm.batch_size == 32


def test_conv3_weight_gradient_takes_the_general_kernels_workspace():
    """32 -> 4 weight gradients run the general Conv3d f32 kernel as a 1x3x3 conv: the workspace query is that kernel's."""
    lib = _lib.get_lib()
    got, want = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.pv_conv2d_bwd_weight_workspace_bytes(608, 32, 4, 28, 28, ctypes.byref(got)) == 0
    g = _lib.Conv3dGeom(608, 32, 4, 1, 28, 28, 1, 3, 3, 1, 1, 1, 0, 0, 0)
    assert lib.pv_conv3d_general_bwd_weight_workspace_bytes(ctypes.byref(g), ctypes.byref(want)) == 0
    assert got.value == want.value > 0


def test_wrappers_reject_mismatched_shapes_before_any_launch():
    from predict_pv_yield_amd import hip_ops as K
    sat = torch.zeros(6, 8, 8, 12)
    w1, b1 = torch.zeros(32, 17, 3, 3), torch.zeros(32)
    with pytest.raises(ValueError, match="x_coords"):
        K.conv2d_coords_fwd_f32(sat, torch.zeros(2, 7), torch.zeros(2, 8), w1, b1, 3)
    with pytest.raises(ValueError, match="x_coords"):
        K.conv2d_coords_fwd_f32(sat, torch.zeros(2, 8), torch.zeros(2, 8), w1, b1, 2)   # t does not match the rows
    with pytest.raises(ValueError, match="multiple of t_per_example"):
        K.conv2d_coords_fwd_f32(sat, torch.zeros(2, 8), torch.zeros(2, 8), w1, b1, 4)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d_coords_fwd_f32(sat, torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(32, 12, 3, 3), b1, 3)
    with pytest.raises(ValueError, match="dy"):
        K.conv2d_coords_bwd_weight_f32(sat, torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(6, 32, 5, 6), 3, (32, 17, 3, 3))
    x = torch.zeros(2, 32, 10, 10)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d_fwd_f32(x, torch.zeros(32, 16, 3, 3), None)
    with pytest.raises(ValueError, match="bias"):
        K.conv2d_fwd_f32(x, torch.zeros(4, 32, 3, 3), torch.zeros(32))
    with pytest.raises(ValueError, match="dy"):
        K.conv2d_bwd_data_f32(torch.zeros(2, 4, 8, 7), None, torch.zeros(4, 32, 3, 3), None, (2, 32, 10, 10))
    with pytest.raises(ValueError, match="x_gate"):
        K.conv2d_bwd_data_f32(torch.zeros(2, 4, 8, 8), None, torch.zeros(4, 32, 3, 3), torch.zeros(2, 32, 10, 9),
                              (2, 32, 10, 10))
    with pytest.raises(ValueError, match="dy"):
        K.conv2d_bwd_weight_f32(x, torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 9), (4, 32, 3, 3))
