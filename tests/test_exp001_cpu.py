"""CPU: experiments/001's LitAutoEncoder and its Conv2d 144 / MaxPool entry points without a GPU -- argument errors of the
C ABI (checked before any launch), the wrappers' shape checks, the state_dict contract against the golden fixture, the
CPU-tensor error, the configs and the fake batch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from predict_pv_yield_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exp001_small.npz")
EINVAL, ESIZE = -1, -2


def _err():
    return _lib.get_lib().pv_last_error()


def test_forward_entry_point_argument_errors_without_gpu():
    lib = _lib.get_lib()
    p = ctypes.byref(ctypes.c_float(0))
    # first layer: sat, x_coords, y_coords, w, bias, y, codes, b, t_total, n_frames, h, w, c_out
    sat = lib.pv_conv2d144_sat_pool_fwd_f32
    assert sat(None, p, p, p, p, p, p, 2, 19, 7, 128, 128, 144, None) == EINVAL
    assert b"null pointer" in _err()
    assert sat(p, p, p, p, p, p, None, 2, 19, 7, 128, 128, 144, None) == EINVAL
    assert sat(p, p, p, p, p, p, p, 2, 19, 20, 128, 128, 144, None) == EINVAL
    assert b"beyond the 19 frames" in _err()
    assert sat(p, p, p, p, p, p, p, 2, 40, 28, 128, 128, 144, None) == ESIZE
    assert b"unsupported channel count" in _err()
    assert sat(p, p, p, p, p, p, p, 2, 19, 7, 128, 128, 32, None) == ESIZE
    assert b"unsupported channel count" in _err()
    assert sat(p, p, p, p, p, p, p, 2, 19, 7, 2, 128, 144, None) == ESIZE
    assert b"smaller than the 3x3 kernel" in _err()
    assert sat(p, p, p, p, p, p, p, 2, 19, 7, 4, 128, 144, None) == ESIZE
    assert b"no whole 3x3 pool window" in _err()
    assert sat(p, p, p, p, p, p, p, 0, 19, 7, 128, 128, 144, None) == EINVAL
    assert sat(p, p, p, p, p, p, p, 8192, 19, 7, 128, 128, 144, None) == ESIZE
    assert b"2^31" in _err()
    # conv2: x, w, bias, y, codes, n, c_in, c_out, h, w
    pool = lib.pv_conv2d144_pool_fwd_f32
    assert pool(p, p, p, p, None, 2, 144, 144, 42, 42, None) == EINVAL
    assert pool(p, p, p, p, p, 2, 32, 144, 42, 42, None) == ESIZE
    assert b"unsupported channel counts" in _err()
    assert pool(p, p, p, p, p, 2, 144, 4, 42, 42, None) == ESIZE
    assert pool(p, p, p, p, p, 2, 144, 144, 42, 4, None) == ESIZE
    assert pool(p, p, p, p, p, 1 << 20, 144, 144, 42, 42, None) == ESIZE
    assert b"2^31" in _err()
    # conv3: x, w, bias, y, n, c_in, c_out, h, w, relu
    fwd = lib.pv_conv2d144_fwd_f32
    assert fwd(None, p, p, p, 2, 144, 144, 13, 13, 1, None) == EINVAL
    assert fwd(p, p, p, p, 2, 17, 144, 13, 13, 1, None) == ESIZE
    assert fwd(p, p, p, p, 2, 144, 144, 2, 13, 1, None) == ESIZE
    assert b"smaller than the 3x3 kernel" in _err()


def test_backward_entry_point_argument_errors_without_gpu():
    lib = _lib.get_lib()
    p = ctypes.byref(ctypes.c_float(0))
    nbytes = ctypes.c_size_t(0)
    # data gradients: dy, dy_gate / codes, w, dx, x_gate, n, c_in, c_out, h, w
    assert lib.pv_conv2d144_bwd_data_f32(p, None, None, p, None, 2, 144, 144, 13, 13, None) == EINVAL
    assert b"null pointer" in _err()
    assert lib.pv_conv2d144_bwd_data_f32(p, None, p, p, None, 2, 144, 12, 13, 13, None) == ESIZE
    assert lib.pv_conv2d144_pool_bwd_data_f32(p, None, p, p, None, 2, 144, 144, 42, 42, None) == EINVAL
    assert b"null pointer" in _err()
    assert lib.pv_conv2d144_pool_bwd_data_f32(p, p, p, p, None, 2, 144, 144, 4, 42, None) == ESIZE
    assert lib.pv_conv2d144_pool_bwd_data_f32(p, p, p, p, None, 2, 100, 144, 42, 42, None) == ESIZE
    # workspace queries
    ws = lib.pv_conv2d144_bwd_weight_workspace_bytes
    for args in ((32, 144, 144, 42, 42, 1), (32, 12, 144, 128, 128, 1), (32, 144, 144, 13, 13, 0)):
        assert ws(*args, ctypes.byref(nbytes)) == 0 and nbytes.value > 0, args
        assert nbytes.value <= 64 << 20, (args, nbytes.value)      # fixed slabs, not one per tile
    assert ws(32, 144, 144, 42, 42, 1, None) == EINVAL
    assert ws(32, 144, 32, 42, 42, 1, ctypes.byref(nbytes)) == ESIZE
    assert ws(32, 64, 144, 42, 42, 1, ctypes.byref(nbytes)) == ESIZE
    assert ws(32, 144, 144, 4, 4, 1, ctypes.byref(nbytes)) == ESIZE
    # weight gradients: a call with too little workspace, null pointers
    assert lib.pv_conv2d144_bwd_weight_f32(p, p, None, p, p, 32, 144, 144, 13, 13, p, 4, None) == EINVAL
    assert b"workspace too small" in _err()
    assert lib.pv_conv2d144_bwd_weight_f32(p, None, None, p, p, 32, 144, 144, 13, 13, p, 1 << 30, None) == EINVAL
    assert lib.pv_conv2d144_pool_bwd_weight_f32(p, p, p, p, p, 32, 144, 144, 42, 42, p, 4, None) == EINVAL
    assert b"workspace too small" in _err()
    assert lib.pv_conv2d144_pool_bwd_weight_f32(p, p, None, p, p, 32, 144, 144, 42, 42, p, 1 << 30, None) == EINVAL
    assert lib.pv_conv2d144_sat_pool_bwd_weight_f32(p, p, p, p, p, p, p, 32, 19, 7, 128, 128, 144, p, 4, None) == EINVAL
    assert b"workspace too small" in _err()
    assert lib.pv_conv2d144_sat_pool_bwd_weight_f32(p, p, p, p, p, p, p, 32, 6, 7, 128, 128, 144, p, 1 << 30,
                                                    None) == EINVAL
    assert b"beyond the 6 frames" in _err()


def test_wrappers_reject_mismatched_shapes_before_any_launch():
    from predict_pv_yield_amd import hip_ops as K
    sat = torch.zeros(2, 19, 16, 16, 1)
    xc, yc = torch.zeros(2, 16), torch.zeros(2, 16)
    w1, b1 = torch.zeros(144, 12, 3, 3), torch.zeros(144)
    with pytest.raises(ValueError, match="sat_data"):
        K.conv2d144_sat_pool_fwd_f32(torch.zeros(2, 19, 16, 16, 3), xc, yc, w1, b1, 7)
    with pytest.raises(ValueError, match="n_frames"):
        K.conv2d144_sat_pool_fwd_f32(sat, xc, yc, w1, b1, 20)
    with pytest.raises(ValueError, match="x_coords"):
        K.conv2d144_sat_pool_fwd_f32(sat, torch.zeros(2, 15), yc, w1, b1, 7)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d144_sat_pool_fwd_f32(sat, xc, yc, torch.zeros(144, 17, 3, 3), b1, 7)
    with pytest.raises(ValueError, match="dy_pooled"):
        K.conv2d144_sat_pool_bwd_weight_f32(sat, xc, yc, torch.zeros(2, 144, 5, 4), torch.zeros(2, 144, 4, 4,
                                                                                                 dtype=torch.uint8), 7)
    x = torch.zeros(2, 144, 14, 14)
    w, b = torch.zeros(144, 144, 3, 3), torch.zeros(144)
    codes = torch.zeros(2, 144, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="x \\[N, 144"):
        K.conv2d144_pool_fwd_f32(torch.zeros(2, 32, 14, 14), w, b)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d144_pool_fwd_f32(x, torch.zeros(144, 144, 5, 5), b)
    with pytest.raises(ValueError, match="bias"):
        K.conv2d144_fwd_f32(x, w, torch.zeros(32))
    with pytest.raises(ValueError, match="at least 5 x 5"):
        K.conv2d144_pool_fwd_f32(torch.zeros(2, 144, 4, 14), w, b)
    with pytest.raises(ValueError, match="dy_pooled / codes"):
        K.conv2d144_pool_bwd_data_f32(torch.zeros(2, 144, 4, 5), codes, w, None, tuple(x.shape))
    with pytest.raises(ValueError, match="x_gate"):
        K.conv2d144_pool_bwd_data_f32(torch.zeros(2, 144, 4, 4), codes, w, torch.zeros(2, 144, 14, 13), tuple(x.shape))
    with pytest.raises(ValueError, match="dy_pooled / codes"):
        K.conv2d144_pool_bwd_weight_f32(x, torch.zeros(2, 144, 4, 4), codes[:, :, :3], tuple(w.shape))
    with pytest.raises(ValueError, match="dy / dy_gate"):
        K.conv2d144_bwd_data_f32(torch.zeros(2, 144, 12, 11), None, w, None, tuple(x.shape))
    with pytest.raises(ValueError, match="dy / dy_gate"):
        K.conv2d144_bwd_weight_f32(x, torch.zeros(2, 144, 12, 12), torch.zeros(2, 144, 12, 13), tuple(w.shape))


def test_state_dict_matches_the_reference_names_and_shapes():
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    gold = np.load(GOLDEN)
    sd = LitAutoEncoder().state_dict()
    assert sorted(sd) == list(gold["param_names"])
    for k, v in sd.items():
        if f"grad/{k}" in gold.files:
            assert tuple(gold[f"grad/{k}"].shape) == tuple(v.shape), k
        else:
            assert f"grad/{k}/sample" in gold.files and v.numel() > 20000, k
    assert tuple(sd["sat_conv1.weight"].shape) == (144, 12, 3, 3)
    assert tuple(sd["fc1.weight"].shape) == (256, 17424) and tuple(sd["fc2.weight"].shape) == (128, 1115)
    assert tuple(sd["fc5.weight"].shape) == (12, 128)
    assert tuple(sd["pv_system_id_embedding.weight"].shape) == (940, 16)
    assert tuple(LitAutoEncoder(n_pv_systems=10).state_dict()["pv_system_id_embedding.weight"].shape) == (10, 16)
    assert tuple(gold["y_hat"].shape) == (2, 12)


def test_cpu_tensors_raise_a_clear_error():
    from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    batch = make_fake_exp001_batch(2, 128, torch.Generator().manual_seed(0))
    with pytest.raises(RuntimeError, match="MI355X only"):
        LitAutoEncoder()(batch)


def test_fake_batch_keys_and_shapes():
    from predict_pv_yield_amd.data.exp001_datamodule import Exp001DataModule, make_fake_exp001_batch
    batch = make_fake_exp001_batch(3, 128, torch.Generator().manual_seed(0))
    want = {"sat_data": (3, 19, 128, 128, 1), "sat_x_coords": (3, 128), "sat_y_coords": (3, 128), "nwp": (3, 10, 19, 2, 2),
            "hour_of_day_sin": (3, 19), "hour_of_day_cos": (3, 19), "day_of_year_sin": (3, 19), "day_of_year_cos": (3, 19),
            "pv_yield": (3, 19), "pv_system_row_number": (3,)}
    assert {k: tuple(v.shape) for k, v in batch.items()} == want
    assert batch["pv_system_row_number"].dtype == torch.int64 and int(batch["pv_system_row_number"].max()) < 940
    again = make_fake_exp001_batch(3, 128, torch.Generator().manual_seed(0))
    assert all(torch.equal(batch[k], again[k]) for k in batch)
    dm = Exp001DataModule(batch_size=2, n_train_data=3, n_val_data=1)
    items = list(dm.train_dataloader())
    assert len(items) == 3 and tuple(items[0]["sat_data"].shape) == (2, 19, 128, 128, 1)
    assert len(list(dm.val_dataloader())) == 1


def test_configs_compose():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=exp001_cnn", "datamodule=exp001_fake",
                                                              "callbacks=none"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.exp001.LitAutoEncoder"
    assert cfg.model.history_len == 6 and cfg.model.forecast_len == 12
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.exp001_datamodule.Exp001DataModule"
    assert cfg.datamodule.batch_size == 32 and cfg.datamodule.image_size_pixels == 128
    model = H.instantiate(cfg.model)
    dm = H.instantiate(cfg.datamodule)
    assert model.forecast_len == 12 and dm.batch_size == 32
