"""GPU: the padded 64 / 128-channel Conv2d frame predictor of notebooks/10_just_conv.ipynb (csrc/conv2d_wide_f32.hip,
conv2d_functional, models/conv2d/nb10_just_conv.py) against float64 on the CPU.

The three passes of conv2d_wide at both paddings and of conv2d_head_s2, and the stripe first layer, are checked by the records
and the one checker of tests/conv_family_checks.py, which hold the shapes and tolerances.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch

import conv_family_checks as C
from conv2d_f32_helpers import _ops

pytestmark = pytest.mark.gpu


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of({"conv2d_wide_pad0": 0, "conv2d_wide_pad2": 2}, ids="{tag}-{shape}-{c_in}")
def test_wide_conv_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@pytest.mark.parametrize("n_hist", C.N_HIST)
@C.twin_shapes("conv2d_wide_stripe")
def test_stripe_layer_against_float64(device, twin, shape, n_hist):
    C.check_stripe_layer(_ops(), device, twin, n_hist, shape)


@C.cases_of("conv2d_head_s2", ids="{shape}-{c_in}")
def test_head_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


def test_refusals_raise_before_any_launch(device):
    import ctypes
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(ValueError, match="C_in, C_out"):                         # unsupported channel pair
        K.conv2d_wide_fwd_f32(z(1, 32, 8, 8), z(128, 32, 3, 3), z(128))
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.conv2d_wide_bwd_data_f32(z(1, 64, 6, 6), None, z(64, 128, 3, 3), None, (1, 128, 8, 8))
    with pytest.raises(ValueError, match="padding"):                             # padding 1
        K.conv2d_wide_fwd_f32(z(1, 64, 8, 8), z(128, 64, 3, 3), z(128), padding=1)
    with pytest.raises(ValueError, match="128"):                                 # 129 columns
        K.conv2d_wide_fwd_f32(z(1, 64, 8, 129), z(128, 64, 3, 3), z(128))
    with pytest.raises(ValueError, match="stripe_start"):
        K.conv2d_wide_stripe_fwd_f32(z(2, 4, 8, 8), z(2), z(64, 5, 3, 3), z(64), 5)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d_head_s2_fwd_f32(z(1, 32, 8, 8), z(2, 32, 3, 3), z(2))
    with pytest.raises(RuntimeError, match="status -1"):                         # the head takes no dy_gate
        K.conv2d_head_s2_bwd_data_f32(z(1, 1, 5, 5), z(1, 1, 5, 5), z(1, 32, 3, 3), None, (1, 32, 8, 8))
    # the ABI itself, from device pointers: the error code, nothing launched
    lib = _lib.get_lib()
    x, wt, y = z(1, 64, 8, 8), z(128, 64, 3, 3), torch.full((1, 128, 6, 6), 7.0, device=device)
    assert lib.pv_conv2d_wide_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 32, 128, 8, 8, 0, 0, None) == -2
    assert lib.pv_conv2d_wide_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 8, 8, 1, 0, None) == -2
    assert lib.pv_conv2d_wide_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 8, 129, 0, 0, None) == -2
    assert lib.pv_conv2d_wide_fwd_f32(ptr(x), None, None, ptr(y), 1, 64, 128, 8, 8, 0, 0, None) == -1
    torch.cuda.synchronize()
    assert (y == 7.0).all(), "a refused call wrote its output"
    need = ctypes.c_size_t(0)
    assert lib.pv_conv2d_wide_bwd_weight_workspace_bytes(1, 64, 128, 8, 8, 0, ctypes.byref(need)) == 0 and need.value > 0
    dw, db, ws = z(128, 64, 3, 3), z(128), z(1 << 20)
    assert lib.pv_conv2d_wide_bwd_weight_f32(ptr(x), ptr(y), None, ptr(dw), ptr(db), 1, 64, 128, 8, 8, 0, ptr(ws),
                                             need.value - 1, None) == -1
    assert "workspace" in lib.pv_last_error().decode()
