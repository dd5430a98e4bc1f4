"""GPU: the stride-2 64 / 128-channel Conv2d / ConvTranspose2d autoencoder of notebooks/09_horizon_represented_as_a_stripe.ipynb
(csrc/conv2d_wide_s2_f32.hip, conv2d_functional, models/conv2d/nb09_stripe_ae.py) against float64 on the CPU.

The three passes of conv2d_wide_s2, convt2d_wide_s2 and convt2d_head and the stripe first layer are checked by the records
and the one checker of tests/conv_family_checks.py, which hold the shapes and tolerances.  The model-level checks (golden fixture, full size,
determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's, run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
from conv2d_f32_helpers import NORM_TOL, _ops, _rel
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu

LOSS_SHAPES = [((2, 9, 25), (2, 8, 24)), ((1, 65, 65), (1, 64, 64))]


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of("conv2d_wide_s2", ids="{shape}-{c_in}")
def test_conv_s2_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.cases_of(("conv2d_wide_s2_tiles128", "conv2d_wide_s2_tiles64"), ids="{c_in}-{shape}")
def test_conv_s2_larger_tiles_against_float64(device, fam, c_in, c_out, shape):
    """The tiles the planners take only on a full grid."""
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.cases_of("convt2d_wide_s2", ids="{shape}")
def test_convt_s2_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.cases_of("convt2d_wide_s2_tiles", ids="{shape}")
def test_convt_s2_larger_tiles_against_float64(device, fam, c_in, c_out, shape):
    """A full grid of tiny planes: the scatter at 128 class positions and the gather at 256 positions per block."""
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@pytest.mark.parametrize("n_hist", C.N_HIST)
@C.twin_shapes("conv2d_wide_s2_stripe")
def test_stripe_layer_against_float64(device, twin, shape, n_hist):
    C.check_stripe_layer(_ops(), device, twin, n_hist, shape)


@C.cases_of("convt2d_head", ids="{shape}-{c_in}")
def test_head_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- 1. the loss over a window of the prediction -----------------------------------------------------------------------
@pytest.mark.parametrize("y_shape, t_shape", LOSS_SHAPES)
def test_mse_pred_window_against_float64(device, y_shape, t_shape):
    K = _ops()
    g = _g(700 + y_shape[2])
    y_hat, target = _randn(g, *y_shape), _randn(g, *t_shape)
    y64 = y_hat.double().requires_grad_(True)
    ref = F.mse_loss(y64[:, :-1, :-1], target.double())
    ref.backward()
    loss, grad = K.mse_pred_window_f32(y_hat.to(device), target.to(device), 0, 0)
    assert tuple(loss.shape) == (1,) and tuple(grad.shape) == tuple(y_shape)
    assert abs(loss.item() - ref.item()) <= 1e-5 * ref.item(), (loss.item(), ref.item())
    assert _rel(grad[:, :-1, :-1], y64.grad[:, :-1, :-1]) <= NORM_TOL
    assert (grad[:, -1, :] == 0).all() and (grad[:, :, -1] == 0).all(), "the gradient outside the window is not exactly 0"
    loss2, none = K.mse_pred_window_f32(y_hat.to(device), target.to(device), 0, 0, need_grad=False)
    assert none is None and torch.equal(loss, loss2)
    # a window that starts inside the prediction: the first row and column are outside
    loss3, grad3 = K.mse_pred_window_f32(y_hat.to(device), target.to(device), 1, 1)
    ref3 = F.mse_loss(y_hat.double()[:, 1:, 1:], target.double()).item()
    assert abs(loss3.item() - ref3) <= 1e-5 * ref3
    assert (grad3[:, 0, :] == 0).all() and (grad3[:, :, 0] == 0).all()
    # through autograd: the gradient scaled by the root gradient
    from predict_pv_yield_amd.conv2d_functional import mse_pred_window
    yd = y_hat.to(device).requires_grad_(True)
    (3.0 * mse_pred_window(yd, target.to(device))).backward()
    assert _rel(yd.grad, 3.0 * y64.grad) <= NORM_TOL


# ---- 2. refusals through the Python surface and the raw ABI ------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    import ctypes
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(ValueError, match="C_in, C_out"):                         # unsupported channel pair
        K.conv2d_wide_s2_fwd_f32(z(1, 32, 8, 8), z(128, 32, 3, 3), z(128))
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.conv2d_wide_s2_bwd_data_f32(z(1, 64, 3, 3), None, z(64, 128, 3, 3), None, (1, 128, 8, 8))
    with pytest.raises(ValueError, match="128"):                                 # 129 columns
        K.conv2d_wide_s2_fwd_f32(z(1, 64, 8, 129), z(128, 64, 3, 3), z(128))
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.convt2d_wide_s2_fwd_f32(z(1, 64, 4, 4), z(64, 128, 3, 3), z(128))
    with pytest.raises(ValueError, match="128"):                                 # output 129 columns wide
        K.convt2d_wide_s2_fwd_f32(z(1, 128, 4, 64), z(128, 128, 3, 3), z(128))
    with pytest.raises(ValueError, match="stripe_start"):
        K.conv2d_wide_s2_stripe_fwd_f32(z(2, 4, 8, 8), z(2), z(64, 5, 3, 3), z(64), 5)
    with pytest.raises(ValueError, match="weight"):
        K.convt2d_head_fwd_f32(z(1, 32, 8, 8), z(32, 2, 3, 3), z(2))
    with pytest.raises(RuntimeError, match="status -1"):                         # the head takes no dy_gate
        K.convt2d_head_bwd_data_f32(z(1, 1, 10, 10), z(1, 1, 10, 10), z(32, 1, 3, 3), None, (1, 32, 8, 8))
    with pytest.raises(RuntimeError, match="status -2"):                         # a window off y_hat
        K.mse_pred_window_f32(z(1, 9, 9), z(1, 8, 8), 2, 0)
    # the ABI itself, from device pointers: the error code, nothing launched
    lib = _lib.get_lib()
    x, wt, y = z(1, 64, 8, 8), z(128, 64, 3, 3), torch.full((1, 128, 3, 3), 7.0, device=device)
    assert lib.pv_conv2d_wide_s2_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 32, 128, 8, 8, 0, None) == -2
    assert lib.pv_conv2d_wide_s2_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 8, 129, 0, None) == -2
    assert lib.pv_conv2d_wide_s2_fwd_f32(ptr(x), None, None, ptr(y), 1, 64, 128, 8, 8, 0, None) == -1
    assert lib.pv_convt2d_wide_s2_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 1, 1, 0, None) == -2
    assert lib.pv_convt2d_head_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 64, 2, 1, 1, 0, None) == -2
    assert lib.pv_convt2d_head_bwd_data_f32(ptr(x), ptr(x), ptr(wt), ptr(y), None, 1, 128, 1, 1, 1, None) == -1
    assert lib.pv_mse_pred_window_f32(ptr(x), ptr(x), 1, 3, 3, 3, 3, 1, 0, ptr(x), ptr(y), ptr(wt), 4, None) == -2
    torch.cuda.synchronize()
    assert (y == 7.0).all(), "a refused call wrote its output"
    need = ctypes.c_size_t(0)
    assert lib.pv_conv2d_wide_s2_bwd_weight_workspace_bytes(1, 64, 128, 8, 8, ctypes.byref(need)) == 0 and need.value > 0
    dw, db, ws = torch.full((128, 64, 3, 3), 7.0, device=device), z(128), z(1 << 20)
    assert lib.pv_conv2d_wide_s2_bwd_weight_f32(ptr(x), ptr(y), None, ptr(dw), ptr(db), 1, 64, 128, 8, 8, ptr(ws),
                                                need.value - 1, None) == -1
    assert "workspace" in lib.pv_last_error().decode()
    torch.cuda.synchronize()
    assert (dw == 7.0).all(), "a refused call wrote its output"
