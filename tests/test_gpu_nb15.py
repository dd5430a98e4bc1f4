"""GPU: the stride-2 Conv2d / ConvTranspose2d autoencoder of notebooks 14 / 15 (csrc/conv2d_s2_f32.hip, conv2d_functional,
models/conv2d/nb15_strided_ae.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  The model has no pool, so the golden fixture
(torch float32 on the CPU) holds every gradient to NORM_TOL.

The three passes of conv2d_s2 and convt2d_s2 and the counts first layer are checked below by the records
and the one checker of tests/conv_family_checks.py.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch

import nb15_reference as R
import conv_family_checks as C
from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of("conv2d_s2", ids="{shape}-{c_in}")
def test_conv_s2_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.twin_shapes("conv2d_s2_counts")
def test_counts_layer_against_float64(device, twin, shape):
    C.check_counts_layer(_ops(), device, twin, shape)


def test_counts_layer_int16_and_f32_inputs_give_identical_bits(device):
    C.check_counts_layer_input_dtypes(_ops(), device, C.TWINS["conv2d_s2_counts"])


@C.cases_of("convt2d_s2", ids="{shape}-{c_in}-{c_out}")
def test_conv_transpose_s2_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- 1. the windowed, normalised MSE -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
@pytest.mark.parametrize("n, side", [(3, 23), (2, 15), (4, 63), (1, 1)])
def test_window_normalised_mse_against_float64(device, dtype, n, side):
    K = _ops()
    g = _g(500 + side)
    y_hat = _randn(g, n, side, side, scale=2.0)
    target = torch.randint(0, 1024, (n, side + 1, side + 1), generator=g).to(dtype)
    loss, grad = K.mse_window_norm_f32(y_hat.to(device), target.to(device), 0, 0)
    t64 = R.normalise64(target)[..., :-1, :-1]
    d64 = y_hat.double() - t64
    ref = (d64 ** 2).mean()
    assert abs(loss.item() - ref.item()) <= 1e-5 * ref.item()
    count = n * side * side
    assert _rel(grad, 2 * d64 / count) <= NORM_TOL
    _within(grad, 2 * d64 / count, 2 * (y_hat.double().abs() + t64.abs()) / count, what="dy_hat")


# ---- 2. refusals through the Python surface ----------------------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    import ctypes
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(RuntimeError, match="status -2"):                       # widths beyond the limit
        K.conv2d_s2_fwd_f32(z(1, 32, 8, 130), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_s2_fwd_f32(z(1, 32, 8, 64), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_s2_counts_fwd_f32(z(1, 4, 40, 130).to(torch.int16), z(1, 40, 130), z(1), z(16, 6, 3, 3), z(16))
    with pytest.raises(RuntimeError, match="status -2"):                       # wrong channel pairs
        K.conv2d_s2_fwd_f32(z(1, 32, 8, 8), z(16, 32, 3, 3), z(16))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_s2_fwd_f32(z(1, 16, 8, 8), z(16, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_s2_bwd_data_f32(z(1, 16, 17, 17), None, z(16, 16, 3, 3), None, (1, 16, 8, 8))
    with pytest.raises(RuntimeError, match="status -2"):                       # too small for four stride-2 layers
        K.conv2d_s2_counts_fwd_f32(z(1, 4, 30, 30).to(torch.int16), z(1, 30, 30), z(1), z(16, 6, 3, 3), z(16))
    with pytest.raises(RuntimeError, match="window"):
        K.mse_window_norm_f32(z(2, 23, 23), z(2, 24, 24).to(torch.int16), 2, 0)
    with pytest.raises(TypeError):
        K.conv2d_s2_counts_fwd_f32(z(1, 4, 40, 40).double(), z(1, 40, 40), z(1), z(16, 6, 3, 3), z(16))
    # a short workspace: one byte less than the query asks for
    lib = _lib.get_lib()
    need = ctypes.c_size_t(0)
    x, dy, dw, db, ws = z(2, 32, 15, 15), z(2, 32, 7, 7), z(32, 32, 3, 3), z(32), z(1 << 20)
    assert lib.pv_conv2d_s2_bwd_weight_workspace_bytes(2, 32, 32, 15, 15, ctypes.byref(need)) == 0 and 0 < need.value < 1 << 22
    assert lib.pv_conv2d_s2_bwd_weight_f32(ptr(x), ptr(dy), None, ptr(dw), ptr(db), 2, 32, 32, 15, 15, ptr(ws),
                                           need.value - 1, None) == -1
    assert lib.pv_convt2d_s2_bwd_weight_workspace_bytes(2, 32, 32, 7, 7, ctypes.byref(need)) == 0 and 0 < need.value < 1 << 22
    assert lib.pv_convt2d_s2_bwd_weight_f32(ptr(dy), ptr(x), None, ptr(dw), ptr(db), 2, 32, 32, 7, 7, ptr(ws),
                                            need.value - 1, None) == -1
    assert "workspace" in lib.pv_last_error().decode()
