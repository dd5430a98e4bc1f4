"""GPU: notebook 16's max-pool Conv2d / ConvTranspose2d frame predictor (csrc/conv2d_ae_f32.hip, conv2d_functional,
models/conv2d/nb16_maxpool.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  A max pool is a selection, so its codes are
checked on their own (the picked entry is the window's float64 maximum within the tolerance) and the float64 gradients are
then routed through the kernel's own codes, every window included.  Against the golden fixture (torch float32 on the CPU,
another implementation's picks) the encoder gradients are held to ROUTED_TOL.

The three passes of conv2d_ae and convt2d_ae and the counts first layer are checked below by the records
and the one checker of tests/conv_family_checks.py.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import nb16_reference as R
import conv_family_checks as C
from conv2d_f32_helpers import ELEM_TOL, NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu

DEAD = 255
CONV_SHAPES = C.BY_NAME["conv2d_ae"].shapes      # the pooled layer at the plain layer's shapes, both routes


def _conv_params(g, c_out, c_in):
    return _randn(g, c_out, c_in, 3, 3, scale=(9 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


def _windows(z, ph, pw):
    n, c = z.shape[:2]
    z = z[:, :, :3 * ph, :3 * pw].reshape(n, c, ph, 3, pw, 3)
    return z.permute(0, 1, 2, 4, 3, 5).reshape(n, c, ph, pw, 9)


def _check_pool(y, codes, pre64, abs64, what):
    """pooled y and codes against float64 pre-activations: the pick and the value (as tests/test_gpu_exp001.py)."""
    ph, pw = codes.shape[2:]
    zc, ac = _windows(pre64, ph, pw), _windows(abs64, ph, pw)
    tol = ELEM_TOL * ac.amax(-1)
    m = zc.amax(-1)
    codes = codes.cpu().long()
    live = codes != DEAD
    assert ((codes <= 8) | ~live).all(), what
    assert (m[~live] <= tol[~live]).all(), f"{what}: a dead window has a positive maximum"
    assert (m[live] >= -tol[live]).all(), f"{what}: a live window has a negative maximum"
    picked = zc.gather(-1, codes.clamp(max=8).unsqueeze(-1)).squeeze(-1)
    assert ((m - picked)[live] <= 2 * tol[live]).all(), f"{what}: the code does not pick the maximum"
    _within(y, m.relu(), ac.amax(-1), what=what)
    assert (y.cpu()[~live] == 0).all()


def _pool_by_codes(z, codes):
    """relu(max_pool2d(z, 3)) in float64 with the window picks of `codes` (autograd routes through them)."""
    ph, pw = codes.shape[2:]
    codes = codes.cpu().long()
    live = codes != DEAD
    picked = _windows(z, ph, pw).gather(-1, codes.clamp(max=8).unsqueeze(-1)).squeeze(-1)
    return torch.where(live, picked, torch.zeros_like(picked))


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.twin_shapes("conv2d_ae_counts")
def test_counts_layer_against_float64(device, twin, shape):
    C.check_counts_layer(_ops(), device, twin, shape)


def test_counts_layer_int16_and_f32_inputs_give_identical_bits(device):
    C.check_counts_layer_input_dtypes(_ops(), device, C.TWINS["conv2d_ae_counts"])


@C.cases_of("conv2d_ae", ids="{shape}-{c_in}")
def test_conv_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.cases_of("convt2d_ae", ids="{shape}-{c_in}-{c_out}")
def test_conv_transpose_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- 1. the fused pool: codes on their own, then float64 gradients routed through them -----------------------------
@pytest.mark.parametrize("n, h, w", CONV_SHAPES)
def test_pooled_conv_against_float64(device, n, h, w):
    K = _ops()
    g = _g(300 + w)
    x = _randn(g, n, 32, h, w)
    wt, b = _conv_params(g, 32, 32)
    b = b - 0.3                                   # some dead windows
    x64 = x.double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.conv2d(x64, w64, b64)
    z.retain_grad()
    absref = F.conv2d(x64.detach().abs(), w64.detach().abs(), b64.detach().abs())
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y, codes = K.conv2d_ae_pool_fwd_f32(xd, wd, bd)
    ph, pw = (h - 2) // 3, (w - 2) // 3
    assert tuple(y.shape) == (n, 32, ph, pw) and codes.dtype == torch.uint8 and tuple(codes.shape) == tuple(y.shape)
    _check_pool(y, codes, z.detach(), absref, "pool forward")
    dyp = _randn(g, n, 32, ph, pw)
    _pool_by_codes(z, codes).backward(dyp.double())
    absdx = F.conv_transpose2d(z.grad.abs(), w64.detach().abs())
    x_gate = _randn(g, *x.shape)
    dx = K.conv2d_ae_pool_bwd_data_f32(dyp.to(device), codes, wd, None, tuple(x.shape))
    _within(dx, x64.grad, absdx, what="pooled dx")
    dxg = K.conv2d_ae_pool_bwd_data_f32(dyp.to(device), codes, wd, x_gate.to(device), tuple(x.shape))
    _within(dxg, x64.grad * (x_gate > 0), absdx, what="pooled dx gated")
    dw, db = K.conv2d_ae_pool_bwd_weight_f32(xd, dyp.to(device), codes, tuple(wt.shape))
    assert _rel(dw, w64.grad) <= NORM_TOL and _rel(db, b64.grad) <= NORM_TOL


# ---- 2. the cropped, normalised MSE ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
@pytest.mark.parametrize("n, side", [(3, 18), (2, 17), (4, 48), (1, 1)])
def test_cropped_normalised_mse_against_float64(device, dtype, n, side):
    K = _ops()
    g = _g(500 + side)
    y_hat = _randn(g, n, side, side, scale=2.0)
    target = torch.randint(0, 1024, (n, side + 16, side + 16), generator=g).to(dtype)
    loss, grad = K.mse_crop_norm_f32(y_hat.to(device), target.to(device))
    t64 = R.normalise64(target)[..., 8:-8, 8:-8]
    d64 = y_hat.double() - t64
    ref = (d64 ** 2).mean()
    assert abs(loss.item() - ref.item()) <= 1e-5 * ref.item()
    count = n * side * side
    _within(grad, 2 * d64 / count, 2 * (y_hat.double().abs() + t64.abs()) / count, what="dy_hat")


# ---- 3. refusals through the Python surface ------------------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 130), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 8), z(16, 32, 3, 3), z(16))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_counts_fwd_f32(z(1, 4, 10, 10).to(torch.int16), z(1, 10, 10), z(1), z(16, 6, 3, 3), z(16))
    with pytest.raises(ValueError, match="at least 5 x 5"):
        K.conv2d_ae_pool_fwd_f32(z(1, 32, 4, 9), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_pool_fwd_f32(z(1, 16, 9, 9), z(32, 16, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_ae_fwd_f32(z(1, 16, 8, 8), z(16, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_ae_fwd_f32(z(1, 32, 8, 127), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="target side"):
        K.mse_crop_norm_f32(z(2, 18, 18), z(2, 33, 33).to(torch.int16))
    with pytest.raises(TypeError):
        K.conv2d_ae_counts_fwd_f32(z(1, 4, 12, 12).double(), z(1, 12, 12), z(1), z(16, 6, 3, 3), z(16))
