"""GPU: notebook 16's max-pool Conv2d / ConvTranspose2d frame predictor (csrc/conv2d_ae_f32.hip, conv2d_functional,
models/conv2d/nb16_maxpool.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  A max pool is a selection, so its codes are
checked on their own (the picked entry is the window's float64 maximum within the tolerance) and the float64 gradients are
then routed through the kernel's own codes, every window included.  Against the golden fixture (torch float32 on the CPU,
another implementation's picks) the encoder gradients are held to ROUTED_TOL.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import nb16_reference as R
from conv2d_f32_helpers import ELEM_TOL, NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _counts, _g, _randn

pytestmark = pytest.mark.gpu

DEAD = 255
# (batch, height, width): widths 128, 127, 44, 38, 36, 11 -- multiples and non-multiples of every tile extent
SHAPES = [(1, 128, 128), (1, 21, 127), (2, 44, 44), (3, 38, 38), (2, 36, 36), (2, 11, 11)]
# the Conv2d layers (plain and pooled) also at a size that takes the general Conv3d route (>= 32768 output positions)
CONV_SHAPES = SHAPES + [(3, 128, 128)]


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


# ---- 1. each entry point against float64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("n, h, w", SHAPES)
def test_counts_layer_against_float64(device, n, h, w):
    K = _ops()
    g = _g(100 + w)
    hist, flow, hor = _counts(g, n, h, w)
    wt, b = _conv_params(g, 16, 6)
    x64 = R.input64(hist, flow, hor)
    w64, b64 = wt.double(), b.double()
    ref = F.conv2d(x64, w64, b64)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs())
    y = K.conv2d_ae_counts_fwd_f32(hist.to(device), flow.to(device), hor.to(device), wt.to(device), b.to(device))
    assert tuple(y.shape) == (n, 16, h - 2, w - 2)
    _within(y, ref.relu(), absref, what="counts forward")
    dy = _randn(g, n, 16, h - 2, w - 2)
    dw, db = K.conv2d_ae_counts_bwd_weight_f32(hist.to(device), flow.to(device), hor.to(device), dy.to(device),
                                               (16, 6, 3, 3))
    dw64 = torch.nn.grad.conv2d_weight(x64, (16, 6, 3, 3), dy.double())
    assert _rel(dw, dw64) <= NORM_TOL and _rel(db, dy.double().sum((0, 2, 3))) <= NORM_TOL


def test_counts_layer_int16_and_f32_inputs_give_identical_bits(device):
    K = _ops()
    g = _g(7)
    hist, flow, hor = _counts(g, 2, 38, 36, integer_flow=True)
    wt, b = _conv_params(g, 16, 6)
    args = [t.to(device) for t in (hor, wt, b)]
    dy = _randn(g, 2, 16, 36, 34).to(device)
    outs = []
    for hd, fd in ((torch.int16, torch.int16), (torch.float32, torch.float32), (torch.int16, torch.float32)):
        hi, fl = hist.to(device=device, dtype=hd), flow.to(device=device, dtype=fd)
        y = K.conv2d_ae_counts_fwd_f32(hi, fl, *args)
        dw, db = K.conv2d_ae_counts_bwd_weight_f32(hi, fl, args[0], dy, (16, 6, 3, 3))
        outs.append((y, dw, db))
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert torch.equal(a, c)


@pytest.mark.parametrize("c_in", [16, 32])
@pytest.mark.parametrize("n, h, w", CONV_SHAPES)
def test_conv_against_float64(device, c_in, n, h, w):
    K = _ops()
    g = _g(200 + w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 32, c_in)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs())
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv2d_ae_fwd_f32(xd, wd, bd, relu=True)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_ae_fwd_f32(xd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref, what="forward plain")
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in ((True, True), (False, False), (True, False)):
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        dx64 = F.conv_transpose2d(dyg, w64)
        absdx = F.conv_transpose2d(dyg.abs(), w64.abs())
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.conv2d_ae_bwd_data_f32(dy.to(device), dy_gate.to(device) if use_dg else None, wd,
                                      x_gate.to(device) if use_xg else None, tuple(x.shape))
        _within(dx, dx64, absdx, what=f"dx gates {use_dg} {use_xg}")
        dw, db = K.conv2d_ae_bwd_weight_f32(xd, dy.to(device), dy_gate.to(device) if use_dg else None, tuple(wt.shape))
        assert _rel(dw, torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dyg)) <= NORM_TOL
        assert _rel(db, dyg.sum((0, 2, 3))) <= NORM_TOL


# ---- 2. the fused pool: codes on their own, then float64 gradients routed through them -----------------------------
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


# ---- 3. ConvTranspose2d ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in, c_out", [(32, 32), (32, 16), (16, 16), (16, 1)])
@pytest.mark.parametrize("n, h, w", [(1, 40, 40), (2, 3, 126), (3, 10, 9), (2, 46, 46), (1, 1, 1)])
def test_conv_transpose_against_float64(device, c_in, c_out, n, h, w):
    K = _ops()
    g = _g(400 + w + c_in + c_out)
    x = _randn(g, n, c_in, h, w)
    wt = _randn(g, c_in, c_out, 3, 3, scale=(9 * c_in) ** -0.5)
    b = _randn(g, c_out, scale=0.1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    x64 = x.double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv_transpose2d(x64, w64, b64)
    absref = F.conv_transpose2d(x64.detach().abs(), w64.detach().abs(), b64.detach().abs())
    for relu in (True, False):
        y = K.convt2d_ae_fwd_f32(xd, wd, bd, relu=relu)
        assert tuple(y.shape) == (n, c_out, h + 2, w + 2)
        _within(y, pre.detach().relu() if relu else pre.detach(), absref, what=f"convT forward relu={relu}")
    _within(K.convt2d_ae_fwd_f32(xd, wd, None, relu=False), pre.detach() - b64.detach().view(1, -1, 1, 1), absref,
            what="convT forward without bias")
    dy, dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg in (True, False):       # with and without a ReLU gate on dy
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        for t in (x64, w64, b64):
            t.grad = None
        pre.backward(dyg, retain_graph=True)
        absdx = F.conv2d(dyg.abs(), w64.detach().abs())
        dx = K.convt2d_ae_bwd_data_f32(dy.to(device), gate_d, wd, None, tuple(x.shape))
        _within(dx, x64.grad, absdx, what=f"convT dx gate={use_dg}")
        dxg = K.convt2d_ae_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device), tuple(x.shape))
        _within(dxg, x64.grad * (x_gate > 0), absdx, what=f"convT dx gated gate={use_dg}")
        dw, db = K.convt2d_ae_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        assert tuple(dw.shape) == tuple(wt.shape) and tuple(db.shape) == (c_out,)
        assert _rel(dw, w64.grad) <= NORM_TOL, (use_dg, _rel(dw, w64.grad))
        assert _rel(db, b64.grad) <= NORM_TOL, (use_dg, _rel(db, b64.grad))


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


# ---- 5. refusals through the Python surface ------------------------------------------------------------------------
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
