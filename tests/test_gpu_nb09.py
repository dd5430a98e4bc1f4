"""GPU: the stride-2 64 / 128-channel Conv2d / ConvTranspose2d autoencoder of notebooks/09_horizon_represented_as_a_stripe.ipynb
(csrc/conv2d_wide_s2_f32.hip, conv2d_functional, models/conv2d/nb09_stripe_ae.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products| (an element whose reference is exactly 0 must be exactly 0), NORM_TOL relative norm for
reductions (weight and bias gradients).  The model has no pool, so the golden fixture (torch float32 on the CPU, the
notebook's own cell) holds every gradient to NORM_TOL.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.

Shapes are (batch, height, width) of the layer's input.  The tile planners of the gather and scatter forms take smaller tiles
while the grid stays under 512 blocks, so the small shapes all run the smallest tile; PLANNER_* are tiny planes at a batch
large enough that the larger tiles (256 / 128 positions per block in the gather, 128 class positions in the scatter) and
weight-gradient slabs of several tiles are taken.
"""
import pytest
import torch
import torch.nn.functional as F

import nb09_reference as R
from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu

# one output; non-square; even sides (dx's last row and column exactly 0); full width (63 output columns, every column band
# the planner makes); the model's own third-layer plane
CONV_SHAPES = [(1, 3, 3), (2, 5, 7), (2, 8, 10), (1, 4, 128), (2, 31, 31)]
# -> 3 x 3, every output from one source; small non-square; -> 11 x 65; -> 7 x 127, the widest; the model's first decoder plane
CONVT_SHAPES = [(1, 1, 1), (2, 2, 3), (1, 5, 32), (1, 3, 63), (2, 15, 15)]
# (c_in, batch, height, width): gather at 256 positions per block + scatter at 128 class positions + slabs of 6 tiles; gather
# at 128 positions per block
PLANNER_CONV = [(128, 256, 9, 9), (64, 128, 17, 35)]
PLANNER_CONVT = [(256, 2, 3)]
STRIPE_SHAPES = [(1, 128, 128), (2, 9, 50), (3, 20, 54), (9, 128, 128)]      # the last: weight-gradient slabs of two tiles
HEAD_SHAPES = [(1, 1, 1), (2, 4, 5), (3, 10, 47), (1, 63, 63), (1, 3, 126)]
LOSS_SHAPES = [((2, 9, 25), (2, 8, 24)), ((1, 65, 65), (1, 64, 64))]
GATES = ((True, True), (False, False))      # (dy_gate, x_gate): every gradient with and without its gates


def _conv_params(g, c_out, c_in, transposed=False):
    shape = (c_in, c_out, 3, 3) if transposed else (c_out, c_in, 3, 3)
    return _randn(g, *shape, scale=(9 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


def _opad(h, w):
    """The last row / column of an even side, which a 3x3 stride-2 forward never reads."""
    return ((h - 3) % 2, (w - 3) % 2)


# ---- 1. Conv2d, stride 2 -----------------------------------------------------------------------------------------------
def _check_conv_grads(K, device, x, wt, pre, g, gates, tag):
    n, c_in, h, w = x.shape
    x64, w64 = x.double(), wt.double()
    xd, wd = x.to(device), wt.to(device)
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in gates:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        dx64 = F.conv_transpose2d(dyg, w64, stride=2, output_padding=_opad(h, w))
        absdx = F.conv_transpose2d(dyg.abs(), w64.abs(), stride=2, output_padding=_opad(h, w))
        assert tuple(dx64.shape) == tuple(x.shape)
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.conv2d_wide_s2_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device) if use_xg else None, tuple(x.shape))
        assert tuple(dx.shape) == tuple(x.shape)
        _within(dx, dx64, absdx, what=f"{tag} dx gates {use_dg} {use_xg}")
        if h % 2 == 0:
            assert (dx[:, :, -1, :] == 0).all(), "the unread last row of dx is not exactly 0"
        if w % 2 == 0:
            assert (dx[:, :, :, -1] == 0).all(), "the unread last column of dx is not exactly 0"
        dw, db = K.conv2d_wide_s2_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        dw2, db2 = K.conv2d_wide_s2_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "the weight gradient's bits differ run to run"
        err_w = _rel(dw, torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dyg, stride=2))
        err_b = _rel(db, dyg.sum((0, 2, 3)))
        print(f"{tag} gates {use_dg}: dw {err_w:.2e} db {err_b:.2e} (bound {NORM_TOL})")
        assert err_w <= NORM_TOL and err_b <= NORM_TOL


@pytest.mark.parametrize("c_in", [64, 128])
@pytest.mark.parametrize("n, h, w", CONV_SHAPES)
def test_conv_s2_against_float64(device, c_in, n, h, w):
    K = _ops()
    g = _g(900 + 7 * w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 128, c_in)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64, stride=2)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    assert tuple(pre.shape) == (n, 128, (h - 3) // 2 + 1, (w - 3) // 2 + 1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv2d_wide_s2_fwd_f32(xd, wd, bd, relu=True)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_wide_s2_fwd_f32(xd, wd, bd, relu=False), pre, absref, what="forward without relu")
    _within(K.conv2d_wide_s2_fwd_f32(xd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref, what="forward plain")
    _check_conv_grads(K, device, x, wt, pre, g, GATES, f"conv s2 {c_in} {(n, h, w)}")


@pytest.mark.parametrize("c_in, n, h, w", PLANNER_CONV)
def test_conv_s2_larger_tiles_against_float64(device, c_in, n, h, w):
    """The tiles the planners take only on a full grid: forward with ReLU and the gated gradients."""
    K = _ops()
    g = _g(950 + w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 128, c_in)
    pre = F.conv2d(x.double(), wt.double(), b.double(), stride=2)
    absref = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), stride=2)
    _within(K.conv2d_wide_s2_fwd_f32(x.to(device), wt.to(device), b.to(device), relu=True), pre.relu(), absref,
            what="forward relu")
    _check_conv_grads(K, device, x, wt, pre, g, GATES[:1], f"conv s2 {c_in} {(n, h, w)}")


# ---- 2. ConvTranspose2d, stride 2 --------------------------------------------------------------------------------------
def _check_convt(K, device, n, h, w, seed, gates, plain):
    g = _g(seed)
    x = _randn(g, n, 128, h, w)
    wt, b = _conv_params(g, 128, 128, transposed=True)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv_transpose2d(x64, w64, b64, stride=2)
    absref = F.conv_transpose2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    assert tuple(pre.shape) == (n, 128, 2 * h + 1, 2 * w + 1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.convt2d_wide_s2_fwd_f32(xd, wd, bd, relu=True)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    if plain:
        _within(K.convt2d_wide_s2_fwd_f32(xd, wd, bd, relu=False), pre, absref, what="forward without relu")
        _within(K.convt2d_wide_s2_fwd_f32(xd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref, what="forward plain")
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in gates:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        dx64 = F.conv2d(dyg, w64, stride=2)
        absdx = F.conv2d(dyg.abs(), w64.abs(), stride=2)
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.convt2d_wide_s2_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device) if use_xg else None, tuple(x.shape))
        assert tuple(dx.shape) == tuple(x.shape)
        _within(dx, dx64, absdx, what=f"dx gates {use_dg} {use_xg}")
        dw, db = K.convt2d_wide_s2_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        dw2, db2 = K.convt2d_wide_s2_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "the weight gradient's bits differ run to run"
        # the weight [c_in][c_out] is the weight of the stride-2 conv dy -> x: its gradient given "grad_output" x
        err_w = _rel(dw, torch.nn.grad.conv2d_weight(dyg, tuple(wt.shape), x64, stride=2))
        err_b = _rel(db, dyg.sum((0, 2, 3)))
        print(f"convt s2 {(n, h, w)} gates {use_dg}: dw {err_w:.2e} db {err_b:.2e} (bound {NORM_TOL})")
        assert err_w <= NORM_TOL and err_b <= NORM_TOL


@pytest.mark.parametrize("n, h, w", CONVT_SHAPES)
def test_convt_s2_against_float64(device, n, h, w):
    _check_convt(_ops(), device, n, h, w, 1100 + 7 * w + h, GATES, plain=True)


@pytest.mark.parametrize("n, h, w", PLANNER_CONVT)
def test_convt_s2_larger_tiles_against_float64(device, n, h, w):
    """A full grid of tiny planes: the scatter at 128 class positions and the gather at 256 positions per block."""
    _check_convt(_ops(), device, n, h, w, 1150 + w, GATES[:1], plain=False)


# ---- 3. the stripe first layer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hist", [4, 1])
@pytest.mark.parametrize("n, h, w", STRIPE_SHAPES)
def test_stripe_layer_against_float64(device, n_hist, n, h, w):
    """Against F.conv2d on the materialised float64 input; the starts rotate through column 0, mid-image, clipped at the right
    edge, at / beyond the width (an all-zero plane) and a negative one (clipped at the left edge by the kernel rule)."""
    K = _ops()
    g = _g(100 + w + n_hist + n)
    hist = _randn(g, n, n_hist, h, w)
    wt, b = _conv_params(g, 64, n_hist + 1)
    w64, b64 = wt.double(), b.double()
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    dy = _randn(g, n, 64, ho, wo)
    pool = [0, w // 2, w - 2, w, w + 3, -3]
    for k in range(len(pool)):
        starts = torch.tensor([pool[(k + i) % len(pool)] for i in range(n)], dtype=torch.int32)
        x64 = torch.cat((hist.double(), R.stripe_plane64(starts, h, w)), dim=1)
        ref = F.conv2d(x64, w64, b64, stride=2)
        absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
        y = K.conv2d_wide_s2_stripe_fwd_f32(hist.to(device), starts.to(device), wt.to(device), b.to(device), R.STRIPE_WIDTH)
        assert tuple(y.shape) == (n, 64, ho, wo)
        _within(y, ref.relu(), absref, what=f"stripe forward starts {starts.tolist()}")
        dw, db = K.conv2d_wide_s2_stripe_bwd_weight_f32(hist.to(device), starts.to(device), dy.to(device), tuple(wt.shape),
                                                        R.STRIPE_WIDTH)
        dw2, db2 = K.conv2d_wide_s2_stripe_bwd_weight_f32(hist.to(device), starts.to(device), dy.to(device), tuple(wt.shape),
                                                          R.STRIPE_WIDTH)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "the weight gradient's bits differ run to run"
        dw64 = torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dy.double(), stride=2)
        assert _rel(dw, dw64) <= NORM_TOL and _rel(db, dy.double().sum((0, 2, 3))) <= NORM_TOL, starts.tolist()
        # the stripe channel's own gradient: exact zeros where the plane is empty
        if int(x64[:, n_hist].sum()) == 0:
            assert (dw[:, n_hist] == 0).all()


# ---- 4. the one-output-channel ConvTranspose2d head --------------------------------------------------------------------
@pytest.mark.parametrize("c_in", [128, 32])
@pytest.mark.parametrize("n, h, w", HEAD_SHAPES)
def test_head_against_float64(device, c_in, n, h, w):
    K = _ops()
    g = _g(500 + w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 1, c_in, transposed=True)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv_transpose2d(x64, w64, b64)
    absref = F.conv_transpose2d(x64.abs(), w64.abs(), b64.abs())
    assert tuple(pre.shape) == (n, 1, h + 2, w + 2)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.convt2d_head_fwd_f32(xd, wd, bd)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre, absref, what="head forward")
    _within(K.convt2d_head_fwd_f32(xd, wd, None), pre - b64.view(1, -1, 1, 1), absref, what="head forward without bias")
    assert torch.equal(y, K.convt2d_head_fwd_f32(xd, wd, bd)), "the head's forward differs run to run"
    dy, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    dx64 = F.conv2d(dy.double(), w64)
    absdx = F.conv2d(dy.double().abs(), w64.abs())
    assert tuple(dx64.shape) == tuple(x.shape)
    for use_xg in (True, False):
        dx = K.convt2d_head_bwd_data_f32(dy.to(device), None, wd, x_gate.to(device) if use_xg else None, tuple(x.shape))
        _within(dx, dx64 * (x_gate > 0) if use_xg else dx64, absdx, what=f"head dx gate {use_xg}")
    dw, db = K.convt2d_head_bwd_weight_f32(xd, dy.to(device), None, tuple(wt.shape))
    dw2, db2 = K.convt2d_head_bwd_weight_f32(xd, dy.to(device), None, tuple(wt.shape))
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "the head's weight gradient differs run to run"
    assert tuple(dw.shape) == tuple(wt.shape) and tuple(db.shape) == (1,)
    err_w = _rel(dw, torch.nn.grad.conv2d_weight(dy.double(), tuple(wt.shape), x64))
    err_b = _rel(db, dy.double().sum((0, 2, 3)))
    print(f"head {c_in} {(n, h, w)}: dw {err_w:.2e} db {err_b:.2e} (bound {NORM_TOL})")
    assert err_w <= NORM_TOL and err_b <= NORM_TOL


# ---- 5. the loss over a window of the prediction -----------------------------------------------------------------------
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


# ---- 6. refusals through the Python surface and the raw ABI ------------------------------------------------------------
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
