"""GPU: the stride-2 Conv2d / ConvTranspose2d autoencoder of notebooks 14 / 15 (csrc/conv2d_s2_f32.hip, conv2d_functional,
models/conv2d/nb15_strided_ae.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  The model has no pool, so the golden fixture
(torch float32 on the CPU) holds every gradient to NORM_TOL.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import nb15_reference as R
from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _counts, _g, _randn

pytestmark = pytest.mark.gpu

# (batch, height, width) of a Conv2d's input: one output; one output with an unread row and column; an unread column only;
# even sides over several tiles; the model's second layer at full size; full width over several row bands
CONV_SHAPES = [(1, 3, 3), (2, 4, 4), (3, 7, 12), (2, 26, 26), (1, 63, 63), (2, 15, 128)]
COUNTS_SHAPES = [(1, 128, 128), (2, 31, 32), (3, 54, 47)]
# (batch, height, width) of a ConvTranspose2d's input; (1, 5, 60) -> 11 x 121 takes two column bands
CONVT_SHAPES = [(1, 1, 1), (2, 2, 5), (3, 7, 7), (1, 15, 15), (2, 31, 31), (1, 5, 60), (2, 40, 3)]
GATES = ((True, True), (False, False))      # (dy_gate, x_gate): every gradient with and without its gates


def _conv_params(g, c_out, c_in):
    return _randn(g, c_out, c_in, 3, 3, scale=(9 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


def _out(s):
    return (s - 3) // 2 + 1


# ---- 1. Conv2d stride 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in", [16, 32])
@pytest.mark.parametrize("n, h, w", CONV_SHAPES)
def test_conv_s2_against_float64(device, c_in, n, h, w):
    K = _ops()
    g = _g(200 + w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 32, c_in)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64, stride=2)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    assert tuple(pre.shape) == (n, 32, _out(h), _out(w))
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv2d_s2_fwd_f32(xd, wd, bd, relu=True)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_s2_fwd_f32(xd, wd, bd, relu=False), pre, absref, what="forward without relu")
    _within(K.conv2d_s2_fwd_f32(xd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref, what="forward plain")
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    opad = (h - (2 * _out(h) + 1), w - (2 * _out(w) + 1))      # the rows / columns the forward never reads
    for use_dg, use_xg in GATES:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        dx64 = F.conv_transpose2d(dyg, w64, stride=2, output_padding=opad)
        absdx = F.conv_transpose2d(dyg.abs(), w64.abs(), stride=2, output_padding=opad)
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.conv2d_s2_bwd_data_f32(dy.to(device), dy_gate.to(device) if use_dg else None, wd,
                                      x_gate.to(device) if use_xg else None, tuple(x.shape))
        assert tuple(dx.shape) == tuple(x.shape)
        _within(dx, dx64, absdx, what=f"dx gates {use_dg} {use_xg}")
        if h % 2 == 0:
            assert (dx[..., -1, :] == 0).all(), "the unread last row's gradient is exactly 0"
        if w % 2 == 0:
            assert (dx[..., :, -1] == 0).all(), "the unread last column's gradient is exactly 0"
        dw, db = K.conv2d_s2_bwd_weight_f32(xd, dy.to(device), dy_gate.to(device) if use_dg else None, tuple(wt.shape))
        assert _rel(dw, torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dyg, stride=2)) <= NORM_TOL
        assert _rel(db, dyg.sum((0, 2, 3))) <= NORM_TOL


# ---- 2. the counts layer -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, h, w", COUNTS_SHAPES)
def test_counts_layer_against_float64(device, n, h, w):
    K = _ops()
    g = _g(100 + w)
    hist, flow, hor = _counts(g, n, h, w)
    wt, b = _conv_params(g, 16, 6)
    x64 = R.input64(hist, flow, hor)
    w64, b64 = wt.double(), b.double()
    ref = F.conv2d(x64, w64, b64, stride=2)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    y = K.conv2d_s2_counts_fwd_f32(hist.to(device), flow.to(device), hor.to(device), wt.to(device), b.to(device))
    assert tuple(y.shape) == (n, 16, _out(h), _out(w))
    _within(y, ref.relu(), absref, what="counts forward")
    dy = _randn(g, *ref.shape)
    dw, db = K.conv2d_s2_counts_bwd_weight_f32(hist.to(device), flow.to(device), hor.to(device), dy.to(device),
                                               (16, 6, 3, 3))
    dw64 = torch.nn.grad.conv2d_weight(x64, (16, 6, 3, 3), dy.double(), stride=2)
    assert _rel(dw, dw64) <= NORM_TOL and _rel(db, dy.double().sum((0, 2, 3))) <= NORM_TOL


def test_counts_layer_int16_and_f32_inputs_give_identical_bits(device):
    K = _ops()
    g = _g(7)
    hist, flow, hor = _counts(g, 2, 54, 47, integer_flow=True)
    wt, b = _conv_params(g, 16, 6)
    args = [t.to(device) for t in (hor, wt, b)]
    dy = _randn(g, 2, 16, 26, 23).to(device)
    outs = []
    for hd, fd in ((torch.int16, torch.int16), (torch.float32, torch.float32), (torch.int16, torch.float32)):
        hi, fl = hist.to(device=device, dtype=hd), flow.to(device=device, dtype=fd)
        y = K.conv2d_s2_counts_fwd_f32(hi, fl, *args)
        dw, db = K.conv2d_s2_counts_bwd_weight_f32(hi, fl, args[0], dy, (16, 6, 3, 3))
        outs.append((y, dw, db))
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert torch.equal(a, c)


# ---- 3. ConvTranspose2d stride 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in, c_out", [(32, 32), (32, 16), (16, 1)])
@pytest.mark.parametrize("n, h, w", CONVT_SHAPES)
def test_conv_transpose_s2_against_float64(device, c_in, c_out, n, h, w):
    K = _ops()
    g = _g(400 + w + c_in + c_out)
    x = _randn(g, n, c_in, h, w)
    wt = _randn(g, c_in, c_out, 3, 3, scale=(9 * c_in) ** -0.5)
    b = _randn(g, c_out, scale=0.1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    x64 = x.double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv_transpose2d(x64, w64, b64, stride=2)
    absref = F.conv_transpose2d(x64.detach().abs(), w64.detach().abs(), b64.detach().abs(), stride=2)
    for relu in (True, False):
        y = K.convt2d_s2_fwd_f32(xd, wd, bd, relu=relu)
        assert tuple(y.shape) == (n, c_out, 2 * h + 1, 2 * w + 1)
        _within(y, pre.detach().relu() if relu else pre.detach(), absref, what=f"convT forward relu={relu}")
    _within(K.convt2d_s2_fwd_f32(xd, wd, None, relu=False), pre.detach() - b64.detach().view(1, -1, 1, 1), absref,
            what="convT forward without bias")
    dy, dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in GATES:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        for t in (x64, w64, b64):
            t.grad = None
        pre.backward(dyg, retain_graph=True)
        absdx = F.conv2d(dyg.abs(), w64.detach().abs(), stride=2)
        dx = K.convt2d_s2_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device) if use_xg else None, tuple(x.shape))
        _within(dx, x64.grad * (x_gate > 0) if use_xg else x64.grad, absdx, what=f"convT dx gates {use_dg} {use_xg}")
        dw, db = K.convt2d_s2_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        assert tuple(dw.shape) == tuple(wt.shape) and tuple(db.shape) == (c_out,)
        assert _rel(dw, w64.grad) <= NORM_TOL, (use_dg, _rel(dw, w64.grad))
        assert _rel(db, b64.grad) <= NORM_TOL, (use_dg, _rel(db, b64.grad))


# ---- 4. the windowed, normalised MSE -----------------------------------------------------------------------------------
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


# ---- 5. refusals through the Python surface ----------------------------------------------------------------------------
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
