"""GPU: the strided depth-2 Conv3d encoder and the horizon ConvTranspose2d of notebooks/08_multiple_historical_images_as_
separate_channels.ipynb (csrc/conv3d_s2_f32.hip, conv3d_wide_functional, models/conv3d/nb08_hist_depth.py) against float64
on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  The references are float64 F.conv3d,
F.conv_transpose2d (conv_transpose3d for a Conv3d's data gradient), torch.nn.grad.conv3d_weight and, for the
ConvTranspose2d's weight gradient, float64 autograd of F.conv_transpose2d (what torch.nn.grad's conv*_weight functions
compute for a Conv; torch has none for the transposed form).

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _to, _within
from notebook_model_checks import CASES, _g, _randn

pytestmark = pytest.mark.gpu

PAIRS = [(1, 8), (8, 32), (32, 32)]
# (batch, depth, height, width) of a Conv3d's input: one output; an unread row and column over two output depths; an unread
# column only, three output depths (interior input depths receive two taps); even sides over several tiles; the model's
# second layer at full size; full width over several row bands
CONV3D_SHAPES = [(1, 2, 3, 3), (2, 3, 4, 4), (3, 4, 7, 12), (2, 2, 26, 26), (1, 3, 63, 63), (2, 2, 15, 128)]
# (batch, height, width) of the horizon ConvTranspose2d's input; (2, 5, 60) -> 11 x 121 takes two column bands
HORIZON_SHAPES = [(1, 1, 1), (2, 2, 5), (3, 7, 7), (1, 15, 15), (2, 5, 60), (2, 40, 3)]
GATES = ((True, True), (False, False))      # (dy_gate, x_gate): every gradient with and without its gates
STRIDE = (1, 2, 2)


def _out(s):
    return (s - 3) // 2 + 1


# ---- 1. Conv3d (2, 3, 3), stride (1, 2, 2) -------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in, c_out", PAIRS)
@pytest.mark.parametrize("n, d, h, w", CONV3D_SHAPES)
def test_conv3d_s2_against_float64(device, c_in, c_out, n, d, h, w):
    K = _ops()
    g = _g(800 + w + 7 * d + c_in)
    x = _randn(g, n, c_in, d, h, w)
    wt, b = _randn(g, c_out, c_in, 2, 3, 3, scale=(18 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv3d(x64, w64, b64, stride=STRIDE)
    absref = F.conv3d(x64.abs(), w64.abs(), b64.abs(), stride=STRIDE)
    assert tuple(pre.shape) == (n, c_out, d - 1, _out(h), _out(w))
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv3d_s2_fwd_f32(xd, wd, bd, relu=True)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv3d_s2_fwd_f32(xd, wd, bd, relu=False), pre, absref, what="forward without relu")
    _within(K.conv3d_s2_fwd_f32(xd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1, 1), absref, what="forward plain")
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    opad = (0, h - (2 * _out(h) + 1), w - (2 * _out(w) + 1))      # the rows / columns the forward never reads
    for use_dg, use_xg in GATES:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        dw, db = K.conv3d_s2_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        assert tuple(dw.shape) == tuple(wt.shape) and tuple(db.shape) == (c_out,)
        dw64 = torch.nn.grad.conv3d_weight(x64, tuple(wt.shape), dyg, stride=STRIDE)
        for kd in range(2):     # each depth tap on its own: the two halves of dw come from two launches
            err = _rel(dw[:, :, kd], dw64[:, :, kd])
            assert err <= NORM_TOL, (use_dg, kd, err)
        assert _rel(db, dyg.sum((0, 2, 3, 4))) <= NORM_TOL
        if c_in == 1:
            continue                                              # the first layer has no data gradient
        dx64 = F.conv_transpose3d(dyg, w64, stride=STRIDE, output_padding=opad)
        absdx = F.conv_transpose3d(dyg.abs(), w64.abs(), stride=STRIDE, output_padding=opad)
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.conv3d_s2_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device) if use_xg else None, tuple(x.shape))
        assert tuple(dx.shape) == tuple(x.shape)
        for z in range(d):      # edge depths receive one depth tap, interior ones two: a dropped or doubled tap shows here
            _within(dx[:, :, z], dx64[:, :, z], absdx[:, :, z], what=f"dx depth {z} of {d}, gates {use_dg} {use_xg}")
        if h % 2 == 0:
            assert (dx[..., -1, :] == 0).all(), "the unread last row's gradient is exactly 0"
        if w % 2 == 0:
            assert (dx[..., :, -1] == 0).all(), "the unread last column's gradient is exactly 0"


def test_conv3d_s2_first_layer_has_no_data_gradient(device):
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)
    with pytest.raises(ValueError, match="no data gradient"):
        K.conv3d_s2_bwd_data_f32(z(1, 8, 1, 3, 3), None, z(8, 1, 2, 3, 3), None, (1, 1, 2, 7, 7))


# ---- 2. the depth-pair identity on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("n, h, w", [(2, 26, 26), (1, 63, 63), (2, 15, 128)])
def test_depth_pair_identity(device, n, h, w):
    """At depth 2 the strided Conv3d is the stride-2 Conv2d over the [n, 2 c, h, w] view with the [m, 2 c, 3, 3] weight view."""
    K = _ops()
    g = _g(900 + w)
    x = _randn(g, n, 8, 2, h, w)
    wt, b = _randn(g, 32, 8, 2, 3, 3, scale=144 ** -0.5), _randn(g, 32, scale=0.1)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    ref = F.conv3d(x64, w64, b64, stride=STRIDE).relu()
    absref = F.conv3d(x64.abs(), w64.abs(), b64.abs(), stride=STRIDE)
    assert torch.equal(ref, F.conv2d(x64.view(n, 16, h, w), w64.view(32, 16, 3, 3), b64, stride=2).relu().unsqueeze(2))
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y3 = K.conv3d_s2_fwd_f32(xd, wd, bd, relu=True)
    y2 = K.conv2d_s2_fwd_f32(xd.view(n, 16, h, w), wd.view(32, 16, 3, 3), bd, relu=True)
    assert tuple(y3.shape) == (n, 32, 1, _out(h), _out(w))
    _within(y3, ref, absref, what="conv3d_s2 at depth 2")
    _within(y2.unsqueeze(2), ref, absref, what="conv2d_s2 on the depth-pair view")


# ---- 3. ConvTranspose2d 33 -> 32 with the horizon as its last input channel ----------------------------------------------
@pytest.mark.parametrize("n, h, w", HORIZON_SHAPES)
def test_horizon_conv_transpose_against_float64(device, n, h, w):
    K = _ops()
    g = _g(1000 + w + h)
    x = _randn(g, n, 32, h, w)
    horizon = torch.tensor([0.0, -1.3, 0.7][:n]) if n > 1 else torch.tensor([-0.4])      # zero and both signs
    wt = _randn(g, 33, 32, 3, 3, scale=(9 * 33) ** -0.5)
    b = _randn(g, 32, scale=0.1)
    xd, hd, wd, bd = x.to(device), horizon.to(device), wt.to(device), b.to(device)
    x33 = torch.cat((x.double(), horizon.double().view(n, 1, 1, 1).expand(n, 1, h, w)), dim=1).requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv_transpose2d(x33, w64, b64, stride=2)
    absref = F.conv_transpose2d(x33.detach().abs(), w64.detach().abs(), b64.detach().abs(), stride=2)
    for relu in (True, False):
        y = K.convt2d_s2_horizon_fwd_f32(xd, hd, wd, bd, relu=relu)
        assert tuple(y.shape) == (n, 32, 2 * h + 1, 2 * w + 1)
        _within(y, pre.detach().relu() if relu else pre.detach(), absref, what=f"horizon convT forward relu={relu}")
    _within(K.convt2d_s2_horizon_fwd_f32(xd, hd, wd, None, relu=False), pre.detach() - b64.detach().view(1, -1, 1, 1), absref,
            what="horizon convT forward without bias")
    dy, dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in GATES:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        for t in (x33, w64, b64):
            t.grad = None
        pre.backward(dyg, retain_graph=True)
        dw, db = K.convt2d_s2_horizon_bwd_weight_f32(xd, hd, dy.to(device), gate_d, tuple(wt.shape))
        assert tuple(dw.shape) == (33, 32, 3, 3) and tuple(db.shape) == (32,)
        dw64 = w64.grad      # float64 autograd of conv_transpose2d (this torch has no torch.nn.grad.conv_transpose2d_weight)
        assert _rel(dw, dw64) <= NORM_TOL, (use_dg, _rel(dw, dw64))
        assert _rel(dw[32], dw64[32]) <= NORM_TOL, (use_dg, "horizon row", _rel(dw[32], dw64[32]))
        assert _rel(dw[:32], dw64[:32]) <= NORM_TOL, (use_dg, "real rows", _rel(dw[:32], dw64[:32]))
        assert _rel(db, b64.grad) <= NORM_TOL, (use_dg, _rel(db, b64.grad))
        # the 32 real channels' data gradient: the existing entry point on the first 32 rows of the weight (contiguous)
        dx = K.convt2d_s2_bwd_data_f32(dy.to(device), gate_d, wd[:32], x_gate.to(device) if use_xg else None, tuple(x.shape))
        absdx = F.conv2d(dyg.abs(), w64.detach()[:32].abs(), stride=2)
        dx64 = x33.grad[:, :32]
        _within(dx, dx64 * (x_gate > 0) if use_xg else dx64, absdx, what=f"horizon convT dx gates {use_dg} {use_xg}")


# ---- 4. refusals through the Python surface ----------------------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    import ctypes
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(ValueError, match="128 columns"):                       # widths beyond the limit
        K.conv3d_s2_fwd_f32(z(1, 8, 2, 8, 130), z(32, 8, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        K.convt2d_s2_horizon_fwd_f32(z(1, 32, 8, 64), z(1), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="C_in, C_out"):                       # wrong channel pairs
        K.conv3d_s2_fwd_f32(z(1, 16, 2, 8, 8), z(32, 16, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="no data gradient"):
        K.conv3d_s2_bwd_data_f32(z(1, 8, 1, 3, 3), None, z(8, 1, 2, 3, 3), None, (1, 1, 2, 8, 8))
    with pytest.raises(TypeError):
        K.conv3d_s2_fwd_f32(z(1, 8, 2, 8, 8).double(), z(32, 8, 2, 3, 3), z(32))
    with pytest.raises(TypeError):
        K.convt2d_s2_horizon_fwd_f32(z(1, 32, 8, 8), z(1).double(), z(33, 32, 3, 3), z(32))
    model = CASES["nb08"].model_cls()().to(device)
    good = _to(CASES["nb08"].full_batch(80, 2, 31), device)
    with pytest.raises(ValueError, match="TARGET_SAT_IMAGE"):
        model.training_step({**good, "TARGET_SAT_IMAGE": z(2, 17, 17)}, 0)
    for side in (14, 129):
        with pytest.raises(ValueError, match="15 to 128"):
            model({**good, "HISTORICAL_SAT_IMAGES": z(2, 4, side, side)})
    for frames in (3, 5):
        with pytest.raises(ValueError, match="HISTORICAL_SAT_IMAGES"):
            model({**good, "HISTORICAL_SAT_IMAGES": z(2, frames, 31, 31)})
    with pytest.raises(ValueError, match="FORECAST_HORIZON"):
        model({**good, "FORECAST_HORIZON": z(3)})
    # the C ABI itself: a shape the glue would have stopped, and a workspace one byte short of what the query asks for
    lib = _lib.get_lib()
    need = ctypes.c_size_t(0)
    x, dy, dw, db, ws = z(2, 8, 3, 15, 15), z(2, 32, 2, 7, 7), z(32, 8, 2, 3, 3), z(32), z(1 << 20)
    assert lib.pv_conv3d_s2_fwd_f32(ptr(x), ptr(dw), ptr(db), ptr(dy), 2, 8, 32, 3, 15, 130, 1, None) == -2
    assert lib.pv_conv3d_s2_bwd_weight_workspace_bytes(2, 8, 32, 3, 15, 15, ctypes.byref(need)) == 0 and 0 < need.value < 1 << 22
    dw.fill_(7.0)
    assert lib.pv_conv3d_s2_bwd_weight_f32(ptr(x), ptr(dy), None, ptr(dw), ptr(db), 2, 8, 32, 3, 15, 15, ptr(ws),
                                           need.value - 1, None) == -1
    torch.cuda.synchronize()
    assert (dw == 7.0).all(), "nothing was launched"
