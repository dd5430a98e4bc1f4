"""GPU: the padded 64 / 128-channel Conv2d frame predictor of notebooks/10_just_conv.ipynb (csrc/conv2d_wide_f32.hip,
conv2d_functional, models/conv2d/nb10_just_conv.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions (weight and bias gradients).  The model has no
pool, so the golden fixture (torch float32 on the CPU, the notebook's own cell) holds every gradient to NORM_TOL.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import nb10_reference as R
from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu

# (batch, height, width) of the layer's input.  Padding 0: one output; non-square; more than one column band; full width.
# Padding 2: every output touches padding; non-square; an odd width over one band; three column bands of the output
WIDE_SHAPES = {0: [(1, 3, 3), (2, 5, 7), (2, 9, 50), (1, 6, 128)], 2: [(1, 1, 1), (2, 2, 5), (2, 7, 47), (1, 12, 124)]}
STRIPE_SHAPES = [(1, 128, 128), (2, 9, 50), (3, 20, 54)]
HEAD_SHAPES = [(1, 1, 1), (2, 4, 5), (3, 10, 47), (2, 9, 46), (1, 126, 126)]
GATES = ((True, True), (False, False))      # (dy_gate, x_gate): every gradient with and without its gates


def _conv_params(g, c_out, c_in):
    return _randn(g, c_out, c_in, 3, 3, scale=(9 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


# ---- 1. the wide family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in", [64, 128])
@pytest.mark.parametrize("pad, n, h, w", [(p, *s) for p, shapes in WIDE_SHAPES.items() for s in shapes])
def test_wide_conv_against_float64(device, c_in, pad, n, h, w):
    K = _ops()
    g = _g(300 + 7 * w + c_in + pad)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 128, c_in)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64, padding=pad)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=pad)
    assert tuple(pre.shape) == (n, 128, h + 2 * pad - 2, w + 2 * pad - 2)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv2d_wide_fwd_f32(xd, wd, bd, relu=True, padding=pad)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_wide_fwd_f32(xd, wd, bd, relu=False, padding=pad), pre, absref, what="forward without relu")
    _within(K.conv2d_wide_fwd_f32(xd, wd, None, relu=False, padding=pad), pre - b64.view(1, -1, 1, 1), absref,
            what="forward plain")
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in GATES:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        dx64 = F.conv_transpose2d(dyg, w64, padding=pad)
        absdx = F.conv_transpose2d(dyg.abs(), w64.abs(), padding=pad)
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.conv2d_wide_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device) if use_xg else None, tuple(x.shape),
                                        padding=pad)
        assert tuple(dx.shape) == tuple(x.shape)
        _within(dx, dx64, absdx, what=f"dx gates {use_dg} {use_xg}")
        dw, db = K.conv2d_wide_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape), padding=pad)
        dw2, db2 = K.conv2d_wide_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape), padding=pad)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "the weight gradient's bits differ run to run"
        err_w = _rel(dw, torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dyg, padding=pad))
        err_b = _rel(db, dyg.sum((0, 2, 3)))
        print(f"wide {c_in} pad {pad} {(n, h, w)} gates {use_dg}: dw {err_w:.2e} db {err_b:.2e} (bound {NORM_TOL})")
        assert err_w <= NORM_TOL and err_b <= NORM_TOL


# ---- 2. the stripe first layer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hist", [4, 1])
@pytest.mark.parametrize("n, h, w", STRIPE_SHAPES)
def test_stripe_layer_against_float64(device, n_hist, n, h, w):
    """Against F.conv2d on the materialised float64 input; the starts rotate through column 0, mid-image, clipped at the right
    edge, at / beyond the width (an all-zero plane) and a negative one (clipped at the left edge by the kernel rule)."""
    K = _ops()
    g = _g(100 + w + n_hist)
    hist = _randn(g, n, n_hist, h, w)
    wt, b = _conv_params(g, 64, n_hist + 1)
    w64, b64 = wt.double(), b.double()
    dy = _randn(g, n, 64, h - 2, w - 2)
    pool = [0, w // 2, w - 2, w, w + 3, -3]
    for k in range(len(pool)):
        starts = torch.tensor([pool[(k + i) % len(pool)] for i in range(n)], dtype=torch.int32)
        x64 = torch.cat((hist.double(), R.stripe_plane64(starts, h, w)), dim=1)
        ref = F.conv2d(x64, w64, b64)
        absref = F.conv2d(x64.abs(), w64.abs(), b64.abs())
        y = K.conv2d_wide_stripe_fwd_f32(hist.to(device), starts.to(device), wt.to(device), b.to(device), R.STRIPE_WIDTH)
        assert tuple(y.shape) == (n, 64, h - 2, w - 2)
        _within(y, ref.relu(), absref, what=f"stripe forward starts {starts.tolist()}")
        dw, db = K.conv2d_wide_stripe_bwd_weight_f32(hist.to(device), starts.to(device), dy.to(device), tuple(wt.shape),
                                                     R.STRIPE_WIDTH)
        dw64 = torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dy.double())
        assert _rel(dw, dw64) <= NORM_TOL and _rel(db, dy.double().sum((0, 2, 3))) <= NORM_TOL, starts.tolist()
        # the stripe channel's own gradient: exact zeros where the plane is empty
        if int(x64[:, n_hist].sum()) == 0:
            assert (dw[:, n_hist] == 0).all()


# ---- 3. the stride-2 head ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in", [128, 32])
@pytest.mark.parametrize("n, h, w", HEAD_SHAPES)
def test_head_against_float64(device, c_in, n, h, w):
    K = _ops()
    g = _g(500 + w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 1, c_in)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64, stride=2, padding=2)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2, padding=2)
    assert tuple(pre.shape) == (n, 1, (h + 1) // 2 + 1, (w + 1) // 2 + 1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv2d_head_s2_fwd_f32(xd, wd, bd)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre, absref, what="head forward")
    _within(K.conv2d_head_s2_fwd_f32(xd, wd, None), pre - b64.view(1, -1, 1, 1), absref, what="head forward without bias")
    assert torch.equal(y, K.conv2d_head_s2_fwd_f32(xd, wd, bd))
    dy, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    opad = ((h + 1) % 2, (w + 1) % 2)              # the last row / column of an even side, which the forward never reads
    dx64 = F.conv_transpose2d(dy.double(), w64, stride=2, padding=2, output_padding=opad)
    absdx = F.conv_transpose2d(dy.double().abs(), w64.abs(), stride=2, padding=2, output_padding=opad)
    assert tuple(dx64.shape) == tuple(x.shape)
    for use_xg in (True, False):
        dx = K.conv2d_head_s2_bwd_data_f32(dy.to(device), None, wd, x_gate.to(device) if use_xg else None, tuple(x.shape))
        _within(dx, dx64 * (x_gate > 0) if use_xg else dx64, absdx, what=f"head dx gate {use_xg}")
    dw, db = K.conv2d_head_s2_bwd_weight_f32(xd, dy.to(device), None, tuple(wt.shape))
    dw2, db2 = K.conv2d_head_s2_bwd_weight_f32(xd, dy.to(device), None, tuple(wt.shape))
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "the head's weight gradient differs run to run"
    assert tuple(dw.shape) == tuple(wt.shape) and tuple(db.shape) == (1,)
    err_w = _rel(dw, torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dy.double(), stride=2, padding=2))
    err_b = _rel(db, dy.double().sum((0, 2, 3)))
    print(f"head {c_in} {(n, h, w)}: dw {err_w:.2e} db {err_b:.2e} (bound {NORM_TOL})")
    assert err_w <= NORM_TOL and err_b <= NORM_TOL


# ---- 4. refusals through the Python surface ----------------------------------------------------------------------------
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
