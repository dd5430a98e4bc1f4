"""GPU: the 64 / 128-channel (2, 3, 3) Conv3d frame predictor of notebooks/12_just_3d_conv.ipynb (csrc/conv3d_wide_f32.hip,
conv3d_wide_functional, models/conv3d/nb12_just_3d_conv.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL = 1e-6 per element relative to the
element's float64 sum of |products|, NORM_TOL = 1e-5 relative norm for reductions (weight and bias gradients).  A float32
running sum's error relative to sum|p| does not grow with K, so the 2 304 products of a 128-channel output need no wider
bound; torch float32 on the CPU is itself 6.4e-8 (elements) and 6.2e-7 (weight gradient) from float64 at these shapes, which
leaves the reference more than 15 x margin.

The three passes of conv3d_wide at both depth paddings and of conv2d_head_s2p1 are checked below by the records
and the one checker of tests/conv_family_checks.py.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nb12_reference as R
import conv_family_checks as C
from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _within
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu

HORIZON_SHAPES = [(1, 128, 128), (2, 9, 50), (3, 5, 7)]


def _conv_params(g, c_out, c_in, kernel=(2, 3, 3)):
    return _randn(g, c_out, c_in, *kernel, scale=(int(np.prod(kernel)) * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of({"conv3d_wide_pd0": 0, "conv3d_wide_pd1": 1}, ids="{tag}-{shape}-{c_in}")
def test_wide_conv3d_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.cases_of("conv2d_head_s2p1", ids="{shape}-{c_in}")
def test_head_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- 1. the horizon first layer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_in", [4, 2])
@pytest.mark.parametrize("n, h, w", HORIZON_SHAPES)
def test_horizon_layer_against_float64(device, d_in, n, h, w):
    """Against F.conv3d on the materialised float64 input; the horizons rotate through 0.0, a negative and positive ones, then
    all are 0: the horizon channel's weight gradient is then exactly 0."""
    K = _ops()
    g = _g(100 + w + d_in)
    hist = _randn(g, n, d_in, h, w)
    wt, b = _conv_params(g, 64, 2)
    w64, b64 = wt.double(), b.double()
    dy = _randn(g, n, 64, d_in - 1, h, w)
    pool = [0.0, -1.6613, 0.5055, 1.5168]
    rounds = [[pool[(k + i) % len(pool)] for i in range(n)] for k in range(len(pool))] + [[0.0] * n]
    for values in rounds:
        horizon = torch.tensor(values, dtype=torch.float32)
        x64 = R.input64(hist, horizon)
        ref = F.conv3d(x64, w64, b64, padding=(0, 1, 1))
        absref = F.conv3d(x64.abs(), w64.abs(), b64.abs(), padding=(0, 1, 1))
        y = K.conv3d_wide_horizon_fwd_f32(hist.to(device), horizon.to(device), wt.to(device), b.to(device))
        assert tuple(y.shape) == (n, 64, d_in - 1, h, w)
        _within(y, ref.relu(), absref, what=f"horizon forward {values}")
        dw, db = K.conv3d_wide_horizon_bwd_weight_f32(hist.to(device), horizon.to(device), dy.to(device), tuple(wt.shape))
        dw2, db2 = K.conv3d_wide_horizon_bwd_weight_f32(hist.to(device), horizon.to(device), dy.to(device), tuple(wt.shape))
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "the weight gradient's bits differ run to run"
        dw64 = torch.nn.grad.conv3d_weight(x64, tuple(wt.shape), dy.double(), padding=(0, 1, 1))
        err_w, err_b = _rel(dw, dw64), _rel(db, dy.double().sum((0, 2, 3, 4)))
        print(f"horizon d {d_in} {(n, h, w)} {values}: dw {err_w:.2e} db {err_b:.2e} (bound {NORM_TOL})")
        assert err_w <= NORM_TOL and err_b <= NORM_TOL, values
        if not any(values):
            assert (dw[:, 1] == 0).all(), "the horizon channel's gradient is not exactly 0 under all-zero horizons"


# ---- 2. the stride-2 padding-1 head against its twins ------------------------------------------------------------------
def test_strided_heads_are_one_kernel_set_at_two_paddings(device):
    """The padding-2 head on x and the padding-1 head on x with a ring of zeros are the same kernels at PAD = 2 and 1, so they
    agree bit for bit: a tap in the zero ring is fmaf(w, 0.0f, s), exactly what the out-of-image predicate gives, and the
    thread -> position maps and slab plans depend only on the output extent ((s + 1) // 2 + 1 on both sides).  c_in = 5 is
    no multiple of the four partial sums, the sides are odd and even, 18 output rows are two bands of 16."""
    K = _ops()
    g = _g(700)
    x = _randn(g, 2, 5, 33, 6)
    wt, b = _conv_params(g, 1, 5, kernel=(3, 3))
    xp = F.pad(x, (1, 1, 1, 1))
    xd, xpd, wd, bd = x.to(device), xp.to(device).contiguous(), wt.to(device), b.to(device)
    y2, y1 = K.conv2d_head_s2_fwd_f32(xd, wd, bd), K.conv2d_head_s2p1_fwd_f32(xpd, wd, bd)
    assert tuple(y2.shape) == tuple(y1.shape) == (2, 1, 18, 4)
    assert torch.equal(y2, y1), "forward"
    dy = _randn(g, *y2.shape).to(device)
    dw2, db2 = K.conv2d_head_s2_bwd_weight_f32(xd, dy, None, tuple(wt.shape))
    dw1, db1 = K.conv2d_head_s2p1_bwd_weight_f32(xpd, dy, None, tuple(wt.shape))
    assert torch.equal(dw2, dw1) and torch.equal(db2, db1), "weight / bias gradient"
    x_gate = _randn(g, *x.shape)
    gate_p = F.pad(x_gate, (1, 1, 1, 1)).to(device).contiguous()
    dx2 = K.conv2d_head_s2_bwd_data_f32(dy, None, wd, x_gate.to(device), tuple(x.shape))
    dx1 = K.conv2d_head_s2p1_bwd_data_f32(dy, None, wd, gate_p, tuple(xp.shape))
    assert torch.equal(dx2, dx1[:, :, 1:-1, 1:-1]), "data gradient"
    assert dx2.abs().sum() > 0 and dw2.abs().sum() > 0


@pytest.mark.parametrize("n, h, w", [(2, 9, 46), (1, 1, 1), (2, 10, 47)])
def test_head_depth2_view_against_float64_conv3d(device, n, h, w):
    """conv.8 on depth 2: the Conv2d head on the views [n][2 c][h][w] / [1][2 c][3][3] against F.conv3d itself."""
    K = _ops()
    g = _g(600 + w)
    x = _randn(g, n, 128, 2, h, w)
    wt, b = _conv_params(g, 1, 128)
    x64, w64, b64 = x.double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv3d(x64, w64, b64, stride=(1, 2, 2), padding=(0, 1, 1))
    absref = F.conv3d(x64.detach().abs(), w64.detach().abs(), b64.detach().abs(), stride=(1, 2, 2), padding=(0, 1, 1))
    assert tuple(pre.shape) == (n, 1, 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv3d_head_d2_fwd_f32(xd, wd, bd)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.detach(), absref, what="depth-2 head forward")
    dy = _randn(g, *pre.shape)
    pre.backward(dy.double())
    absdx = torch.autograd.grad(F.conv3d(x64, w64.detach().abs(), None, stride=(1, 2, 2), padding=(0, 1, 1)), x64,
                                dy.double().abs())[0]
    dx = K.conv3d_head_d2_bwd_data_f32(dy.to(device), None, wd, None, tuple(x.shape))
    assert tuple(dx.shape) == tuple(x.shape)
    _within(dx, x64.grad, absdx, what="depth-2 head dx")
    dw, db = K.conv3d_head_d2_bwd_weight_f32(xd, dy.to(device), None, tuple(wt.shape))
    assert tuple(dw.shape) == tuple(wt.shape)
    assert _rel(dw, w64.grad) <= NORM_TOL and _rel(db, b64.grad) <= NORM_TOL


# ---- 3. refusals before any launch -------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    import ctypes
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(ValueError, match="C_in, C_out"):                         # unsupported channel pair
        K.conv3d_wide_fwd_f32(z(1, 32, 3, 8, 8), z(128, 32, 2, 3, 3), z(128))
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.conv3d_wide_bwd_data_f32(z(1, 64, 2, 8, 8), None, z(64, 128, 2, 3, 3), None, (1, 128, 3, 8, 8))
    with pytest.raises(ValueError, match="padding"):                             # depth padding 2
        K.conv3d_wide_fwd_f32(z(1, 64, 3, 8, 8), z(128, 64, 2, 3, 3), z(128), padding=(2, 1, 1))
    with pytest.raises(ValueError, match="padding"):                             # spatial padding other than 1
        K.conv3d_wide_fwd_f32(z(1, 64, 3, 8, 8), z(128, 64, 2, 3, 3), z(128), padding=(0, 0, 0))
    with pytest.raises(ValueError, match="128"):                                 # 129 columns
        K.conv3d_wide_fwd_f32(z(1, 64, 3, 8, 129), z(128, 64, 2, 3, 3), z(128))
    with pytest.raises(ValueError, match="one slice"):                           # depth 1 without depth padding
        K.conv3d_wide_fwd_f32(z(1, 64, 1, 8, 8), z(128, 64, 2, 3, 3), z(128))
    with pytest.raises(ValueError, match="horizon"):
        K.conv3d_wide_horizon_fwd_f32(z(2, 4, 8, 8), z(3), z(64, 2, 2, 3, 3), z(64))
    with pytest.raises(ValueError, match="depth 2"):                             # the head's view at depth 3
        K.conv3d_head_d2_fwd_f32(z(1, 128, 3, 8, 8), z(1, 128, 2, 3, 3), z(1))
    with pytest.raises(ValueError, match="depth 2"):
        K.conv3d_head_d2_bwd_weight_f32(z(1, 128, 3, 8, 8), z(1, 1, 1, 4, 4), None, (1, 128, 2, 3, 3))
    with pytest.raises(RuntimeError, match="status -1"):                         # the head takes no dy_gate
        K.conv2d_head_s2p1_bwd_data_f32(z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 32, 3, 3), None, (1, 32, 8, 8))
    # the ABI itself, from device pointers: the error code, nothing launched
    lib = _lib.get_lib()
    x, wt, y = z(1, 64, 3, 8, 8), z(128, 64, 2, 3, 3), torch.full((1, 128, 2, 8, 8), 7.0, device=device)
    fwd = lib.pv_conv3d_wide_fwd_f32
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 32, 128, 3, 8, 8, 0, 1, 0, None) == -2      # channel pair
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 64, 64, 3, 8, 8, 0, 1, 0, None) == -2
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 3, 8, 8, 2, 1, 0, None) == -2      # depth padding 2
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 3, 8, 8, 0, 0, 0, None) == -2      # spatial padding 0
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 3, 8, 8, 0, 2, 0, None) == -2      # spatial padding 2
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 3, 8, 129, 0, 1, 0, None) == -2    # 129 columns
    assert fwd(ptr(x), ptr(wt), None, ptr(y), 1, 64, 128, 1, 8, 8, 0, 1, 0, None) == -2      # depth 1, no depth padding
    assert "depth" in lib.pv_last_error().decode()
    assert fwd(ptr(x), None, None, ptr(y), 1, 64, 128, 3, 8, 8, 0, 1, 0, None) == -1         # null pointer
    assert lib.pv_conv3d_wide_bwd_data_f32(ptr(y), None, ptr(wt), ptr(y), None, 1, 64, 128, 3, 8, 8, 2, 1, None) == -2
    assert lib.pv_conv3d_wide_horizon_fwd_f32(ptr(x), ptr(x), ptr(wt), ptr(wt), ptr(y), 1, 3, 8, 8, 128, None) == -2
    assert lib.pv_conv3d_wide_horizon_fwd_f32(ptr(x), None, ptr(wt), ptr(wt), ptr(y), 1, 3, 8, 8, 64, None) == -1
    assert lib.pv_conv2d_head_s2p1_fwd_f32(ptr(x), ptr(wt), None, ptr(y), 1, 64, 2, 8, 8, 0, None) == -2
    torch.cuda.synchronize()
    assert (y == 7.0).all(), "a refused call wrote its output"
    need = ctypes.c_size_t(0)
    assert lib.pv_conv3d_wide_bwd_weight_workspace_bytes(1, 64, 128, 3, 8, 8, 0, 1, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv3d_wide_bwd_weight_workspace_bytes(1, 64, 128, 3, 8, 8, 2, 1, ctypes.byref(need)) == -2
    dw, db, ws = z(128, 64, 2, 3, 3), z(128), z(1 << 20)
    assert lib.pv_conv3d_wide_bwd_weight_workspace_bytes(1, 64, 128, 3, 8, 8, 0, 1, ctypes.byref(need)) == 0
    assert lib.pv_conv3d_wide_bwd_weight_f32(ptr(x), ptr(y), None, ptr(dw), ptr(db), 1, 64, 128, 3, 8, 8, 0, 1, ptr(ws),
                                             need.value - 1, None) == -1
    assert "workspace" in lib.pv_last_error().decode()
    assert lib.pv_conv2d_head_s2p1_bwd_weight_workspace_bytes(1, 256, 1, 8, 8, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_head_s2p1_bwd_weight_f32(ptr(x), ptr(y), None, ptr(dw), ptr(db), 1, 256, 1, 8, 8, ptr(ws),
                                                  need.value - 1, None) == -1
    torch.cuda.synchronize()
    assert (dw == 0).all() and (db == 0).all(), "a refused call wrote its output"
