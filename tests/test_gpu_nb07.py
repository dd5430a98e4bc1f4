"""GPU: the weight-shared per-frame encoder's first layer and the one-frame identity of the 128 -> 32 ConvTranspose2d of
notebooks/07_multiple_historical_images.ipynb (csrc/conv2d_frames_f32.hip, conv2d_functional,
models/conv2d/nb07_multi_hist.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  The references are float64 F.conv2d on the
explicitly built [F B, 2, H, W] input, torch.nn.grad.conv2d_weight and F.conv_transpose2d.

The three passes of convt2d_s2_frames are checked below by the records
and the one checker of tests/conv_family_checks.py.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import nb07_reference as R
import conv_family_checks as C
from conv2d_f32_helpers import NORM_TOL, _ops, _rel, _to, _within
from notebook_model_checks import CASES, _g, _randn
from predict_pv_yield_amd.models.conv2d.nb07_multi_hist import LitAutoEncoder      # absent: the file fails at import

pytestmark = pytest.mark.gpu

# (batch, height, width) of the history frames: one output; an unread row and column; odd and even sides; one block of nine
# 16-position tiles over its four waves; the model's second size, the only one whose forward takes several row bands (31
# rows of outputs as 16 + 15); full width, 7 x 63 outputs: one block in the forward, two row bands (the 384-position limit) in
# the weight gradient
FIRST_SHAPES = [(1, 3, 3), (2, 4, 4), (3, 7, 12), (2, 26, 26), (1, 63, 63), (2, 15, 128)]
HORIZONS = [0.0, -1.3, 0.7]                 # per example distinct: zero and both signs


def _out(s):
    return (s - 3) // 2 + 1


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of("convt2d_s2_frames", ids="{shape}")
def test_frames_conv_transpose_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- 1. the first layer: every frame with the horizon as a second channel, folded into the batch -------------------------
def _first_layer(device, n, frames, h, w, horizon, seed):
    K = _ops()
    g = _g(seed)
    history = _randn(g, n, frames, h, w)
    wt, b = _randn(g, 32, 2, 3, 3, scale=18 ** -0.5), _randn(g, 32, scale=0.1)
    x64 = R.folded_input64(history, horizon)
    assert tuple(x64.shape) == (n * frames, 2, h, w)
    for i in range(n * frames):       # image F b + f: frame f of example b, then that example's horizon
        assert torch.equal(x64[i, 0], history[i // frames, i % frames].double()) and (x64[i, 1] == horizon[i // frames].double()).all()
    w64, b64 = wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64, stride=2)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    assert tuple(pre.shape) == (n * frames, 32, _out(h), _out(w))
    hd, zd, wd, bd = history.to(device), horizon.to(device), wt.to(device), b.to(device)
    y = K.conv2d_s2_frame_horizon_fwd_f32(hd, zd, wd, bd, relu=True)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_s2_frame_horizon_fwd_f32(hd, zd, wd, bd, relu=False), pre, absref, what="forward without relu")
    _within(K.conv2d_s2_frame_horizon_fwd_f32(hd, zd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref,
            what="forward without bias")
    dy, dy_gate = _randn(g, *pre.shape), _randn(g, *pre.shape)
    for use_dg in (True, False):
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        dw, db = K.conv2d_s2_frame_horizon_bwd_weight_f32(hd, zd, dy.to(device), (32, 2, 3, 3),
                                                          dy_gate=dy_gate.to(device) if use_dg else None)
        assert tuple(dw.shape) == (32, 2, 3, 3) and tuple(db.shape) == (32,)
        dw64 = torch.nn.grad.conv2d_weight(x64, (32, 2, 3, 3), dyg, stride=2)
        for ch, what in ((0, "history channel"), (1, "horizon channel")):      # each on its own: neither hides in the other's norm
            if ch == 1 and not horizon.any():
                assert (dw[:, 1] == 0).all(), "all horizons 0: the horizon channel's gradient is exactly 0"
                continue
            err = _rel(dw[:, ch], dw64[:, ch])
            assert err <= NORM_TOL, (use_dg, what, err)
        assert _rel(db, dyg.sum((0, 2, 3))) <= NORM_TOL


@pytest.mark.parametrize("n, h, w", FIRST_SHAPES)
def test_first_layer_against_float64(device, n, h, w):
    _first_layer(device, n, 4, h, w, torch.tensor(HORIZONS[:n]) if n > 1 else torch.tensor([-0.4]), 700 + w + h)


def test_first_layer_with_one_frame(device):
    _first_layer(device, 3, 1, 7, 12, torch.tensor(HORIZONS), 731)


def test_first_layer_with_all_horizons_zero(device):
    """dw[:, 1] is exactly 0, and the history channel's gradient is unchanged by it."""
    _first_layer(device, 3, 4, 7, 12, torch.zeros(3), 732)


# ---- 2. ConvTranspose2d 128 -> 32 along the frame seam -------------------------------------------------------------------
@pytest.mark.parametrize("f", range(4))
def test_frames_conv_transpose_of_one_frame_is_the_32_channel_layer(device, f):
    """x nonzero in frame f only: the forward is pv_convt2d_s2_fwd_f32 on that slice and weight slice (the other frames'
    passes add exact zeros)."""
    K = _ops()
    g = _g(1200 + f)
    n, h, w = 2, 7, 7
    rows = slice(32 * f, 32 * f + 32)
    x = torch.zeros(n, 128, h, w)
    x[:, rows] = _randn(g, n, 32, h, w)
    wt, b = _randn(g, 128, 32, 3, 3, scale=(9 * 128) ** -0.5), _randn(g, 32, scale=0.1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.convt2d_s2_frames_fwd_f32(xd, wd, bd, relu=False)
    one = K.convt2d_s2_fwd_f32(xd[:, rows].contiguous(), wd[rows].contiguous(), bd, relu=False)
    x64, w64, b64 = x.double()[:, rows], wt.double()[rows], b.double()
    absref = F.conv_transpose2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    _within(y, one.double().cpu(), absref, what=f"frame {f} against the 32 -> 32 layer")
    _within(y, F.conv_transpose2d(x64, w64, b64, stride=2), absref, what=f"frame {f} against float64")


# ---- 3. refusals through the Python surface ----------------------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    import ctypes
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(ValueError, match="128 columns"):                       # widths beyond the limit
        K.conv2d_s2_frame_horizon_fwd_f32(z(1, 4, 8, 130), z(1), z(32, 2, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        K.convt2d_s2_frames_fwd_f32(z(1, 128, 8, 64), z(128, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="x \\[N, 128"):                       # wrong channel pairs
        K.convt2d_s2_frames_fwd_f32(z(1, 32, 8, 8), z(32, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="weight \\[32, 2, 3, 3\\]"):
        K.conv2d_s2_frame_horizon_fwd_f32(z(1, 4, 8, 8), z(1), z(32, 6, 3, 3), z(32))
    with pytest.raises(ValueError, match="horizon"):
        K.conv2d_s2_frame_horizon_fwd_f32(z(2, 4, 8, 8), z(8), z(32, 2, 3, 3), z(32))
    with pytest.raises(TypeError):
        K.convt2d_s2_frames_fwd_f32(z(1, 128, 8, 8).double(), z(128, 32, 3, 3), z(32))
    with pytest.raises(TypeError):
        K.conv2d_s2_frame_horizon_fwd_f32(z(1, 4, 8, 8), z(1).double(), z(32, 2, 3, 3), z(32))
    model = LitAutoEncoder().to(device)
    good = _to(CASES["nb07"].full_batch(80, 2, 31), device)
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
    x, dy, dw, db, ws = z(2, 128, 7, 7), z(2, 32, 15, 15), z(128, 32, 3, 3), z(32), z(1 << 20)
    assert lib.pv_convt2d_s2_frames_fwd_f32(ptr(x), ptr(dw), ptr(db), ptr(dy), 2, 128, 32, 7, 64, 1, None) == -2
    assert lib.pv_convt2d_s2_frames_bwd_weight_workspace_bytes(2, 128, 32, 7, 7, ctypes.byref(need)) == 0 and 0 < need.value < 1 << 22
    dw.fill_(7.0)
    assert lib.pv_convt2d_s2_frames_bwd_weight_f32(ptr(x), ptr(dy), None, ptr(dw), ptr(db), 2, 128, 32, 7, 7, ptr(ws),
                                                   need.value - 1, None) == -1
    torch.cuda.synchronize()
    assert (dw == 7.0).all(), "nothing was launched"
