"""GPU: the strided depth-2 Conv3d encoder and the horizon ConvTranspose2d of notebooks/08_multiple_historical_images_as_
separate_channels.ipynb (csrc/conv3d_s2_f32.hip, conv3d_wide_functional, models/conv3d/nb08_hist_depth.py) against float64
on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  The shapes, references and assertions of the
conv3d_s2 family's three passes and of the horizon ConvTranspose2d are tests/conv_family_checks.py's: one record and one
checker for every plain f32 conv family, float64 autograd through the reference op.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
from conv2d_f32_helpers import _ops, _to, _within
from notebook_model_checks import CASES, _g, _randn

pytestmark = pytest.mark.gpu

STRIDE = (1, 2, 2)


def _out(s):
    return (s - 3) // 2 + 1


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of("conv3d_s2", ids="{shape}-{c_in}-{c_out}")
def test_conv3d_s2_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


@C.twin_shapes("convt2d_s2_horizon")
def test_horizon_conv_transpose_against_float64(device, twin, shape):
    C.check_horizon_conv_transpose(_ops(), device, twin, shape)


# ---- 1. Conv3d (2, 3, 3), stride (1, 2, 2): no data gradient at the first layer --------------------------------------------
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


# ---- 3. refusals through the Python surface ----------------------------------------------------------------------------
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
