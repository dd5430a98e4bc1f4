"""GPU: the per-frame Conv2d stack and convolution over time of notebooks/11_just_conv_and_conv_over_time.ipynb
(csrc/conv2d_ae_f32.hip: the frame-stripe first layer and the padded 32 -> 32 layer; csrc/conv_time_f32.hip; conv2d_functional,
models/conv2d/nb11_conv_over_time.py) against float64 on the CPU (tests/nb11_reference.py).

The padded layer's three passes run through the one checker of tests/conv_family_checks.py on a record built here (it is not
in the shared table); the model-level checks are notebook_model_checks.py's on a record built here as well.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
import nb11_reference as R
import notebook_model_checks as N
from conv2d_f32_helpers import ELEM_TOL, NORM_TOL, _ops, _rel, _within
from nb10_reference import STRIPE_WIDTH, stripe_plane64

pytestmark = pytest.mark.gpu


# ---- 1. the first layer: Conv2d 2 -> 16 on every frame, the stripe plane as the second channel ---------------------------
FIRST_SHAPES = [(1, 3, 3, 4), (2, 4, 4, 4), (3, 7, 12, 4), (2, 26, 26, 4), (2, 5, 128, 4), (3, 7, 12, 1)]      # (n, H, W, frames)


def first_layer_input64(hist, starts):
    """[F N, 2, H, W] float64, built image by image: image F b + f = (frame f of example b, the stripe plane of example b)."""
    n, frames, h, w = hist.shape
    planes = stripe_plane64(starts, h, w)
    x = torch.zeros(n * frames, 2, h, w, dtype=torch.float64)
    for b in range(n):
        for f in range(frames):
            x[frames * b + f, 0] = hist[b, f].double()
            x[frames * b + f, 1] = planes[b, 0]
    return x


@pytest.mark.parametrize("n, h, w, frames", FIRST_SHAPES, ids=lambda v: str(v))
def test_frame_stripe_layer_against_float64(device, n, h, w, frames):
    """Stripe starts per example rotate through: inside the image, straddling the right edge, at W, beyond W, negative and
    straddling column 0, and column 0; one round has every example's plane empty, where dw[:, 1] must be exactly 0."""
    K = _ops()
    g = N._g(1100 + 7 * w + h + frames)
    hist = N._randn(g, n, frames, h, w)
    wt, b = C._conv_params(g, 16, 2)
    dy = N._randn(g, n * frames, 16, h - 2, w - 2)
    hd, wd, bd, dyd = hist.to(device), wt.to(device), b.to(device), dy.to(device)
    pool = [w // 2 - 2, w - 2, w, w + 3, -3, 0]
    rounds = [[pool[(k + i) % len(pool)] for i in range(n)] for k in range(len(pool))] + [[w + i for i in range(n)]]
    for starts in rounds:
        st = torch.tensor(starts, dtype=torch.int32)
        sd = st.to(device)
        x64 = first_layer_input64(hist, st)
        if frames == 4:      # the order the model folds its frames in: image 4 b + f is frame f of example b
            horizon_free = R.input_frames(hist, torch.zeros(n))[:, 0]
            assert all(torch.equal(x64[4 * bi + f, 0], hist[bi, f].double()) for bi in range(n) for f in range(4))
            assert torch.equal(x64[:, 0], horizon_free)
        dw = C.check_first_layer(lambda: K.conv2d_ae_frame_stripe_fwd_f32(hd, sd, wd, bd, STRIPE_WIDTH),
                                 lambda: K.conv2d_ae_frame_stripe_bwd_weight_f32(hd, sd, dyd, tuple(wt.shape), STRIPE_WIDTH),
                                 x64, wt, b, dy, {}, f"frame stripe starts {starts}")
        w64 = wt.double().requires_grad_(True)
        dw64, = torch.autograd.grad(F.conv2d(x64, w64), (w64,), dy.double())
        C._norm(dw[:, 0], dw64[:, 0], f"starts {starts}: dw of the frame channel")
        if float(x64[:, 1].sum()) == 0:      # every plane empty: the stripe channel's gradient is exact zeros
            assert (dw[:, 1] == 0).all(), "the gradient of an empty stripe plane's channel is not exactly 0"
        else:
            C._norm(dw[:, 1], dw64[:, 1], f"starts {starts}: dw of the stripe channel")
    # a stripe of width 0 is an empty plane whatever its start
    y0 = K.conv2d_ae_frame_stripe_fwd_f32(hd, torch.zeros(n, dtype=torch.int32, device=device), wd, bd, 0)
    pre = F.conv2d(first_layer_input64(hist, torch.full((n,), w)), wt.double(), b.double())
    absref = F.conv2d(first_layer_input64(hist, torch.full((n,), w)).abs(), wt.double().abs(), b.double().abs())
    _within(y0, pre.relu(), absref, what="stripe width 0")


# ---- 2. the padded 32 -> 32 layer: conv2d_ae_*(padding=2) -----------------------------------------------------------------
# one output; non-square; two row bands of the forward (19 rows of 35 columns) and two column tiles; 126 columns out; two row
# bands at one column band in every pass (32 rows of 22 columns)
P2 = C.Family("conv2d_ae_p2", F.conv2d, {"padding": 2}, (3, 3), ((32, 32),),
              ((1, 1, 1), (2, 3, 5), (1, 17, 33), (2, 8, 124), (2, 30, 20)),
              lambda ci, co, n, h, w: 1100 + 7 * w + h, stem="conv2d_ae", kwargs={"padding": 2}, gates=C.ALL_GATES,
              x_is_relu_output=True)


@pytest.mark.parametrize("shape", P2.shapes, ids=lambda s: "-".join(map(str, s)))
def test_padded_conv_against_float64(device, shape):
    C.check_family(_ops(), device, P2, 32, 32, shape)


@pytest.mark.parametrize("shape", P2.shapes, ids=lambda s: "-".join(map(str, s)))
def test_padded_conv_is_the_conv_transpose_on_the_flipped_transposed_weight(device, shape):
    """conv2d(x, w, padding=2) == conv_transpose2d(x, w.flip(2, 3).transpose(0, 1)): both entry points against the same
    float64 pre-activation within ELEM_TOL of its sum of |products|; the padded one makes no such weight copy."""
    K = _ops()
    g, x, w, b = C.draw_case(P2, 32, 32, shape)
    pre = F.conv2d(x.double(), w.double(), b.double(), padding=2)
    absref = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=2)
    xd, bd = x.to(device), b.to(device)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    assert _rel(F.conv_transpose2d(x.double(), wt.double(), b.double()), pre) <= 1e-12
    _within(K.conv2d_ae_fwd_f32(xd, w.to(device), bd, relu=False, padding=2), pre, absref, what="padded conv")
    _within(K.convt2d_ae_fwd_f32(xd, wt.to(device), bd, relu=False), pre, absref, what="conv transpose")


# ---- 3. the convolution over time ---------------------------------------------------------------------------------------------
BLOCK = 256      # pixels of a block of pv_conv_time_*
# one pixel; a block's pixels less one, exactly, plus one; three slabs of the parameter-gradient sum; example boundaries
# inside a wave (B = 3, P odd); more 256-pixel chunks than slabs (514 > 512: two chunks per block)
# (B, P, seed): the first seed from 1100 up whose float64 hidden pre-activations all lie at least 2e-4 from 0
HEAD_CASES = [(1, 1, 1100), (1, BLOCK - 1, 1100), (1, BLOCK, 1100), (1, BLOCK + 1, 1100), (1, 700, 1101), (3, 85, 1100),
              (1, 513 * BLOCK + 1, 1100)]
N_PATTERNS = 23
GATE_MARGIN = 1e-4
PARAM_NAMES = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")


def head_case(b, p, seed):
    """u [4 B, 1, 1, P] (ReLU outputs: non-negative, a third exact zeros), dy [B, 1, 1, P] and the six parameters.  The pixels
    take their four frame values from N_PATTERNS drawn patterns in a scrambled order: the hidden pre-activations depend on
    the pattern alone, so that every one of them can be held clear of 0 whatever B P is (with B P independent pixels of 80
    units each, about 1.6e-4 B P 80 of them would lie within 1e-4 of 0 and no seed could avoid it)."""
    g = N._g(seed)
    base = N._randn(g, N_PATTERNS, 4).relu() * (torch.rand(N_PATTERNS, 4, generator=g) > 1 / 3)
    which = (torch.arange(b * p) * 7 + 3) % N_PATTERNS
    u = base[which].reshape(b, p, 4).permute(0, 2, 1).reshape(4 * b, 1, 1, p).contiguous()
    dy = N._randn(g, b, 1, 1, p)
    shapes = R.G.PARAM_SHAPES
    params = {k: N._randn(g, *shapes[f"temporal_conv.{k}"], scale=0.5 if k.endswith("weight") else 0.2) for k in PARAM_NAMES}
    return u, dy, params


def head_float64(u, dy, params, absolute=False):
    """(y, du, the six parameter gradients, the two hidden pre-activations) of temporal_conv in float64.  absolute: the
    all-absolute-values network -- |u|, |parameters|, |dy|, no ReLU -- whose y and du are each element's sum of |products|."""
    fix = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    p64 = {f"temporal_conv.{k}": fix(v).requires_grad_(True) for k, v in params.items()}
    u64 = fix(u).requires_grad_(True)
    t = R.time_image(u64)
    if absolute:
        z1 = F.conv2d(t, p64["temporal_conv.0.weight"], p64["temporal_conv.0.bias"])
        z2 = F.conv2d(z1, p64["temporal_conv.2.weight"], p64["temporal_conv.2.bias"])
        out, hidden = F.conv2d(z2, p64["temporal_conv.4.weight"], p64["temporal_conv.4.bias"]), (z1, z2)
    else:
        out, hidden = R.temporal_layers(p64, t)
    y = out.reshape(dy.shape)
    grads = torch.autograd.grad(y, [u64] + list(p64.values()), fix(dy))
    return y.detach(), grads[0], dict(zip(PARAM_NAMES, grads[1:])), [h.detach() for h in hidden]


def head_float32_yardstick(u, dy, params):
    """The same three layers in float32 torch on the CPU: (y, du)."""
    p32 = {f"temporal_conv.{k}": v.clone().requires_grad_(True) for k, v in params.items()}
    u32 = u.clone().requires_grad_(True)
    y = R.temporal_layers(p32, R.time_image(u32))[0].reshape(dy.shape)
    du, = torch.autograd.grad(y, [u32], dy)
    return y.detach(), du


@pytest.mark.parametrize("b, p, seed", HEAD_CASES, ids=lambda v: str(v))
def test_conv_over_time_against_float64(device, b, p, seed):
    """Forward, du (plain, and gated by u > 0) and each of the six parameter gradients against float64; two backward calls give
    identical bits.

    Tolerance: the project's ELEM_TOL = 1e-6 per element of y and du, relative to the element's sum of |products| through the
    all-absolute-values network (|u|, |parameters|, |dy|, no ReLU), and NORM_TOL = 1e-5 relative norm for each parameter
    gradient, a sum over B P pixels.  The yardstick -- float32 torch on the CPU for the same three layers and inputs -- measured
    over these seven cases: its largest error is 9.5e-7 in y and 5.4e-6 in du, which is 0.014 and 0.035 of the ELEM_TOL bound
    (the test prints both per case).  ELEM_TOL against the all-absolute-values network holds for the kernels, so it is the
    bound asserted, on every element, in place of 4 x the yardstick.

    The backward gates by its own recomputed hidden layers, so the float64 reference must have no hidden pre-activation
    within 1e-4 of 0 (asserted; the seeds are chosen for it on the CPU) and no element is skipped."""
    K = _ops()
    u, dy, params = head_case(b, p, seed)
    y64, du64, g64, hidden = head_float64(u, dy, params)
    closest = min(h.abs().min().item() for h in hidden)
    assert closest >= GATE_MARGIN, f"a hidden pre-activation at {closest:.2e} of 0: draw another seed"
    absy, absdu, _, _ = head_float64(u, dy, params, absolute=True)
    y32, du32 = head_float32_yardstick(u, dy, params)
    for what, got, ref, scale in (("y", y32, y64, absy), ("du", du32, du64, absdu)):
        print(f"yardstick {what}: {((got.double() - ref).abs() / (ELEM_TOL * scale + 1e-30)).max().item():.3f} x the bound")
    ud, dyd = u.to(device), dy.to(device)
    pd = [params[k].to(device) for k in PARAM_NAMES]
    y = K.conv_time_fwd_f32(ud, *pd)
    assert tuple(y.shape) == (b, 1, 1, p)
    du, *grads = K.conv_time_bwd_f32(ud, dyd, *pd[:5])
    assert tuple(du.shape) == tuple(u.shape)
    for what, got, ref, scale in (("y", y, y64, absy), ("du", du, du64, absdu)):
        print(f"{what}: {((got.double().cpu() - ref).abs() / (ELEM_TOL * scale + 1e-30)).max().item():.3f} x the bound")
    _within(y, y64, absy, what="y")
    _within(du, du64, absdu, what="du")
    for k, got in zip(PARAM_NAMES, grads):
        assert tuple(got.shape) == tuple(params[k].shape)
        C._norm(got, g64[k], f"temporal_conv.{k} gradient")
    again = K.conv_time_bwd_f32(ud, dyd, *pd[:5])
    C._same_bits((du, *grads), again, "du and the parameter gradients")
    # u as a ReLU's output (a third of it exact zeros): du zeroed there, the parameter gradients the same bits
    gated = K.conv_time_bwd_f32(ud, dyd, *pd[:5], u_is_relu_output=True)
    _within(gated[0], du64 * (u > 0), absdu, what="du gated by u > 0")
    assert (gated[0][ud == 0] == 0).all() and (u == 0).any()
    C._same_bits(tuple(grads), gated[1:], "the parameter gradients with and without the gate on du")
    assert torch.equal(y, K.conv_time_fwd_f32(ud, *pd))


def test_conv_over_time_reads_the_heads_output_in_place(device):
    """u as the model has it, [4 B, 1, s1, s2] with image 4 b + f: pixel p of example b mixes images 4 b .. 4 b + 3."""
    K = _ops()
    u, dy, params = head_case(2, 35, 1101)
    u, dy = u.reshape(8, 1, 5, 7), dy.reshape(2, 1, 5, 7)
    y64, *_ = head_float64(u, dy, params)
    absy, *_ = head_float64(u, dy, params, absolute=True)
    y = K.conv_time_fwd_f32(u.to(device), *(params[k].to(device) for k in PARAM_NAMES))
    assert tuple(y.shape) == (2, 1, 5, 7)
    _within(y, y64, absy, what="y")


# ---- 4. refusals, through Python and through the C ABI, before any launch --------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    from predict_pv_yield_amd import _lib
    from predict_pv_yield_amd.hip_ops import ptr
    K = _ops()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, device=device, dtype=dtype)      # noqa: E731
    zi = lambda n: torch.zeros(n, device=device, dtype=torch.int32)      # noqa: E731
    with pytest.raises(ValueError, match="128 columns"):                         # width 130
        K.conv2d_ae_frame_stripe_fwd_f32(z(1, 4, 8, 130), zi(1), z(16, 2, 3, 3), z(16), 5)
    with pytest.raises(ValueError, match="128 columns"):                         # 127 + 2 columns out
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 127), z(32, 32, 3, 3), z(32), padding=2)
    with pytest.raises(ValueError, match="C_in, C_out"):                         # wrong channel pairs
        K.conv2d_ae_fwd_f32(z(1, 16, 8, 8), z(32, 16, 3, 3), z(32), padding=2)
    with pytest.raises(ValueError, match="C_in, C_out"):
        K.conv2d_ae_bwd_data_f32(z(1, 16, 10, 10), None, z(16, 32, 3, 3), None, (1, 32, 8, 8), padding=2)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d_ae_frame_stripe_fwd_f32(z(2, 4, 8, 8), zi(2), z(32, 2, 3, 3), z(32), 5)
    with pytest.raises(ValueError, match="parameters"):
        K.conv_time_fwd_f32(z(8, 1, 3, 3), z(32, 1, 1, 2), z(32), z(16, 32, 1, 2), z(16), z(1, 16, 1, 2), z(1))
    with pytest.raises(ValueError, match="stripe_start"):                        # a horizon of the wrong length
        K.conv2d_ae_frame_stripe_fwd_f32(z(2, 4, 8, 8), zi(3), z(16, 2, 3, 3), z(16), 5)
    with pytest.raises(ValueError, match="stripe_start"):
        K.conv2d_ae_frame_stripe_bwd_weight_f32(z(2, 4, 8, 8), zi(1), z(8, 16, 6, 6), (16, 2, 3, 3), 5)
    with pytest.raises(TypeError, match="float32"):                              # a float64 tensor
        K.conv2d_ae_frame_stripe_fwd_f32(z(2, 4, 8, 8, dtype=torch.float64), zi(2), z(16, 2, 3, 3), z(16), 5)
    with pytest.raises(TypeError, match="float32"):
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 8), z(32, 32, 3, 3, dtype=torch.float64), z(32), padding=2)
    with pytest.raises(TypeError, match="float32"):
        K.conv_time_fwd_f32(z(8, 1, 3, 3, dtype=torch.float64), z(16, 1, 1, 2), z(16), z(16, 16, 1, 2), z(16), z(1, 16, 1, 2), z(1))
    with pytest.raises(ValueError, match="padding"):
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 8), z(32, 32, 3, 3), z(32), padding=1)
    # the ABI itself, from device pointers: the error code, the outputs untouched
    lib = _lib.get_lib()
    need = ctypes.c_size_t(0)
    hist, st, wt, bias = z(2, 4, 8, 8), zi(2), z(16, 2, 3, 3), z(16)
    y = torch.full((8, 16, 6, 6), 7.0, device=device)
    dw, db, ws = torch.full((16, 2, 3, 3), 7.0, device=device), torch.full((16,), 7.0, device=device), z(1 << 16)
    assert lib.pv_conv2d_ae_frame_stripe_fwd_f32(ptr(hist), ptr(st), ptr(wt), ptr(bias), ptr(y), 2, 4, 8, 130, 16, 5, None) == -2
    assert lib.pv_conv2d_ae_frame_stripe_fwd_f32(ptr(hist), ptr(st), ptr(wt), ptr(bias), ptr(y), 2, 4, 8, 8, 64, 5, None) == -2
    assert lib.pv_conv2d_ae_frame_stripe_fwd_f32(ptr(hist), ptr(st), ptr(wt), ptr(bias), ptr(y), 2, 8, 8, 8, 16, 5, None) == -2
    assert lib.pv_conv2d_ae_frame_stripe_bwd_weight_workspace_bytes(2, 4, 8, 8, ctypes.byref(need)) == 0 and 0 < need.value <= 1 << 18
    assert lib.pv_conv2d_ae_frame_stripe_bwd_weight_f32(ptr(hist), ptr(st), ptr(y), ptr(dw), ptr(db), 2, 4, 8, 8, 16, 5, ptr(ws),
                                                        need.value - 1, None) == -1
    x, w32 = z(1, 32, 8, 8), z(32, 32, 3, 3)
    y2 = torch.full((1, 32, 10, 10), 7.0, device=device)
    dw2, db2 = torch.full((32, 32, 3, 3), 7.0, device=device), torch.full((32,), 7.0, device=device)
    assert lib.pv_conv2d_ae_p2_fwd_f32(ptr(x), ptr(w32), None, ptr(y2), 1, 16, 32, 8, 8, 0, None) == -2
    assert lib.pv_conv2d_ae_p2_fwd_f32(ptr(x), ptr(w32), None, ptr(y2), 1, 32, 32, 8, 128, 0, None) == -2
    assert lib.pv_conv2d_ae_p2_bwd_weight_workspace_bytes(1, 32, 32, 8, 8, ctypes.byref(need)) == 0 and 0 < need.value <= 1 << 18
    assert lib.pv_conv2d_ae_p2_bwd_weight_f32(ptr(x), ptr(y2), None, ptr(dw2), ptr(db2), 1, 32, 32, 8, 8, ptr(ws), need.value - 1,
                                              None) == -1
    u, dyt = z(8, 1, 3, 3), z(2, 1, 3, 3)
    tp = [z(*s) for s in K.TIME_PARAM_SHAPES]
    yt, du = torch.full((2, 1, 3, 3), 7.0, device=device), torch.full((8, 1, 3, 3), 7.0, device=device)
    tg = [torch.full(s, 7.0, device=device) for s in K.TIME_PARAM_SHAPES]
    assert lib.pv_conv_time_fwd_f32(ptr(u), *(ptr(t) for t in tp), ptr(yt), 2, 3, 16, 9, None) == -2
    assert lib.pv_conv_time_fwd_f32(ptr(u), *(ptr(t) for t in tp), ptr(yt), 2, 4, 32, 9, None) == -2
    assert lib.pv_conv_time_bwd_workspace_bytes(2, 4, 16, 9, ctypes.byref(need)) == 0 and need.value == 609 * 4
    assert lib.pv_conv_time_bwd_f32(ptr(u), ptr(dyt), *(ptr(t) for t in tp[:5]), ptr(du), *(ptr(t) for t in tg), 2, 4, 16, 9,
                                    1, ptr(ws), need.value - 1, None) == -1
    torch.cuda.synchronize()
    for t in (y, dw, db, y2, dw2, db2, yt, du, *tg):
        assert (t == 7.0).all()


# ---- 5. the model ---------------------------------------------------------------------------------------------------------------
CASE = N.Case("nb11", N.M2 + "nb11_conv_over_time", N._stripe_batch(N._half), ((2, 128, (2, 1, 64, 64)),), 3, lr=1e-4,
              horizons=(7.9, 25.0), batch_of_one=(21, (1, 1, 11, 11)), deterministic="drawn",
              datamodule="nb10_datamodule:Nb10DataModule", dm_args=N.DM2, graph_fit_extra=2)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_against_golden(device, tag):
    N.check_model_against_golden(device, CASE, tag)


def test_full_size_forward_and_loss(device):
    for b, s, shape in CASE.full_sizes:
        N.check_full_size_forward_and_loss(device, CASE, b, s, shape)


def test_batch_of_one(device):
    N.check_batch_of_one(device, CASE)


def test_two_eager_runs_are_equal_bit_for_bit(device):
    N.check_two_eager_runs_are_equal_bit_for_bit(device, CASE)


def test_train_step_replays_as_a_hip_graph(device):
    N.check_train_step_replays_as_a_hip_graph(device, CASE)


def test_trainer_fit_with_hip_graph_matches_the_eager_fit(device):
    N.check_trainer_fit_with_hip_graph_matches_the_eager_fit(device, CASE)
