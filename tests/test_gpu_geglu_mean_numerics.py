"""The GEGLU and mean kernels -- csrc/perceiver_ops_f32.hip: geglu_{fwd,bwd}_f32, mean_axis1_{fwd,bwd}_f32 -- per element against
float64, at the element counts, widths and gates where they can go wrong, and CPU tests that show the checker rejects a kernel that
is subtly wrong.  Vocabulary and manner: tests/test_gpu_linear_numerics.py.

Reference (float64 on the CPU, on the float32 operands as the kernel receives them) and bounds, per element, never a norm
(`_check_terms`, through conv2d_f32_helpers._within): |c - c64| <= C 2^-24 S + the device functions' term.
GEGLU, x = (a | g), erf = erf(g / sqrt 2), pdf = exp(-g^2 / 2) / sqrt(2 pi):
    y     a 0.5 g (1 + erf)                        S = |a| 0.5 |g| (1 + |erf|)
    dx_a  d 0.5 g (1 + erf)                        S = |d| 0.5 |g| (1 + |erf|)
    dx_g  d a (0.5 (1 + erf) + g pdf)              S = |d a| (0.5 (1 + |erf|) + |g| pdf)
S does not cancel where 1 + erf does: at g = -5.5 erff returns -1 + 2^-24 or -1 and 1 + erff has lost its bits, but the result is
then of the order 2^-24 |a g| against a bound of 27 x 2^-24 |a g|: the bound holds and asks of such an element only that it be
about zero.
Mean over axis 1 of [b, n, d]: y = sum_j x / n with S = sum |x| / n; dx = dy / n with S = |dy| / n.

Constants.  From the REFERENCE's own error, never from the kernels: 4 x the worst error / (2^-24 S) of reference-only evaluations
over every case of this file -- float32 torch (a * F.gelu(g), x.mean(1), autograd) and the emulation of the source's order
(`_emu_geglu`: gelu_erf and gelu_erf_grad operation by operation with their constants narrowed to float32; `_emu_mean`:
mean_axis1_fwd_f32's index-order sum, then one division by (float) n, and dy / (float) n).  `python
tests/test_gpu_geglu_mean_numerics.py` prints the table:
    GEGLU      float32 torch   emulation   constant
    y              6.67          2.54        26.7
    dx_a           6.64          2.72        26.6
    dx_g           6.72          3.08        26.9
    (float32 torch's worst is one gate, g = 0.0211 at the models' width 256, where the CPU library's vectorised erf is about 7 x 2^-24
    off in absolute terms; the emulation, through torch.erf, is not)
    mean, n    forward: float32 torch / emulation   backward   constants (forward, backward)
    1             0.00 /  0.00                     0.00        0.0, 0.0     exact: 0 + x, x / 1
    2             0.99 /  0.99                     0.00        4.0, 0.0     a division by a power of two is exact
    9             1.84 /  2.09                     0.86        8.4, 3.5
    128           2.05 /  6.27                     0.00       25.1, 0.0
    1000          1.10 / 15.30                     0.78       61.2, 3.2
The mean's constant depends on n -- the kernel adds in index order, float32 torch pairwise -- so it is taken per n (C_MEAN).  A
constant 0.0 asks for the float64 value exactly (the 1e-30 of `_within` aside).

Device math functions.  erff and expf on the GPU are not the CPU's; their error is measured on the GPU through torch's own
elementwise erf and exp against float64, never through the kernels under test, over the arguments the cases produce (g / sqrt 2 and
-g^2 / 2 of every gate), and enters as the additive term F 2^-23 |function value| x the factor the value is multiplied by
(|a| 0.5 |g| for y, |d| 0.5 |g| for dx_a, 0.5 |d a| for erf and |d a g| for pdf in dx_g), F = 2 x the worst observed error in ulps
of the function value.  Measured on the MI355X over 22 089 gates: erf 0.820 ulps -> F_ERF = 1.65; exp 0.576 ulps on [-50, 0] ->
F_EXP = 1.16 (2 x the worst, rounded up to 0.01; far below 8, above which the file's premise would fail).
test_device_math_functions_are_within_F measures again and holds the constants to it.

Cases.  GEGLU (rows, h): (1, 1); (1, 255), (1, 256), (1, 257) either side of a 256-thread block; (3, 85), 255 elements with rows
crossing inside a block; (7, 37); (50, 96); 5 rows at the models' own h, read from the Perceiver's feed-forward (256).  Gates: a
shuffled sweep over [-9, 9], and in three plantings 0.0, -0.0, +-2^-126, +-1e-6, +-5.5 (above) and +-10 (expf(-50) sits near the
denormals) in the first and last column of the first and last row.  Mean (b, n, d): (1, 1, 1); (4, 9, 13); (3, 2, 100), b d = 300
crosses a block; (2, 1000, 7), the long index-order sum; (1, 128, the models' latent width that to_logits averages, 64); zero-mean
and all-positive inputs.  Both families: PF.geglu and PF.mean_axis1 against the direct calls, bitwise; every output of (7, 37) and
(4, 9, 13) inside a buffer filled with 1.2345678e30, handed over through the C ABI.

What the checker is sensitive to (CPU tests).  It accepts float32 torch and the emulation at every case, and rejects, applied to
ONE element of an otherwise correct float32 result: GEGLU with the tanh approximation of gelu (at the gate nearest 2, in y, dx_a
and dx_g); GEGLU reading the gate one column off (the same three); the mean dividing by n - 1 (y and dx, at n = 9, 2 and 1000).
What it cannot see: which of two bitwise-equal schedules ran; a read outside an operand whose value is discarded; the tanh
approximation at gates where it agrees with erf to within the bound (large |g|, and 0); a gate read one column off where the two gates
happen to be equal.

Measured on the MI355X with these constants, worst error / bound over all cases: GEGLU y 0.091, dx_a 0.083, dx_g 0.108; mean y 0.250
(the index-order sum at n = 1000, the emulation's own figure), dx 0.246.  Every bitwise relation held.  No case found a fault in the
kernels' results.  The 20 GPU cases take 3 s together (the first pays 1 s for loading the library); the 24 CPU cases take 3 s.
"""
import functools
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _ops, _within

U32 = 2.0 ** -24
ULP = 2.0 ** -23         # one unit in the last place of a float32 value, relative
SENTINEL = 1.2345678e30
GUARD = 64
TINY = 2.0 ** -126
RSQRT2 = 0.70710678118654752440
RSQRT2PI = 0.39894228040143267794

# 4 x the reference-only ratios printed by `python tests/test_gpu_geglu_mean_numerics.py` (module docstring)
C_GEGLU = {"y": 26.7, "dx_a": 26.6, "dx_g": 26.9}
C_MEAN = {1: (0.0, 0.0), 9: (8.4, 3.5), 2: (4.0, 0.0), 1000: (61.2, 3.2), 128: (25.1, 0.0)}      # n -> (forward, backward)
# 2 x the worst error of torch's own elementwise erf / exp on the MI355X, in ulps of the function value (module docstring)
F_ERF, F_EXP = 1.65, 1.16
F_MAX = 8.0

MODEL = "model"          # the width the Perceiver models use, read from their code (_model_widths)
GEGLU_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (3, 85), (7, 37), (50, 96), (5, MODEL)]      # (rows, h)
MEAN_SHAPES = [(1, 1, 1), (4, 9, 13), (3, 2, 100), (2, 1000, 7), (1, 128, MODEL)]                    # (b, n, d)
MEAN_REGIMES = ("zero_mean", "positive")
SPECIAL_GATES = [(0.0, -0.0, TINY, -TINY), (1e-6, -1e-6, 5.5, -5.5), (10.0, -10.0, 5.5, -0.0)]      # three plantings of four corners


@functools.lru_cache(maxsize=1)
def _model_widths():
    """(h of the Perceiver's feed-forward GEGLU, the width of the latents that to_logits averages) at the models' own defaults."""
    from predict_pv_yield_amd.models.perceiver.perceiver import PerceiverModel
    from predict_pv_yield_amd.models.perceiver.perceiver_core import FeedForward
    dim = inspect.signature(PerceiverModel.__init__).parameters["latent_dim"].default
    return FeedForward(dim).net[0].out_features // 2, dim


def _resolve(shape, which):
    return tuple(_model_widths()[which] if s == MODEL else s for s in shape)


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _d(x):
    return x.detach().double().cpu()


# ---- GEGLU: inputs, float64 reference, float32 evaluations -------------------------------------------------------------------------
class Geglu:
    """x [rows, 2 h] = (a | g): a ~ 2 randn, g a shuffled sweep over [-9, 9] with four special gates in the first and last column
    of the first and last row; dy ~ randn.  Float64: y = a gelu(g), dx_a = d gelu(g), dx_g = d a gelu'(g), and each one's S."""

    def __init__(self, rows, h, planting):
        g = torch.Generator().manual_seed(10007 * rows + 13 * h + planting)
        a = torch.randn(rows, h, generator=g) * 2
        gate = torch.linspace(-9.0, 9.0, rows * h)[torch.randperm(rows * h, generator=g)].view(rows, h)
        i = 0
        for r in sorted({0, rows - 1}):
            for c in sorted({0, h - 1}):
                gate[r, c] = SPECIAL_GATES[planting][i % 4]
                i += 1
        self.x, self.dy = torch.cat([a, gate], 1), torch.randn(rows, h, generator=g)
        self.rows, self.h = rows, h
        a, gt, d = a.double(), gate.double(), self.dy.double()
        erf, pdf = torch.erf(gt * RSQRT2), RSQRT2PI * torch.exp(-0.5 * gt * gt)
        half_g, cdf_abs = 0.5 * gt.abs(), 0.5 * (1 + erf.abs())
        gelu, dgelu = 0.5 * gt * (1 + erf), 0.5 * (1 + erf) + gt * pdf
        # the device functions' share: F 2^-23 |function value| x the factor the value is multiplied by
        e_erf, e_pdf = F_ERF * ULP * erf.abs(), F_EXP * ULP * pdf
        self.terms64 = {"y": (a * gelu, a.abs() * half_g * (1 + erf.abs()), a.abs() * half_g * e_erf),
                        "dx_a": (d * gelu, d.abs() * half_g * (1 + erf.abs()), d.abs() * half_g * e_erf),
                        "dx_g": (d * a * dgelu, (d * a).abs() * (cdf_abs + gt.abs() * pdf), (d * a).abs() * (0.5 * e_erf + gt.abs() * e_pdf))}
        self.gate = gate

    def terms(self, y, dx):
        dx = _d(dx)
        got = {"y": _d(y), "dx_a": dx[:, :self.h], "dx_g": dx[:, self.h:]}
        return {q: (got[q],) + self.terms64[q] for q in got}


@functools.lru_cache(maxsize=4)
def _geglu(rows, h, planting):
    return Geglu(rows, h, planting)


def _geglu32(P, how):
    """float32 -> (y, dx).  "torch": a * F.gelu(g) and autograd; "emulation": the source's operations in its order (gelu_erf,
    gelu_erf_grad); "tanh": the tanh approximation of gelu; "column_off": the gate read one column off."""
    if how in ("torch", "tanh"):
        x = P.x.clone().requires_grad_(True)
        a, g = x.chunk(2, dim=-1)
        y = a * F.gelu(g, approximate="tanh" if how == "tanh" else "none")
        y.backward(P.dy)
        return y.detach(), x.grad
    return _emu_geglu(P.x[:, :P.h], P.x[:, P.h:].roll(1, 1) if how == "column_off" else P.x[:, P.h:], P.dy)


def _emu_geglu(a, g, dy):
    """gelu_erf and gelu_erf_grad of the source, operation by operation in float32 (its constants narrowed to float32)."""
    cdf = 0.5 * (1.0 + torch.erf(g * RSQRT2))
    gelu = 0.5 * g * (1.0 + torch.erf(g * RSQRT2))
    pdf = RSQRT2PI * torch.exp(-0.5 * g * g)
    return a * gelu, torch.cat([dy * gelu, dy * a * (cdf + g * pdf)], 1)


# ---- mean over axis 1: inputs, float64 reference, float32 evaluations -------------------------------------------------------------
class Mean:
    def __init__(self, b, n, d, regime):
        g = torch.Generator().manual_seed(1009 * b + 31 * n + d + 7 * (regime == "positive"))
        self.x, self.dy = torch.randn(b, n, d, generator=g), torch.randn(b, d, generator=g)
        if regime == "positive":
            self.x = self.x.abs()
        self.b, self.n, self.d = b, n, d
        x, dy = self.x.double(), self.dy.double()
        self.terms64 = {"y": (x.mean(1), x.abs().sum(1) / n), "dx": ((dy / n)[:, None].expand(b, n, d), (dy.abs() / n)[:, None].expand(b, n, d))}

    def terms(self, y, dx):
        got = {"y": _d(y), "dx": _d(dx)}
        return {q: (got[q],) + self.terms64[q] + (torch.zeros(()),) for q in got}


@functools.lru_cache(maxsize=4)
def _mean(b, n, d, regime):
    return Mean(b, n, d, regime)


def _mean32(P, how):
    """float32 -> (y, dx).  "torch": x.mean(1) and autograd; "emulation": mean_axis1_fwd_f32's index-order sum, then one division
    by (float) n, and dy / (float) n; "n_minus_1": the emulation dividing by n - 1."""
    if how == "torch":
        x = P.x.clone().requires_grad_(True)
        y = x.mean(1)
        y.backward(P.dy)
        return y.detach(), x.grad
    return _emu_mean(P.x, P.dy, float(P.n - 1 if how == "n_minus_1" else P.n))


def _emu_mean(x, dy, div):
    s = torch.zeros(x.shape[0], x.shape[2])
    for j in range(x.shape[1]):
        s = s + x[:, j]
    return s / div, (dy / div)[:, None].expand(x.shape)


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def _ratio(got, c64, bound):
    ratio = (got - c64).abs() / (bound + 1e-30)
    return float(torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).max()) if got.numel() else 0.0


WORST = {}      # (family, quantity) -> worst error / bound of a run (the MI355X figures of the docstring come from here)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the file's last test: the worst error / bound per kernel and quantity (shown with -s)."""
    yield
    for family, q in sorted(WORST):
        if family != "cpu":
            print(f"worst error / bound, {family} {q}: {WORST[(family, q)]:.3f}")


def _check_terms(family, terms, constants, what):
    """|got - c64| <= C[q] 2^-24 S + the additive term, per element and per quantity; prints the worst error / bound."""
    for q, (got, c64, s, extra) in terms.items():
        bound = constants[q] * U32 * s + extra
        worst = _ratio(got, c64, bound)
        WORST[(family, q)] = max(WORST.get((family, q), 0.0), worst)
        print(f"[{family}] {what} {q}: error / bound {worst:.3f}")
        _within(got, c64, bound / U32, tol=U32, what=f"{family} {what} {q}")


def _mean_constants(n):
    return {"y": C_MEAN[n][0], "dx": C_MEAN[n][1]}


def _rejected(terms, constants, q, what):
    with pytest.raises(AssertionError, match=f" {q}: error .* x the bound"):
        _check_terms("cpu", {q: terms[q]}, constants, what)


def _one_element(good, bad, index):
    out = good.clone()
    out[index] = bad[index]
    return out


# ---- CPU: the checker accepts the reference-only evaluations and rejects what it must -------------------------------------------
@pytest.mark.parametrize("shape", GEGLU_SHAPES, ids=_sid)
def test_geglu_checker_accepts_float32_torch_and_the_emulation(shape):
    rows, h = _resolve(shape, 0)
    for planting in range(len(SPECIAL_GATES)):
        P = _geglu(rows, h, planting)
        for how in ("torch", "emulation"):
            _check_terms("cpu", P.terms(*_geglu32(P, how)), C_GEGLU, f"{rows}x{h} planting {planting} {how}")


@pytest.mark.parametrize("shape", [(3, 85), (7, 37), (50, 96)], ids=_sid)
def test_geglu_checker_rejects_the_tanh_approximation_and_a_gate_one_column_off(shape):
    """In ONE element of an otherwise correct float32 result: the element whose gate is nearest 2 (where the tanh form of gelu is
    2^-13 off, against a bound of a few 2^-24) and, for the shifted gate, the same element."""
    rows, h = shape
    P = _geglu(rows, h, 0)
    y, dx = _geglu32(P, "emulation")
    _check_terms("cpu", P.terms(y, dx), C_GEGLU, "unmutated")
    flat = int((P.gate - 2.0).abs().argmin())
    r, c = flat // h, flat % h
    for how in ("tanh", "column_off"):
        by, bdx = _geglu32(P, how)
        _rejected(P.terms(_one_element(y, by, (r, c)), dx), C_GEGLU, "y", f"{how} in one element")
        _rejected(P.terms(y, _one_element(dx, bdx, (r, c))), C_GEGLU, "dx_a", f"{how} in one element")
        _rejected(P.terms(y, _one_element(dx, bdx, (r, h + c))), C_GEGLU, "dx_g", f"{how} in one element")


@pytest.mark.parametrize("regime", MEAN_REGIMES)
@pytest.mark.parametrize("shape", MEAN_SHAPES, ids=_sid)
def test_mean_checker_accepts_float32_torch_and_the_emulation(shape, regime):
    b, n, d = _resolve(shape, 1)
    P = _mean(b, n, d, regime)
    for how in ("torch", "emulation"):
        _check_terms("cpu", P.terms(*_mean32(P, how)), _mean_constants(n), f"{b}x{n}x{d} {regime} {how}")


@pytest.mark.parametrize("shape", [(4, 9, 13), (3, 2, 100), (2, 1000, 7)], ids=_sid)
def test_mean_checker_rejects_a_division_by_n_minus_1(shape):
    """In one element, `positive` operands (nothing cancels: the error is S / (n - 1), some 270 x the bound even at n = 1000)."""
    b, n, d = shape
    P = _mean(b, n, d, "positive")
    y, dx = _mean32(P, "emulation")
    by, bdx = _mean32(P, "n_minus_1")
    _check_terms("cpu", P.terms(y, dx), _mean_constants(n), "unmutated")
    _rejected(P.terms(_one_element(y, by, (b - 1, d - 1)), dx), _mean_constants(n), "y", "n - 1 in one element")
    _rejected(P.terms(y, _one_element(dx.clone(), bdx, (b - 1, n - 1, d - 1))), _mean_constants(n), "dx", "n - 1 in one element")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GEGLU_SHAPES, ids=_sid)
def test_geglu_kernels_per_element(shape, device):
    """geglu_fwd_f32 and geglu_bwd_f32 at every planting of the special gates; PF.geglu's autograd binding bitwise."""
    from predict_pv_yield_amd import perceiver_functional as PF
    K = _ops()
    rows, h = _resolve(shape, 0)
    for planting in range(len(SPECIAL_GATES)):
        P = _geglu(rows, h, planting)
        x, dy = P.x.to(device), P.dy.to(device)
        y, dx = K.geglu_fwd(x), K.geglu_bwd(x, dy)
        _check_terms("geglu", P.terms(y, dx), C_GEGLU, f"{rows}x{h} planting {planting}")
        xa = x.clone().requires_grad_(True)
        ya = PF.geglu(xa)
        ya.backward(dy)
        _same_bits(ya.detach(), y, "PF.geglu forward against the direct call")
        _same_bits(xa.grad, dx, "PF.geglu backward against the direct call")


@pytest.mark.gpu
@pytest.mark.parametrize("regime", MEAN_REGIMES)
@pytest.mark.parametrize("shape", MEAN_SHAPES, ids=_sid)
def test_mean_kernels_per_element(shape, regime, device):
    """mean_axis1_fwd_f32 and mean_axis1_bwd_f32; PF.mean_axis1's autograd binding bitwise."""
    from predict_pv_yield_amd import perceiver_functional as PF
    K = _ops()
    b, n, d = _resolve(shape, 1)
    P = _mean(b, n, d, regime)
    x, dy = P.x.to(device), P.dy.to(device)
    y, dx = K.mean_axis1_fwd(x), K.mean_axis1_bwd(dy, n)
    _check_terms("mean", P.terms(y, dx), _mean_constants(n), f"{b}x{n}x{d} {regime}")
    xa = x.clone().requires_grad_(True)
    ya = PF.mean_axis1(xa)
    ya.backward(dy)
    _same_bits(ya.detach(), y, "PF.mean_axis1 forward against the direct call")
    _same_bits(xa.grad, dx, "PF.mean_axis1 backward against the direct call")


def _ulps(fn, x, device):
    """Worst |fn(x) on the device - fn(x) in float64| in units of 2^-23 |value|, over the normal results."""
    ref = fn(x.double())
    got = fn(x.to(device)).double().cpu()
    ok = ref.abs() >= TINY
    return float(((got - ref).abs() / (ULP * ref.abs()))[ok].max())


@pytest.mark.gpu
def test_device_math_functions_are_within_F(device):
    """torch's own elementwise erf and exp on the GPU against float64 over the arguments of every GEGLU case: F = 2 x the worst."""
    gates = torch.cat([_geglu(*_resolve(s, 0), p).gate.flatten() for s in GEGLU_SHAPES for p in range(len(SPECIAL_GATES))])
    for name, fn, x, f in (("erf", torch.erf, gates * RSQRT2, F_ERF), ("exp", torch.exp, -0.5 * gates * gates, F_EXP)):
        worst = _ulps(fn, x, device)
        print(f"device {name}: worst error {worst:.3f} ulps over {x.numel()} arguments in [{float(x.min()):.2f}, {float(x.max()):.2f}] -> F = {2 * worst:.2f}")
        assert f <= F_MAX, f"F of {name} is {f}: above {F_MAX}, the bounds of this file no longer say anything"
        assert 2 * worst <= f, f"device {name}: 2 x {worst:.3f} ulps exceeds F = {f}"


class Guarded:
    """`shape` elements inside a sentinel-filled buffer."""

    def __init__(self, shape, device):
        numel = math.prod(shape)
        self.buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=device)
        self.t = self.buf[GUARD:GUARD + numel].view(*shape)

    def intact(self):
        want = _bits(torch.tensor([SENTINEL]))
        b = _bits(self.buf.cpu())
        return bool((b[:GUARD] == want).all() and (b[-GUARD:] == want).all())


@pytest.mark.gpu
def test_outputs_stay_inside_their_buffers(device):
    """One ragged shape per family, (7, 37) and (4, 9, 13): every output inside a sentinel-filled buffer, through the C ABI."""
    from predict_pv_yield_amd import _lib
    K = _ops()
    lib, ptr, stream = _lib.get_lib(), _lib.ptr, _lib.current_stream_ptr
    rows, h = 7, 37
    P = _geglu(rows, h, 0)
    x, dy = P.x.to(device), P.dy.to(device)
    y, dx = Guarded((rows, h), device), Guarded((rows, 2 * h), device)
    K.check(lib.pv_geglu_fwd_f32(ptr(x), ptr(y.t), rows, h, stream()), "pv_geglu_fwd_f32")
    K.check(lib.pv_geglu_bwd_f32(ptr(x), ptr(dy), ptr(dx.t), rows, h, stream()), "pv_geglu_bwd_f32")
    torch.cuda.synchronize()
    assert y.intact() and dx.intact(), "GEGLU wrote outside its result"
    _check_terms("geglu", P.terms(y.t, dx.t), C_GEGLU, "7x37 guarded")
    b, n, d = 4, 9, 13
    M = _mean(b, n, d, "zero_mean")
    xm, dym = M.x.to(device), M.dy.to(device)
    ym, dxm = Guarded((b, d), device), Guarded((b, n, d), device)
    K.check(lib.pv_mean_axis1_fwd_f32(ptr(xm), ptr(ym.t), b, n, d, stream()), "pv_mean_axis1_fwd_f32")
    K.check(lib.pv_mean_axis1_bwd_f32(ptr(dym), ptr(dxm.t), b, n, d, stream()), "pv_mean_axis1_bwd_f32")
    torch.cuda.synchronize()
    assert ym.intact() and dxm.intact(), "the mean wrote outside its result"
    _check_terms("mean", M.terms(ym.t, dxm.t), _mean_constants(n), "4x9x13 guarded")


# ---- the tables in the module docstring -----------------------------------------------------------------------------------------
def _measure():
    worst = {q: [0.0, 0.0] for q in C_GEGLU}
    for shape in GEGLU_SHAPES:
        rows, h = _resolve(shape, 0)
        for planting in range(len(SPECIAL_GATES)):
            P = _geglu(rows, h, planting)
            for col, how in enumerate(("torch", "emulation")):
                for q, (got, c64, s, _) in P.terms(*_geglu32(P, how)).items():
                    worst[q][col] = max(worst[q][col], _ratio(got, c64, U32 * s))
    print("    GEGLU      float32 torch   emulation   constant (4 x the worse)")
    for q, (t32, emu) in worst.items():
        print(f"    {q:<10} {t32:8.2f}      {emu:8.2f}      {4 * max(t32, emu):6.1f}")
    print("    mean n     forward: float32 torch / emulation   backward: float32 torch / emulation   constants")
    for shape in MEAN_SHAPES:
        b, n, d = _resolve(shape, 1)
        w = {"y": [0.0, 0.0], "dx": [0.0, 0.0]}
        for regime in MEAN_REGIMES:
            P = _mean(b, n, d, regime)
            for col, how in enumerate(("torch", "emulation")):
                for q, (got, c64, s, _) in P.terms(*_mean32(P, how)).items():
                    w[q][col] = max(w[q][col], _ratio(got, c64, U32 * s))
        print(f"    {n:<10} {w['y'][0]:6.2f} / {w['y'][1]:6.2f}      {w['dx'][0]:6.2f} / {w['dx'][1]:6.2f}      {n}: ({math.ceil(40 * max(w['y'])) / 10}, {math.ceil(40 * max(w['dx'])) / 10})")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the model widths are read from the package
    _measure()
