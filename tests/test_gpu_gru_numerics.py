"""The GRU kernels -- csrc/gru_f32.hip: gru_seq_{fwd,bwd}_f32, gru_seq_{fwd,bwd}_hs_f32<16>, gru_sum_rows_f32 -- per element against
float64, at the hidden sizes, lengths and batches where each of their rules begins and ends, and CPU tests that show the checker
rejects a kernel that is subtly wrong.  Vocabulary and manner: tests/test_gpu_linear_numerics.py.

Reference: never a whole sequence.  The project's bound is |c - c64| <= C 2^-24 S with S the float64 sum of the absolute terms of
the element's own expression; carried through T steps of a recurrence S grows to 10^4 .. 10^45 times the result and accepts
anything.  So every element is held to a float64 evaluation of ONE STEP's expression on THE KERNEL'S OWN STORED OPERANDS (float32
values, exact in float64), and S is that step's.  Forward, with hprev the kernel's own out[:, t - 1] (h0, or zeros, at t = 0)
(`_forward_terms`):
    an      b_hn + sum_k W_hn[j, k] hprev_k                          S = |b_hn| + sum |W| |hprev|
    r, z    sigmoid(gi + b + W hprev)                                S = (|gi| + |b| + sum |W| |hprev|) / 4 + value
    n       tanh(gi_n + r an) on the kernel's own r, an              S = |gi_n| + |r an| + |n|
    out     (1 - z) n + z hprev on the kernel's own z, n             S = |n| + |z n| + |z hprev|
Backward, dgi and dh0 (`_backward_terms`): a T-step call equals T chained one-step calls (t_len = 1, dh_last = the previous call's
dh0, h0 = hprev, dout[:, t:t + 1], out and saved the contiguous slices of step t): the library is built without contraction and a
step does the same arithmetic in either call.  The T-step dgi and dh0 are asserted BITWISE equal to the chain's, and every one-step
call is checked per element, dh = dh_last + dout in float64:
    dn_pre  dh (1 - z)(1 - n^2)                                      S = (|dh_last| + |dout|)(1 + z)(1 + n^2)
    dz_pre  dh (hprev - n) z (1 - z)                                 S = (|dh_last| + |dout|)(|hprev| + |n|) z (1 + z)
    dr_pre  dn_pre64 an r (1 - r)                                    S = S_dn |an| r (1 + r)
    dh0     dh z + sum_j W[g hs + j, k] g_j, g the call's own dgi
            (g_n = dn_pre r)                                         S = |dh z| + sum |W| |g|
dW_hh and db_hh of the T-step call (`_weight_terms`): the float64 sums over batch and time of g_{b,t,j} hprev_{b,t,k} and of
g_{b,t,j}, from the kernel's own dgi, saved and out; S the same sums of |g| |hprev| and |g|.
Whole layers, free-running (PF.gru, two layers, against float64 nn.GRU; outputs, h_n, dx, dh0, every parameter gradient): no local
S exists, so the relative norm per tensor (`_rel`) against FREE_TOL.

Constants.  From the REFERENCE's own error, never from the kernels: 4 x the worst error / (2^-24 S) of reference-only evaluations
of every case of this file, at every argument set, one constant per quantity.  The evaluations: float32 torch (matmul, einsum,
torch.sigmoid) and the emulation of the source's order (`_emu_forward`, `_emu_backward`): the forward's fmaf chain over k starting
from the bias and 1 / (1 + exp(-x)); every backward product and sum rounded separately; the general backward's
(w_r g_r + w_z g_z) + w_n g_n per lane, then the xor-shuffle tree with offsets 32 .. 1 over 64 lanes (`_emu_xor_tree`), added to
dh z; the <16> backward's index-order sum of the same three-term sums onto dh z; each row's dW_hh += g hprev walking t down, then
gru_sum_rows_f32's index-order sum over the batch rows.  `python tests/test_gpu_gru_numerics.py` prints the table:
    quantity   float32 torch   emulation   constant
    an             4.70          4.30        18.8
    r              2.21          2.02         8.9
    z              2.15          2.23         9.0
    n              1.26          1.25         5.1
    out            2.29          2.29         9.2
    dn_pre         2.92          2.80        11.7
    dz_pre         3.91          3.99        16.0
    dr_pre         3.93          3.75        15.8
    dh0            7.89          6.10        31.6
    dw_hh         13.84          7.95        55.4     (float32 torch: one einsum over up to 70 x 31 terms in the CPU library's order)
    db_hh          3.94          4.19        16.8
Free-running: float32 nn.GRU against float64 nn.GRU on the CPU over FREE_CASES with and without h0, worst relative norm per kind of
tensor: out 4.15e-7, h_n 4.76e-7, dx 1.19e-6, dh0 2.04e-7, d weight_ih 1.20e-6, d weight_hh 1.36e-6, d bias_ih 1.21e-6, d bias_hh
1.42e-6 -> FREE_TOL = 4 x 1.418e-6 = 5.68e-6, one tolerance for every tensor.

Device math functions.  expf and tanhf on the GPU are not the CPU's; their error is measured on the GPU through torch's own
elementwise exp and tanh against float64, never through the kernels under test, over the arguments the cases produce (-x of both
sigmoids, gi_n + r an; `_function_arguments`), and enters the bounds of r, z and n as the additive term F 2^-23 |value| with F = 2 x
the worst observed error in ulps of the function value (a sigmoid's error from its exp is value (1 - value) x the exp's relative
error, at most the same term).  Measured on the MI355X: exp 0.688 ulps over 2 088 712 arguments in [-14.99, 15.29] -> F_EXP = 1.38;
tanh 1.220 ulps over 1 044 356 arguments in [-13.46, 15.40] -> F_TANH = 2.45 (each 2 x the worst, rounded up to 0.01; both far below
8, above which the file's premise would fail).  test_device_math_functions_are_within_F measures again and holds the constants to it.

Cases (the smallest shapes at which each rule begins or ends).  Hidden 1; 7; 16 through the <16> kernels; 16 with PV_GRU_GENERAL=1
(read per call); 17; 33, the first size where the lane that zeroes an entry of dw_part (i % 64) and the lane that accumulates into
it (i / hs) differ for most entries; 63; 64 = GRU_MAXH, every lane active, no idle lane in the shuffle tree.  Each at (T, batch) =
(1, 1), (2, 3), (24, 3); hidden 16 (both kernel pairs), 33 and 64 also at (31, 70), so that gru_sum_rows_f32 adds 70 rows.  Two
regimes: `init` (w_hh, b_hh uniform in +-1 / sqrt(hs) as nn.GRU.reset_parameters draws them, gi ~ randn) and `saturating` (weights,
bias and gi x 3: gates near 0 and 1, 1 - n n cancels).  Argument sets: with h0; without h0; dout = None; dh_last = None (two branches
of the C entry point that autograd never takes); each again with need_dh0=False (dh0 == nullptr): dgi, dW_hh, db_hh must be the bits
of the call that asks for dh0.  Planted: 0.0, -0.0, +-2^-126 in h0 and in gi (first and last step, every gate) at the first and last
unit of the first and last batch row.  Every backward output has identical bits across two calls.  <16> against the general
kernels: out and saved bitwise at every (T, batch); at T = 1 dgi, dW_hh and db_hh bitwise, as the source's comment claims (dh0 is
held to its float64 bound in both).  Refusals through the C ABI: hidden = 65 and 0 return -2, a workspace one byte short -1, every
output buffer keeps its sentinel.  Sentinels: hidden 7 and 64 at (2, 3), out, saved, dgi, dh0, dw_hh, db_hh and the workspace each
inside a buffer filled with 1.2345678e30.  PF.gru: hidden 16 and 64, input widths 9, 33 and 2048 (the smallest that takes gru()'s
linear_f32 route; batch 2, T 3), with and without h0.

What the checker is sensitive to (CPU tests, `init`, hidden 7 / 17 / 16 with the <16> emulation).  It accepts float32 torch and the
emulation at every case and argument set, and rejects, applied to ONE step of an otherwise correct float32 evaluation, each by the
quantity named: the last k term of W_hn h dropped (an); the r and z blocks of W_hh swapped (r, z); n = tanh(gi_n + r W_hn h + b_hn),
the other common GRU (n); h' = z n + (1 - z) h (out); the backward's hprev taken from step t (dz_pre, dw_hh); dh z left out of
dh_prev (dh0); g_n = dn_pre without r (dh0, dw_hh, db_hh); one batch row missing from db_hh (db_hh); one (j, k) entry of dW_hh left
at the previous step's value (dw_hh).
What it cannot see: which of two bitwise-equal schedules ran (the <16> kernels and the general ones give one forward); a read
outside an operand whose value is discarded (the <16> kernels' idle lanes read row 0 of W_hh and b_hh by design); an ordering
hazard that the hardware happens to resolve in program order -- the general backward zeroes dw_part[i] from lane i % 64 and
accumulates into it from lane i / hs of the same wave with nothing between the two but program order: hidden 33, 63 and 64 give the
float64 sums here and the same bits twice, which shows the result, not that the order is guaranteed; an error common to the
kernel's stored operand and its use (a wrong `saved` that the backward then reads is caught by the forward's check, not the
backward's); and, in the free-running test, anything below 5.68e-6 of a tensor's norm.

Measured on the MI355X with these constants, worst error / bound over all cases (general kernels at hidden <= 32 / hidden > 32 /
<16> kernels): an 0.245 / 0.240 / 0.245; r 0.148 / 0.226 / 0.148; z 0.150 / 0.231 / 0.150; n 0.188 / 0.185 / 0.188; out 0.239 /
0.248 / 0.239; dn_pre 0.227 / 0.251 / 0.264; dz_pre 0.202 / 0.256 / 0.226; dr_pre 0.192 / 0.263 / 0.182; one-step dh0 0.089 / 0.113 /
0.199; dw_hh 0.117 / 0.144 / 0.095; db_hh 0.215 / 0.293 / 0.201.  The CPU evaluations' own worst is 0.25 of the bound by
construction.  PF.gru, worst relative norm / FREE_TOL: out 0.18, h_n 0.20, dx 0.29, dh0 0.07, d weight_ih 0.29, d weight_hh 0.39, d
bias_ih 0.32, d bias_hh 0.64.  Every bitwise relation held, the source's comment about the <16> kernels included.  No case found a
fault in the kernels' results: not the dw_part zero-then-accumulate at hidden > 32, not dh0 at hidden 64, not the null-gradient
branches.  The 42 GPU cases take 3 s together, the slowest (hidden 64, T 31, batch 70) 0.2 s; the 112 CPU cases take 10 s.
"""
import functools
import math

import pytest
import torch

from conv2d_f32_helpers import _ops, _rel, _within

U32 = 2.0 ** -24
ULP = 2.0 ** -23         # one unit in the last place of a float32 value, relative
SENTINEL = 1.2345678e30
GUARD = 64
TINY = 2.0 ** -126
GRU_MAXH = 64            # csrc/gru_f32.hip
F64 = torch.float64

# 4 x the reference-only ratios printed by `python tests/test_gpu_gru_numerics.py` (module docstring), one per checked quantity
C = {"an": 18.8, "r": 8.9, "z": 9.0, "n": 5.1, "out": 9.2, "dn_pre": 11.7, "dz_pre": 16.0, "dr_pre": 15.8, "dh0": 31.6, "dw_hh": 55.4, "db_hh": 16.8}
# 2 x the worst error of torch's own elementwise exp / tanh on the MI355X, in ulps of the function value (module docstring)
F_EXP, F_TANH = 1.38, 2.45
F_MAX = 8.0              # above this the file's premise fails: test_device_math_functions_are_within_F says so
FREE_TOL = 5.68e-6           # 4 x the worst _rel of float32 nn.GRU against float64 nn.GRU over FREE_CASES (module docstring)

REGIMES = ("init", "saturating")
HIDDEN = [(1, False), (7, False), (16, False), (16, True), (17, False), (33, False), (63, False), (64, False)]      # (hidden, PV_GRU_GENERAL)
SHAPES = [(1, 1), (2, 3), (24, 3)]                                                                                 # (T, batch)
LONG = (31, 70)
CASES = [(hs, gen, t, b) for hs, gen in HIDDEN for t, b in SHAPES] + [(hs, gen, *LONG) for hs, gen in ((16, False), (16, True), (33, False), (64, False))]
FREE_CASES = [(hs, inp, b, t) for hs in (16, 64) for inp, b, t in ((9, 3, 7), (33, 3, 12), (2048, 2, 3))]           # (hidden, input width, batch, T)
REJECT = [(7, 2, 3), (17, 24, 3), (16, 24, 3)]                                                                     # (hidden, T, batch)


def _cid(case):
    hs, gen, t, b = case
    return f"h{hs}{'general' if gen else ''}-T{t}-B{b}"


def _mode(hs, general):
    """Which kernel pair a hidden size runs: the emulation of dh_prev follows it."""
    return "hs16" if hs == 16 and not general else "general"


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
class Problem:
    """One layer's sequential part on the CPU: w_hh [3 hs, hs], b_hh [3 hs] drawn as nn.GRU.reset_parameters draws them
    (uniform in +-1 / sqrt(hs)), gi [b, T, 3 hs] ~ randn, h0 in (-1, 1), dout and dh_last ~ randn; `saturating`: w, b and gi x 3."""

    def __init__(self, hs, t, b, regime):
        g = torch.Generator().manual_seed(100003 * hs + 1009 * t + 17 * b + (regime == "saturating"))
        stdv, scale = 1.0 / math.sqrt(hs), 3.0 if regime == "saturating" else 1.0
        self.w = (torch.rand(3 * hs, hs, generator=g) * 2 - 1) * stdv * scale
        self.bias = (torch.rand(3 * hs, generator=g) * 2 - 1) * stdv * scale
        self.gi = torch.randn(b, t, 3 * hs, generator=g) * scale
        self.h0 = torch.tanh(torch.randn(b, hs, generator=g))
        self.dout, self.dh_last = torch.randn(b, t, hs, generator=g), torch.randn(b, hs, generator=g)
        special, i = (0.0, -0.0, TINY, -TINY), 0
        for row in sorted({0, b - 1}):
            for unit in sorted({0, hs - 1}):
                self.h0[row, unit] = special[i % 4]
                for step in sorted({0, t - 1}):
                    for gate in range(3):
                        self.gi[row, step, gate * hs + unit] = special[(i + gate + step) % 4]
                i += 1
        self.hs, self.t, self.b, self.regime = hs, t, b, regime


@functools.lru_cache(maxsize=8)
def _problem(hs, t, b, regime):
    return Problem(hs, t, b, regime)


def _d(x):
    return x.detach().double().cpu()


def _zeros(*shape):
    return torch.zeros(*shape)


# ---- the float64 references of one step, on the candidate's own stored operands -------------------------------------------------
def _hprev(h0, out):
    first = h0 if h0 is not None else torch.zeros_like(out[:, 0])
    return torch.cat([first[:, None], out[:, :-1]], 1)


def _forward_terms(P, h0, out, saved):
    """-> {quantity: (got, float64 reference, S, additive term)} over every step at once: hprev is the candidate's own out[:, t - 1]."""
    hs = P.hs
    o, sv = _d(out), _d(saved)
    hprev = _hprev(None if h0 is None else _d(h0), o)
    r, z, n, an = sv.split(hs, 2)
    w, bias = P.w.double(), P.bias.double()
    a, sa = hprev @ w.t() + bias, hprev.abs() @ w.abs().t() + bias.abs()
    (ar, az, an64), (sr, sz, san) = a.split(hs, 2), sa.split(hs, 2)
    gr, gz, gn = P.gi.double().split(hs, 2)
    r64, z64, n64 = torch.sigmoid(gr + ar), torch.sigmoid(gz + az), torch.tanh(gn + r * an)
    none = torch.zeros(())
    return {"an": (an, an64, san, none),
            "r": (r, r64, (gr.abs() + sr) / 4 + r64, F_EXP * ULP * r64),
            "z": (z, z64, (gz.abs() + sz) / 4 + z64, F_EXP * ULP * z64),
            "n": (n, n64, gn.abs() + (r * an).abs() + n64.abs(), F_TANH * ULP * n64.abs()),
            "out": (o, (1 - z) * n + z * hprev, n.abs() + (z * n).abs() + (z * hprev).abs(), none)}


def _g_own(P, saved, dgi):
    """The candidate's own gradients of the three W_hh h + b_hh pre-activations: (dr_pre, dz_pre, dn_pre r) -> [b, T, 3 hs]."""
    hs = P.hs
    dr, dz, dn = _d(dgi).split(hs, 2)
    return torch.cat([dr, dz, dn * _d(saved)[..., :hs]], 2)


def _backward_terms(P, dout, h0, out, saved, dgi, dhl, dh0s):
    """One-step calls, every step at once: dhl[:, t] is the dh_last that step t's call received, dh0s[:, t] the dh0 it returned."""
    hs = P.hs
    o, sv, dhl = _d(out), _d(saved), _d(dhl)
    do = torch.zeros_like(o) if dout is None else _d(dout)
    hprev = _hprev(None if h0 is None else _d(h0), o)
    r, z, n, an = sv.split(hs, 2)
    dr, dz, dn = _d(dgi).split(hs, 2)
    dh, sdh = dhl + do, dhl.abs() + do.abs()
    dn64, sdn = dh * (1 - z) * (1 - n * n), sdh * (1 + z) * (1 + n * n)
    g, w = _g_own(P, saved, dgi), P.w.double()
    none = torch.zeros(())
    return {"dn_pre": (dn, dn64, sdn, none),
            "dz_pre": (dz, dh * (hprev - n) * z * (1 - z), sdh * (hprev.abs() + n.abs()) * z * (1 + z), none),
            "dr_pre": (dr, dn64 * an * r * (1 - r), sdn * an.abs() * r * (1 + r), none),
            "dh0": (_d(dh0s), dh * z + g @ w, (dh * z).abs() + g.abs() @ w.abs(), none)}


def _weight_terms(P, h0, out, saved, dgi, dw, db):
    """The T-step call's dW_hh and db_hh against the float64 sums over batch and time of the candidate's own g and hprev."""
    o = _d(out)
    hprev, g = _hprev(None if h0 is None else _d(h0), o), _g_own(P, saved, dgi)
    none = torch.zeros(())
    return {"dw_hh": (_d(dw), torch.einsum("btj,btk->jk", g, hprev), torch.einsum("btj,btk->jk", g.abs(), hprev.abs()), none),
            "db_hh": (_d(db), g.sum((0, 1)), g.abs().sum((0, 1)), none)}


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def _ratio(got, c64, bound):
    ratio = (got - c64).abs() / (bound + 1e-30)
    return float(torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).max()) if got.numel() else 0.0


WORST = {}      # (family, quantity) -> worst error / bound of a run (the MI355X figures of the docstring come from here)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the file's last test: the worst error / bound per kernel family and quantity (shown with -s)."""
    yield
    for family, q in sorted(WORST):
        if family != "cpu":
            print(f"worst error / bound, {family} {q}: {WORST[(family, q)]:.3f}")


def _check_terms(family, terms, what):
    """|got - c64| <= C[q] 2^-24 S + the additive term, per element and per quantity; prints the worst error / bound."""
    for q, (got, c64, s, extra) in terms.items():
        bound = C[q] * U32 * s + extra
        worst = _ratio(got, c64, bound)
        WORST[(family, q)] = max(WORST.get((family, q), 0.0), worst)
        print(f"[{family}] {what} {q}: error / bound {worst:.3f}")
        _within(got, c64, bound / U32, tol=U32, what=f"{family} {what} {q}")


def _rejected(terms, q, what):
    """The checker rejects quantity q (and says so by name)."""
    with pytest.raises(AssertionError, match=f" {q}: error .* x the bound"):
        _check_terms("cpu", {q: terms[q]}, what)


# ---- reference-only float32 evaluations: float32 torch and the emulation of the source's order ----------------------------------
def _emu_sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))      # sigmoidf_ of the source


def _fwd32(P, h0, emu, mutation=None, at=-1):
    """float32 forward -> (out, saved).  emu: the source's fmaf chain over k starting from the bias (exact product, one rounding
    per step) and its sigmoid; else float32 torch (matmul, torch.sigmoid).  A mutation is applied to step `at` alone."""
    hs, b = P.hs, P.b
    h = h0 if h0 is not None else _zeros(b, hs)
    outs, saved = [], []
    for t in range(P.t):
        mut = mutation if t == at else None
        w = P.w
        if mut == "swap_rz":
            w = torch.cat([w[hs:2 * hs], w[:hs], w[2 * hs:]])
        if mut == "drop_last_k":
            w = w.clone()
            w[2 * hs:, -1] = 0.0
        if emu:
            a = P.bias.expand(b, 3 * hs).clone()
            for k in range(hs):
                a = (a.double() + w[:, k].double() * h[:, k:k + 1].double()).float()
        else:
            a = h @ w.t() + P.bias
        ar, az, an = a.split(hs, 1)
        gr, gz, gn = P.gi[:, t].split(hs, 1)
        sig = _emu_sigmoid if emu else torch.sigmoid
        r, z = sig(gr + ar), sig(gz + az)
        n = torch.tanh(gn + r * (an - P.bias[2 * hs:]) + P.bias[2 * hs:]) if mut == "bias_outside" else torch.tanh(gn + r * an)
        h = z * n + (1.0 - z) * h if mut == "swapped_update" else (1.0 - z) * n + z * h
        outs.append(h)
        saved.append(torch.cat([r, z, n, an], 1))
    return torch.stack(outs, 1), torch.stack(saved, 1)


def _emu_xor_tree(c):
    """for (off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64) over the last axis (64 lanes)."""
    lane = torch.arange(64)
    off = 32
    while off:
        c = c + c[..., lane ^ off]
        off //= 2
    return c


def _step32(P, dh_last, dout_t, hprev, saved_t, mode, mutation=None):
    """One step of the backward in float32, every operation rounded as the source's (no contraction) -> (dgi_t, dh_prev, g).
    mode: "torch" (dh_prev through a float32 matmul), "general" ((w_r g_r + w_z g_z) + w_n g_n per lane, then the xor-shuffle
    tree over 64 lanes), "hs16" (the same three-term sum of unit j added onto dh z in index order)."""
    hs, w = P.hs, P.w
    dh = dh_last + dout_t
    r, z, n, an = saved_t.split(hs, 1)
    dn = dh * (1.0 - z) * (1.0 - n * n)
    dz = dh * (hprev - n) * z * (1.0 - z)
    dr = dn * an * r * (1.0 - r)
    gr, gz, gn = dr, dz, (dn if mutation == "gn_without_r" else dn * r)
    keep = torch.zeros_like(dh) if mutation == "no_dh_z" else dh * z
    wr, wz, wn = w[:hs], w[hs:2 * hs], w[2 * hs:]
    if mode == "torch":
        dh_prev = keep + torch.cat([gr, gz, gn], 1) @ w
    elif mode == "general":
        c = torch.zeros(P.b, hs, 64)      # [row, column k, lane j]
        c[:, :, :hs] = ((wr * gr[:, :, None] + wz * gz[:, :, None]) + wn * gn[:, :, None]).transpose(1, 2)
        dh_prev = keep + _emu_xor_tree(c)[:, :, 0]
    else:
        dh_prev = keep
        for j in range(hs):
            dh_prev = dh_prev + ((wr[j] * gr[:, j:j + 1] + wz[j] * gz[:, j:j + 1]) + wn[j] * gn[:, j:j + 1])
    return torch.cat([dr, dz, dn], 1), dh_prev, torch.cat([gr, gz, gn], 1)


def _bwd32(P, dout, dh_last, h0, out, saved, mode, mutation=None, at=-1):
    """float32 backward of T steps -> (dgi, dh0, dw_hh, db_hh, dhl, dh0s); dhl / dh0s: what each step received / returned.
    Emulation: each row's dW_hh += g hprev (rounded product, then the add) walking t down, then gru_sum_rows_f32's index-order sum
    over the batch rows; "torch": one float32 einsum.  Mutations act on step `at` (or, for the two sums, on their last term)."""
    hs, b, T = P.hs, P.b, P.t
    dh = dh_last if dh_last is not None else _zeros(b, hs)
    hp_all = _hprev(h0, out)
    dgi, dhl, dh0s, gs = [None] * T, [None] * T, [None] * T, [None] * T
    dw_rows, db_rows = _zeros(b, 3 * hs, hs), _zeros(b, 3 * hs)
    for t in reversed(range(T)):
        mut = mutation if t == at else None
        hprev = out[:, t] if mut == "hprev_of_step_t" else hp_all[:, t]
        dhl[t] = dh
        dgi[t], dh, gs[t] = _step32(P, dh, dout[:, t] if dout is not None else _zeros(b, hs), hprev, saved[:, t], mode, mut)
        dh0s[t] = dh
        stale = dw_rows[:, hs - 1, 0].clone()
        dw_rows, db_rows = dw_rows + gs[t][:, :, None] * hprev[:, None, :], db_rows + gs[t]
        if mut == "stale_dw_entry":
            dw_rows[:, hs - 1, 0] = stale
    if mode == "torch":
        g = torch.stack(gs, 1)
        dw, db = torch.einsum("btj,btk->jk", g, torch.stack([out[:, t] if (mutation == "hprev_of_step_t" and t == at) else hp_all[:, t] for t in range(T)], 1)), g.sum((0, 1))
        if mutation == "stale_dw_entry":
            dw[hs - 1, 0] = dw[hs - 1, 0] - (gs[at][:, hs - 1] * hp_all[:, at, 0]).sum()
        if mutation == "db_row_missing":
            db = db - torch.stack(gs, 1)[b - 1].sum(0)
    else:
        dw, db = _zeros(3 * hs, hs), _zeros(3 * hs)
        for row in range(b):
            dw = dw + dw_rows[row]
            if not (mutation == "db_row_missing" and row == b - 1):
                db = db + db_rows[row]
    return torch.stack(dgi, 1), dh, dw, db, torch.stack(dhl, 1), torch.stack(dh0s, 1)


def _emu_forward(P, h0, mutation=None, at=-1):
    return _fwd32(P, h0, True, mutation, at)


def _emu_backward(P, dout, dh_last, h0, out, saved, mode, mutation=None, at=-1):
    """mode "general": gru_seq_bwd_f32, "hs16": gru_seq_bwd_hs_f32<16>; both followed by gru_sum_rows_f32."""
    assert mode in ("general", "hs16")
    return _bwd32(P, dout, dh_last, h0, out, saved, mode, mutation, at)


def _terms32(P, h0, emu, mode, dout, dh_last, mutation=None, at=-1):
    """Forward and backward in float32 and every quantity's terms; a forward mutation leaves the backward alone and the reverse."""
    fwd_mut = mutation in ("swap_rz", "drop_last_k", "bias_outside", "swapped_update")
    fm, bm = (mutation, None) if fwd_mut else (None, mutation)
    if emu:
        out, saved = _emu_forward(P, h0, fm, at)
        dgi, _, dw, db, dhl, dh0s = _emu_backward(P, dout, dh_last, h0, out, saved, mode, bm, at)
    else:
        out, saved = _fwd32(P, h0, False, fm, at)
        dgi, _, dw, db, dhl, dh0s = _bwd32(P, dout, dh_last, h0, out, saved, "torch", bm, at)
    terms = _forward_terms(P, h0, out, saved)
    terms.update(_backward_terms(P, dout, h0, out, saved, dgi, dhl, dh0s))
    terms.update(_weight_terms(P, h0, out, saved, dgi, dw, db))
    return terms


def _argument_sets(P):
    """(h0, dout, dh_last): with and without h0, and the two null-gradient branches of the C entry point."""
    return [(P.h0, P.dout, P.dh_last), (None, P.dout, P.dh_last), (P.h0, None, P.dh_last), (P.h0, P.dout, None)]


# ---- CPU: the checker accepts the reference-only evaluations -------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_checker_accepts_float32_torch_and_the_emulation(case):
    hs, general, t, b = case
    for regime in REGIMES:
        P = _problem(hs, t, b, regime)
        for h0, dout, dh_last in _argument_sets(P):
            for emu in (False, True):
                _check_terms("cpu", _terms32(P, h0, emu, _mode(hs, general), dout, dh_last),
                             f"{_cid(case)} {regime} {'emulation' if emu else 'float32 torch'}")


# ---- CPU: the checker rejects what it must ---------------------------------------------------------------------------------------
MUTATIONS = [("drop_last_k", "an"), ("swap_rz", "r"), ("swap_rz", "z"), ("bias_outside", "n"), ("swapped_update", "out"),
             ("hprev_of_step_t", "dz_pre"), ("hprev_of_step_t", "dw_hh"), ("no_dh_z", "dh0"), ("gn_without_r", "dh0"),
             ("gn_without_r", "dw_hh"), ("gn_without_r", "db_hh"), ("db_row_missing", "db_hh"), ("stale_dw_entry", "dw_hh")]


@pytest.mark.parametrize("emu", [False, True], ids=["float32_torch", "emulation"])
@pytest.mark.parametrize("mutation,quantity", MUTATIONS)
@pytest.mark.parametrize("shape", REJECT, ids=lambda s: f"h{s[0]}-T{s[1]}-B{s[2]}")
def test_checker_rejects_one_wrong_step(shape, mutation, quantity, emu):
    """Each fault in ONE step (the last: its hprev is a computed state, not h0) of an otherwise correct float32 evaluation, or in
    one term of the sums over the batch, is rejected by the quantity named -- and the same evaluation without it is accepted."""
    hs, t, b = shape
    P = _problem(hs, t, b, "init")
    what = f"h{hs} T{t} B{b} {mutation}"
    _check_terms("cpu", _terms32(P, P.h0, emu, _mode(hs, False), P.dout, P.dh_last), what + " (unmutated)")
    _rejected(_terms32(P, P.h0, emu, _mode(hs, False), P.dout, P.dh_last, mutation, at=t - 1), quantity, what)


# ---- the free-running layers: float64 nn.GRU ------------------------------------------------------------------------------------
class Free:
    """Two nn.GRU layers in float64 on the CPU, outputs and h_n both carrying gradients; `grads` in named_parameters' order."""

    def __init__(self, hs, inp, b, t, with_h0):
        with torch.random.fork_rng():
            torch.manual_seed(7919 * hs + 31 * inp + with_h0)
            self.module = torch.nn.GRU(input_size=inp, hidden_size=hs, num_layers=2, batch_first=True)
        g = torch.Generator().manual_seed(hs + inp + 5 * with_h0)
        self.x, self.h0 = torch.randn(b, t, inp, generator=g), (torch.tanh(torch.randn(2, b, hs, generator=g)) if with_h0 else None)
        self.d_out, self.d_hn = torch.randn(b, t, hs, generator=g), torch.randn(2, b, hs, generator=g)
        self.ref = self.run(lambda m, x, h0: m(x, h0), torch.float64, "cpu")

    def run(self, fn, dtype, device):
        """-> {name: tensor} of fn(module, x, h0) -> (out, h_n) and the gradients of sum(out d_out) + sum(h_n d_hn)."""
        mod = torch.nn.GRU(input_size=self.module.input_size, hidden_size=self.module.hidden_size, num_layers=2, batch_first=True)
        mod.load_state_dict(self.module.state_dict())
        mod = mod.to(dtype).to(device)
        x = self.x.to(dtype).to(device).requires_grad_(True)
        h0 = None if self.h0 is None else self.h0.to(dtype).to(device).requires_grad_(True)
        out, hn = fn(mod, x, h0)
        (out * self.d_out.to(dtype).to(device)).sum().add((hn * self.d_hn.to(dtype).to(device)).sum()).backward()
        res = {"out": out, "h_n": hn, "dx": x.grad}
        if h0 is not None:
            res["dh0"] = h0.grad
        res.update({f"d {k}": p.grad for k, p in mod.named_parameters()})
        return {k: _d(v) for k, v in res.items()}


@functools.lru_cache(maxsize=2)
def _free(hs, inp, b, t, with_h0):
    return Free(hs, inp, b, t, with_h0)


def _check_free(family, got, ref, what):
    for k in ref:
        rel = _rel(got[k], ref[k])
        WORST[(family, "free " + k.split("_l")[0])] = max(WORST.get((family, "free " + k.split("_l")[0]), 0.0), rel / FREE_TOL)
        print(f"[{family}] {what} {k}: relative norm {rel:.3e}")
        _within(torch.tensor([rel], dtype=F64), torch.zeros(1, dtype=F64), torch.ones(1, dtype=F64), tol=FREE_TOL, what=f"{family} {what} {k} (relative norm)")


@pytest.mark.parametrize("case", FREE_CASES, ids=lambda c: f"h{c[0]}-in{c[1]}-B{c[2]}-T{c[3]}")
def test_free_running_tolerance_accepts_float32_nn_gru(case):
    for with_h0 in (True, False):
        fr = _free(*case, with_h0)
        _check_free("cpu", fr.run(lambda m, x, h0: m(x, h0), torch.float32, "cpu"), fr.ref, f"float32 nn.GRU h0 {with_h0}")


# ---- GPU helpers -----------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


def _dev(t, device):
    return None if t is None else t.to(device)


def _gpu_chain(K, dout, dh_last, h0, out, saved, w):
    """T one-step calls: t_len = 1, dh_last = the previous call's dh0, h0 = hprev, the contiguous slices of step t
    -> (dgi, dh0, dhl, dh0s)."""
    b, T, hs = out.shape
    cur = dh_last
    dgi, dhl, dh0s = [None] * T, [None] * T, [None] * T
    for t in reversed(range(T)):
        hp = out[:, t - 1].contiguous() if t > 0 else h0
        d_t = None if dout is None else dout[:, t:t + 1].contiguous()
        dhl[t] = cur if cur is not None else torch.zeros(b, hs, device=out.device)
        g_t, cur, _, _ = K.gru_seq_bwd(d_t, cur, hp, out[:, t:t + 1].contiguous(), saved[:, t:t + 1].contiguous(), w, True)
        dgi[t], dh0s[t] = g_t[:, 0], cur
    return torch.stack(dgi, 1), cur, torch.stack(dhl, 1), torch.stack(dh0s, 1)


def _gpu_case(P, family, device, what):
    """Forward and backward of one problem on the GPU at every argument set -> the forward's (out, saved) with h0 and without."""
    K = _ops()
    w, bias, gi = P.w.to(device), P.bias.to(device), P.gi.to(device)
    forwards = {}
    for h0c, doutc, dh_lastc in _argument_sets(P):
        tag = f"{what} h0 {h0c is not None} dout {doutc is not None} dh_last {dh_lastc is not None}"
        h0, dout, dh_last = _dev(h0c, device), _dev(doutc, device), _dev(dh_lastc, device)
        out, saved = K.gru_seq_fwd(gi, h0, w, bias)
        forwards.setdefault(h0c is not None, (out, saved))
        _check_terms(family, _forward_terms(P, h0c, out, saved), tag)
        dgi, dh0, dw, db = K.gru_seq_bwd(dout, dh_last, h0, out, saved, w, True)
        c_dgi, c_dh0, dhl, dh0s = _gpu_chain(K, dout, dh_last, h0, out, saved, w)
        _same_bits(dgi, c_dgi, f"{tag}: dgi of the T-step call against the chain of one-step calls")
        _same_bits(dh0, c_dh0, f"{tag}: dh0 of the T-step call against the chain of one-step calls")
        _check_terms(family, _backward_terms(P, doutc, h0c, out, saved, dgi, dhl, dh0s), tag)
        _check_terms(family, _weight_terms(P, h0c, out, saved, dgi, dw, db), tag)
        again = K.gru_seq_bwd(dout, dh_last, h0, out, saved, w, True)
        for name, x, y in zip(("dgi", "dh0", "dw_hh", "db_hh"), (dgi, dh0, dw, db), again):
            _same_bits(x, y, f"{tag}: {name} across two calls")
        no_dh0 = K.gru_seq_bwd(dout, dh_last, h0, out, saved, w, False)
        assert no_dh0[1] is None
        for name, x, y in zip(("dgi", "dw_hh", "db_hh"), (dgi, dw, db), (no_dh0[0], no_dh0[2], no_dh0[3])):
            _same_bits(x, y, f"{tag}: {name} with need_dh0=False")
    return forwards


# ---- GPU: every kernel per element -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_gru_kernels_per_element(case, device, monkeypatch):
    """gru_seq_{fwd,bwd}_f32, or at hidden 16 without PV_GRU_GENERAL gru_seq_{fwd,bwd}_hs_f32<16>, + gru_sum_rows_f32."""
    hs, general, t, b = case
    if general:
        monkeypatch.setenv("PV_GRU_GENERAL", "1")
    family = "hs16" if _mode(hs, general) == "hs16" else ("general h<=32" if hs <= 32 else "general h>32")
    for regime in REGIMES:
        _gpu_case(_problem(hs, t, b, regime), family, device, f"{_cid(case)} {regime}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + [LONG], ids=lambda s: f"T{s[0]}-B{s[1]}")
def test_registers_kernels_against_the_general_kernels(shape, device, monkeypatch):
    """gru_seq_*_hs_f32<16> against gru_seq_*_f32 at hidden 16: out and saved bitwise at every (T, batch); at T = 1 dgi, dW_hh and
    db_hh bitwise, as the source's comment claims (beyond one step dh_prev, summed in another order, feeds the next step's dgi)."""
    K = _ops()
    t, b = shape
    for regime in REGIMES:
        P = _problem(16, t, b, regime)
        w, bias, gi, h0 = P.w.to(device), P.bias.to(device), P.gi.to(device), P.h0.to(device)
        dout, dh_last = P.dout.to(device), P.dh_last.to(device)
        res = []
        for general in (False, True):
            if general:
                monkeypatch.setenv("PV_GRU_GENERAL", "1")
            out, saved = K.gru_seq_fwd(gi, h0, w, bias)
            res.append((out, saved) + tuple(K.gru_seq_bwd(dout, dh_last, h0, out, saved, w, True)))
            monkeypatch.delenv("PV_GRU_GENERAL", raising=False)
        for name, x, y in zip(("out", "saved", "dgi", "dh0", "dw_hh", "db_hh"), *res):
            if name in ("out", "saved") or (t == 1 and name != "dh0"):
                _same_bits(x, y, f"T{t} B{b} {regime}: {name} of the <16> kernels against the general kernels")


# ---- GPU: the device's expf and tanhf --------------------------------------------------------------------------------------------
def _function_arguments():
    """The arguments the cases hand to expf (-x of both sigmoids) and tanhf, from the float32 torch forward on the CPU."""
    ex, th = [], []
    for hs, general, t, b in CASES:
        if general:
            continue
        for regime in REGIMES:
            P = _problem(hs, t, b, regime)
            for h0 in (P.h0, None):
                out, saved = _fwd32(P, h0, False)
                hprev = _hprev(h0, out)
                a = hprev @ P.w.t() + P.bias
                ex.append(-(P.gi[..., :2 * hs] + a[..., :2 * hs]).flatten())
                th.append((P.gi[..., 2 * hs:] + saved[..., :hs] * saved[..., 3 * hs:]).flatten())
    return torch.cat(ex), torch.cat(th)


def _ulps(fn, x, device):
    """Worst |fn(x) on the device - fn(x) in float64| in units of 2^-23 |value|, over the normal results."""
    ref = fn(x.double())
    got = fn(x.to(device)).double().cpu()
    ok = ref.abs() >= TINY
    return float(((got - ref).abs() / (ULP * ref.abs()))[ok].max())


@pytest.mark.gpu
def test_device_math_functions_are_within_F(device):
    """torch's own elementwise exp and tanh on the GPU against float64 over the arguments of every case: F = 2 x the worst."""
    ex, th = _function_arguments()
    for name, fn, x, f in (("exp", torch.exp, ex, F_EXP), ("tanh", torch.tanh, th, F_TANH)):
        worst = _ulps(fn, x, device)
        print(f"device {name}: worst error {worst:.3f} ulps over {x.numel()} arguments in [{float(x.min()):.2f}, {float(x.max()):.2f}] -> F = {2 * worst:.2f}")
        assert f <= F_MAX, f"F of {name} is {f}: above {F_MAX}, the bounds of this file no longer say anything"
        assert 2 * worst <= f, f"device {name}: 2 x {worst:.3f} ulps exceeds F = {f}"


# ---- GPU: refusals and sentinels through the C ABI -------------------------------------------------------------------------------
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

    def untouched(self):
        return bool((_bits(self.buf.cpu()) == _bits(torch.tensor([SENTINEL]))).all())


def _abi():
    from predict_pv_yield_amd import _lib
    return _lib.get_lib(), _lib.ptr, _lib.current_stream_ptr


@pytest.mark.gpu
def test_refusals_return_the_error_and_write_nothing(device):
    """hidden = 65 and hidden = 0: the size error (-2); a workspace one byte short: the argument error (-1); no output written."""
    lib, ptr, stream = _abi()
    b, t, big = 2, 3, GRU_MAXH + 1
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    gi, h0, w, bias, dout = z(b, t, 3 * big), z(b, big), z(3 * big, big), z(3 * big), z(b, t, big)
    out, saved = Guarded((b, t, big), device), Guarded((b, t, 4 * big), device)
    dgi, dh0, dw, db = Guarded((b, t, 3 * big), device), Guarded((b, big), device), Guarded((3 * big, big), device), Guarded((3 * big,), device)
    ws = torch.empty(b * (3 * big * big + 3 * big) * 4, dtype=torch.uint8, device=device)
    for hidden in (big, 0):
        assert lib.pv_gru_seq_fwd_f32(ptr(gi), ptr(h0), ptr(w), ptr(bias), ptr(out.t), ptr(saved.t), b, t, hidden, stream()) == -2
        assert "hidden" in lib.pv_last_error().decode()
        assert lib.pv_gru_seq_bwd_f32(ptr(dout), ptr(h0), ptr(h0), ptr(gi), ptr(gi), ptr(w), ptr(dgi.t), ptr(dh0.t), ptr(dw.t), ptr(db.t),
                                      b, t, hidden, ptr(ws), ws.numel(), stream()) == -2
    hs = GRU_MAXH
    need = b * (3 * hs * hs + 3 * hs) * 4
    assert lib.pv_gru_seq_bwd_f32(ptr(dout), ptr(h0), ptr(h0), ptr(gi), ptr(gi), ptr(w), ptr(dgi.t), ptr(dh0.t), ptr(dw.t), ptr(db.t),
                                  b, t, hs, ptr(ws), need - 1, stream()) == -1
    assert "workspace" in lib.pv_last_error().decode()
    torch.cuda.synchronize()
    for name, g in (("out", out), ("saved", saved), ("dgi", dgi), ("dh0", dh0), ("dw_hh", dw), ("db_hh", db)):
        assert g.untouched(), f"a refused call wrote {name}"


@pytest.mark.gpu
@pytest.mark.parametrize("hs", [7, 64])
def test_outputs_stay_inside_their_buffers(hs, device):
    """(T, batch) = (2, 3): out, saved, dgi, dh0, dw_hh, db_hh each inside a sentinel-filled buffer, handed over through the C ABI."""
    K = _ops()
    lib, ptr, stream = _abi()
    t, b = 2, 3
    P = _problem(hs, t, b, "init")
    gi, h0, w, bias, dout, dh_last = (x.to(device) for x in (P.gi, P.h0, P.w, P.bias, P.dout, P.dh_last))
    out, saved = Guarded((b, t, hs), device), Guarded((b, t, 4 * hs), device)
    dgi, dh0, dw, db = Guarded((b, t, 3 * hs), device), Guarded((b, hs), device), Guarded((3 * hs, hs), device), Guarded((3 * hs,), device)
    ws = Guarded((b * (3 * hs * hs + 3 * hs),), device)
    K.check(lib.pv_gru_seq_fwd_f32(ptr(gi), ptr(h0), ptr(w), ptr(bias), ptr(out.t), ptr(saved.t), b, t, hs, stream()), "pv_gru_seq_fwd_f32")
    K.check(lib.pv_gru_seq_bwd_f32(ptr(dout), ptr(dh_last), ptr(h0), ptr(out.t), ptr(saved.t), ptr(w), ptr(dgi.t), ptr(dh0.t), ptr(dw.t), ptr(db.t),
                                   b, t, hs, ptr(ws.t), ws.t.numel() * 4, stream()), "pv_gru_seq_bwd_f32")
    torch.cuda.synchronize()
    for name, g in (("out", out), ("saved", saved), ("dgi", dgi), ("dh0", dh0), ("dw_hh", dw), ("db_hh", db), ("workspace", ws)):
        assert g.intact(), f"written outside {name}"
    family = "guarded"
    _check_terms(family, _forward_terms(P, P.h0, out.t, saved.t), f"h{hs}")
    _check_terms(family, _weight_terms(P, P.h0, out.t, saved.t, dgi.t, dw.t, db.t), f"h{hs}")
    ref = K.gru_seq_bwd(dout, dh_last, h0, out.t.clone(), saved.t.clone(), w, True)
    for name, x, y in zip(("dgi", "dh0", "dw_hh", "db_hh"), (dgi.t, dh0.t, dw.t, db.t), ref):
        _same_bits(x, y, f"h{hs}: guarded {name} against the call through hip_ops (checked per element in test_gru_kernels_per_element)")


# ---- GPU: two layers, free-running -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", FREE_CASES, ids=lambda c: f"h{c[0]}-in{c[1]}-B{c[2]}-T{c[3]}")
def test_two_layers_free_running(case, device):
    """PF.gru (input projections through PF.linear, or linear_f32 at width 2048) against float64 nn.GRU: relative norm per tensor."""
    from predict_pv_yield_amd import perceiver_functional as PF
    for with_h0 in (True, False):
        fr = _free(*case, with_h0)
        _check_free("PF.gru", fr.run(lambda m, x, h0: PF.gru(x, m, h0), torch.float32, device), fr.ref, f"h0 {with_h0}")


# ---- the tables in the module docstring -----------------------------------------------------------------------------------------
def _measure():
    worst = {q: [0.0, 0.0] for q in C}
    for case in CASES:
        hs, general, t, b = case
        for regime in REGIMES:
            P = _problem(hs, t, b, regime)
            for h0, dout, dh_last in _argument_sets(P):
                for emu in (False, True):
                    for q, (got, c64, s, _) in _terms32(P, h0, emu, _mode(hs, general), dout, dh_last).items():
                        worst[q][emu] = max(worst[q][emu], _ratio(got, c64, U32 * s))
    print("    quantity   float32 torch   emulation   constant (4 x the worse)")
    for q, (t32, emu) in worst.items():
        print(f"    {q:<10} {t32:8.2f}      {emu:8.2f}      {4 * max(t32, emu):6.1f}")
    print("C = {" + ", ".join(f'"{q}": {math.ceil(40 * max(v)) / 10}' for q, v in worst.items()) + "}")
    rels = {}
    for case in FREE_CASES:
        for with_h0 in (True, False):
            fr = _free(*case, with_h0)
            got = fr.run(lambda m, x, h0: m(x, h0), torch.float32, "cpu")
            for k in fr.ref:
                kind = k.split("_l")[0]
                rels[kind] = max(rels.get(kind, 0.0), _rel(got[k], fr.ref[k]))
    for kind, rel in rels.items():
        print(f"    float32 nn.GRU against float64 nn.GRU, {kind:<12} worst relative norm {rel:.3e}")
    print(f"FREE_TOL = 4 x {max(rels.values()):.3e} = {4 * max(rels.values()):.3e}")


if __name__ == "__main__":
    _measure()
