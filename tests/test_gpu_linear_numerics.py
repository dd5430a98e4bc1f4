"""The fully-connected and Adam kernels -- csrc/linear_bf16.hip, dense_f32.hip, linear_f32_skinny.hip, adam.h -- per element against
float64, at the shapes where each of their launch rules and tiles begins and ends, and CPU tests that show the checker rejects a
kernel that is subtly wrong.  Vocabulary and manner: tests/test_gpu_gemm_numerics.py.  Shapes are written (m, n, k): x [m, k],
w [n, k], y and dy [m, n].

Reference (`Problem`, float64 on the CPU).  c64 is the float64 result of the operands as the kernel receives them (bf16 operands as
stored; the one-pass and the K-sharded kernel multiply dx by their PRE-update master weights rounded to bf16, so their dx reference
does too); dy is gated in float64 by y > 0 (false for 0.0 and -0.0, true for 2^-126); S is the float64 sum of the absolute terms,
plus |bias|.

Bounds, per element, never a norm and never a maximum over the tensor (`_check`, through conv2d_f32_helpers._within):
    f32 outputs (y, f32 dw, db, f32 dx)                                  |c - c64| <= C 2^-24 S
    bf16 outputs of kernels that take g in f32 (linear_bwd_dx_bf16_kernel,
      linear_bwd_dw_bf16_kernel<2>)                                      ... + 2^-8 |c64|   (bfloat16's unit roundoff)
    bf16 outputs of kernels that take g as a bf16 hi + lo pair
      (linear_bwd_dx_bf16_v2_kernel, one-pass and tall dx,
      linear_wgrad_bf16out_mfma_kernel)                                  ... + C_pair 2^-16 S
Adam (`_adam64`: adam.h's four lines in float64 on the same f32 p, m, v, g and the scalars built as adam_scalars builds them, in
double, narrowed to f32): each of p, m, v within C_adam 2^-24 x the sum of the absolute terms of its own line
    m: |m| + (1 - b1)(|g| + |m|)     v: |v b2| + |(1 - b2) g g|     p: |p| + |step_size m / denom|
and the bf16 shadow bitwise p.to(bfloat16).
Fused kernels (wgrad_adam_bf16, wgrad_adam_f32, one-pass, one-pass _dev, tall): m and v against float64 Adam on the float64
gradient, the gradient's own bound B_g = C 2^-24 S_g propagated through the two lines -- (1 - b1) B_g for m,
(1 - b2)(2 |g64| B_g + B_g^2) for v -- plus the Adam term above; p within |dp/dg| B_g (float64 autograd, elementwise) plus its Adam
term.  Starting moments are non-zero with v0 >= 1e-8 so that p is a smooth function of g; a float32 evaluation (float32 torch
gradient and the emulated gradient, then adam.h's lines in float32) stays within these bounds at every case of this file
(test_checker_accepts_float32_adam_on_both_gradients).

Regimes: `zero_mean` (randn) at every shape; `positive` (|randn|) only where the contraction (k forward, n for dx, m for dw and
db) is <= 128 long, for the reason given in the GEMM file.

Constants.  From the REFERENCE's own error, never from the kernels: 4 x the worst error / (unit x S) of reference-only evaluations
of every (family, shape, regime) of this file -- float32 torch, and `_emu_*`, the arithmetic the kernel comments document:
16-deep matrix steps into one f32 accumulator (the register-tiled forward's k-permutation inside a 64-block, v3's 128-column
tiles), the workgroups' slabs added in linear_reduce_bf16path's order (four groups of slabs g, g + 4, ... over four running sums,
(s0 + s1) + (s2 + s3) per group, then (0 + 1) + (2 + 3)); g split into RNE hi + RNE lo of the remainder (hi then lo in
linear_bwd_dx_bf16_v2_kernel, lo then hi elsewhere); the tall kernel's exact three-term split, smallest term first, x grad_scale;
the vector-ALU kernels' fma chains in index order; dense_f32.hip's forward (four strided sums; lanes, shuffle tree, waves, slabs in
order; the GEMM route through the GEMM file's emulation); the skinny kernels' two-deep f32 matrix steps and eight-group reduce.
`python tests/test_gpu_linear_numerics.py` prints the table (worst per family; float32 torch / emulation, and the split alone):
    family (kernel)                                   zero_mean        positive
    fwd_rt    linear_fwd_bf16_kernel                   1.32 / 0.65      1.55 / 1.66
    fwd_v3    linear_fwd_bf16_v3_kernel                1.60 / 0.75      7.96 / 3.42
    dx_rt     linear_bwd_dx_bf16_kernel, db            3.58 / 3.58      4.23 / 4.23
    dx_v2     linear_bwd_dx_bf16_v2_kernel, db         5.74 / 2.65      9.41 / 4.99      split 0.24 / 0.23 x 2^-16 S
    wg_f32    linear_bwd_dw_bf16_kernel<0>             4.45 / 4.45      7.41 / 7.41
    wg_b16    <2> / linear_wgrad_bf16out_mfma_kernel   4.48 / 4.48      7.68 / 7.68      split 0.41 / 0.47
    one_pass  linear_bwd_dw_dx_adam_kernel (dw, dx)    3.81 / 3.37      4.80 / 4.80      split 0.37 / 0.42
    tall      linear_bwd_dw_dx_adam_tall_kernel        4.43 / 3.15      7.40 / 4.52      split 0.40 / 0.38
    f32_fwd   dense_f32.hip forward, skinny forward    3.20 / 2.26      4.75 / 2.60
    f32_bwd   linear_bwd_dx_body / _dw_body            4.78 / 4.78      8.55 / 8.55
    f32_wgrad_adam  linear_bwd_dw_bf16_kernel<1, float> 4.51 / 4.51     6.13 / 6.13
    skinny_dx linear_dx_f32_skinny_kernel              5.58 / 4.62     11.34 / 10.27
    (float32 torch and the fma chains agree to the digit where the contraction is short: the CPU library adds in index order too)
    worst zero_mean: float32 torch 5.74, emulation 4.78 -> C["zero_mean"] = 23.0
    worst positive:  float32 torch 11.34, emulation 10.27 -> C["positive"] = 45.4
    worst split alone: 0.467 x 2^-16 S -> C_pair = 1.87
    adam.h's lines in float32 torch, over ADAM_CASES x ADAM_SIZES and the fused cases' gradients, worst error / (2^-24 x the line's
    sum of absolute terms): p 12.69, m 2.58, v 2.78 -> C_adam = 50.8 for p, 10.4 for m, 11.2 for v (one constant per line: the
    issue's single C_adam would be p's 50.8 for all three; p's own line is where the rounding of m and v arrives divided by a
    denominator that can be small against |p|)

What the checker is sensitive to (CPU tests below, at the small-contraction REJECT shapes).  It rejects, applied to one element
or one tile of a correct result: the last contraction term dropped; the gate taken as y >= 0; the gate read one column off; the
bias added twice or not at all; the last 8-column chunk of a row left at zero; a row computed from the previous row's g; a missing
split-K slab; the third term of the tall kernel's split dropped (seen in m); Adam with p formed from the moment read before its
update while v is already updated; Adam with eps inside the square root.
What it cannot see: a dropped lo term behind a bf16 result -- the error, about 2^-9 of each product, is smaller than the bf16
rounding term 2^-8 |c64| wherever the result does not cancel.  Measured at (32, 128, 256)
(test_dropped_lo_term_is_below_the_bf16_rounding_of_most_elements): error 2^-12.1 S (median) against a rounding term of 2^-10.9 S
for `zero_mean`, 2^-12.3 S against 2^-8.0 S for `positive`; `positive`: 0.2 % of the elements exceed the bound, the worst by 1.09
-- invisible; `zero_mean`: 26 % of the elements, those whose sum cancels, the worst 30 x the bound -- a whole tensor with the
fault is rejected, the same fault in one element passes three times out of four.  Nor can it see a read outside an operand whose
value is discarded (the ragged tail of linear_fwd_bf16_kernel read bytes 64 .. 79 of a 16-byte row at k = 8 until this file
was written: found by reading, fixed in the source, no result changed), or which of two bitwise-equal schedules ran.

GPU cases (tiles read from the sources).
  1 bf16 forward, register-tiled, linear_fwd_bf16_kernel<MT> (n not in {32, 48, ..., 128}): 4 waves x 32 outputs per column block
    (grid.y = ceil(n / 128)), MT = ceil(m / 32) row tiles, 64-deep k-blocks, bf16_fwd_split: min(blocks, 1024) workgroups.
    FWD_RT: (1,1,8); (7,5,72) ragged 64-block; (33,16,136), (65,24,200), (128,31,1032) MT = 2, 3, 4 with a ragged last row tile;
    (5,130,264) second column block with two live columns; (2,16,65608) 1026 k-blocks = two per workgroup, the last ragged;
    (129,16,136) 128 + 1 rows through hip_ops.  Without bias, with bias, with bias and ReLU.
  2 bf16 forward, linear_fwd_bf16_v3_kernel<MB> (n in {32, ..., 128 step 16}): 128-column tiles, v3_split: min(tiles, 256)
    workgroups; MB = 1 (m <= 32), 2 (<= 128: rows 64 per launch), 4 (> 128: 128 per launch).  FWD_V3: (1,32,8), (32,128,128),
    (31,48,136), (5,128,840); (33,64,392), (64,128,2440); (129,96,264) second launch of one row, (200,32,904); (17,96,32904) two
    tiles per workgroup, (3,128,65544) three.
  3 bf16 dx.  linear_bwd_dx_bf16_kernel (BT = 16 rows, 8 columns per thread, 256 threads = 2048 columns per k-block, xcd_tile
    order): DX_RT (1,1,8), (7,5,72), (17,16,136) second row tile of one row, (40,24,2056) second k-block of one thread,
    (3,8,16392) nine k-blocks over the eight-XCD order.  linear_bwd_dx_bf16_v2_kernel (256-column tiles, v2_split: min(tiles, 512)
    workgroups, 32 rows per launch): DX_V2 (1,32,8), (32,128,256), (31,48,264), (5,128,840), (17,96,131080) two tiles per
    workgroup, (33,64,520), (72,128,264) blocks of 32 rows.  Each with and without mask, with and without gate_dx_by_x
    (gate_bf16_by_relu_kernel); db from the v2 kernel (m <= 32), linear_bwd_db_bf16path (all others) and the one-pass kernel (5).
  4 bf16 weight gradient.  f32 out (linear_bwd_dw_bf16_kernel<0>, BT = 16 outputs): WG_F32.  bf16 out: PV_WGRAD_BF16OUT_VALU=1
    (read per call; <2>) and linear_wgrad_bf16out_mfma_kernel (m <= 64, n <= 128; 128-column tiles, min(tiles, 512) persistent
    workgroups): WG_B16 (16,24,4096), (64,128,2048), (7,40,1000), (33,100,136), (16,32,65672) 514 tiles: the loop's second trip,
    last tile of 8 columns; (70,128,1024) beyond 64 rows: vector ALU either way.
  5 one-pass backward linear_bwd_dw_dx_adam_kernel (m <= 32, n <= 128, n % 8 == 0; 128 columns per workgroup; thread (kq, rg) =
    8 rows x 8 columns), host and device scalars: ONE_PASS (1,8,8), (32,128,128), (7,128,1032), (32,16,4096), (31,120,392):
    dx, db, p, m, v, shadow; moments_tiled where k % 128 == 0; PV_FC1_FETCH=late|early1|early2; bitwise fused == two-pass,
    one-pass == fused, dev == host, tiled == rows, variants == default.
  6 K-sharded backward linear_bwd_dw_dx_adam_tall_kernel (row blocks of 32): TALL (1,8,8), (32,128,128), (33,8,136), (72,16,704),
    (95,120,392), (256,128,264); grad_scale 0.125; with and without gate_dx_by_x; moments_tiled.
  7 f32 dense head.  linear_fwd_small_f32 (k <= 4096 and m n <= 65536): (1,1,1), (3,6,64), (4,7,37) rows not 16-byte aligned,
    (41,41,133) 64-, 32-, 4- and 1-deep stages, (5,128,1000), (32,64,4096).  linear_fwd_tile_f32 (k % 4 == 0, aligned): (257,256,8),
    (9,9,4100), (2,16,34816); (8,8,8196) with x one element into its buffer goes to linear_fwd_partial_f32, as do (9,3,4097) and
    (2,5,16390); (3,5,65540) goes to pv_gemm_f32 (k >= 65536).  linear_bwd_small_f32 (one launch; dx_body's 32-, 8-, 1-column
    stages at n = 41, dw_body's 32-row stage and remainder at m = 41, 40): (1,1,1), (41,41,133), (40,9,257), (5,128,1000); separate
    linear_bwd_dx_f32 / _dw_f32 / _db_f32: (2,16,34816), (33,41,4100), (5,128,1000) with need_dx=False.  With and without mask.
    linear_bwd_dw_bf16_kernel<1, float> (wgrad_adam_f32): (5,24,1032), (40,17,136), (32,128,8192).
  8 f32 skinny (k >= 65536, k % 128 == 0): (1,8,65536), (32,128,65536), (5,100,65664): LDS forward, direct forward
    (PV_LINEAR_F32_SKINNY_DIRECT=1), dx.
  9 Adam: sizes 1, 3, 1027, 4101; steps 1, 2, 1000; grad_scale 1 and 0.125; with and without shadow; gradients holding exact zeros,
    1e-12 and 1e4; adam_step, adam_step_multi, adam_step_multi_dev, adam_step_bf16grad.
 10 sentinels: one ragged shape per entry point, every output inside a buffer filled with 1.2345678e30 and handed over through the
    C ABI; the elements outside the result keep their bits.
Gates: every masked case plants 0.0, -0.0 and 2^-126 in y, every gate_dx_by_x case +0 and -0 in x: first and last row and column
and one each side of every tile edge (8, 16, 32, 64, 96, 128 columns of y; 8, 16, 32, 64, 128 rows; 8, 32, 64, 128, 256, k - 8 columns
of x).  Where x gates, dx is an exact zero.
Not covered: linear_fwd_bf16_v2_kernel is launched only when the weight exceeds 4 GB (`fits32` in pv_linear_fwd_bf16); no shape of a
few seconds reaches it.

Measured on the MI355X with these constants, worst error / bound over all cases per kernel: bf16 forward register-tiled 0.04,
v3 0.09; bf16 dx register-tiled 0.995, v2 0.99, one-pass 0.98, tall 0.985 and bf16 dw vector ALU 0.996, matrix cores 0.99 (each
the bf16 rounding term alone: a value half a step from both neighbours at the bottom of its binade, as in the GEMM file); bf16
dw f32 out 0.25; db from the v2 kernel 0.10, linear_bwd_db_bf16path 0.12, one-pass 0.12; p / m / v of the fused bf16 kernel and
the one-pass kernel 0.18, tall 0.17, f32 wgrad + Adam 0.20; f32 forward small 0.05, tile 0.10, partial 0.005, GEMM route 0.008;
f32 backward in one launch dx 0.24, dw 0.15, db 0.09, separate kernels dx 0.17, dw 0.21, db 0.08; skinny forward 0.005 (both forms),
skinny dx 0.25; Adam single, multi, multi-dev 0.23, bf16 gradient 0.25.  The CPU evaluations' own worst is 0.25 of the bound by
construction: every f32 figure stays within 1.1 x that.  Every bitwise relation held.  No case found a fault in the kernels' results.  The 90 GPU cases of
this file take 5 s together, the slowest ((17, 96, 131080), dx and db) 0.8 s; the 186 CPU cases take 6 s.
"""
import ctypes
import functools
import math

import pytest
import torch

from conv2d_f32_helpers import _ops, _within

U32 = 2.0 ** -24
U16 = 2.0 ** -8          # unit roundoff of bfloat16
UPAIR = 2.0 ** -16       # the unit of the hi + lo split
SENTINEL = 1.2345678e30
GUARD = 64               # sentinel elements on either side of an output (keeps 16-byte alignment for f32 and bf16)
TINY = 2.0 ** -126

# 4 x the reference-only ratios printed by `python tests/test_gpu_linear_numerics.py` (module docstring)
C = {"zero_mean": 23.0, "positive": 45.4}
C_PAIR = 1.87
C_ADAM = {"p": 50.8, "m": 10.4, "v": 11.2}      # per line of adam_update

REGIMES = ("zero_mean", "positive")
POSITIVE_MAX = 128
LR, BETAS, EPS = 5e-4, (0.9, 0.999), 1e-8

FWD_RT = [(1, 1, 8), (7, 5, 72), (33, 16, 136), (65, 24, 200), (128, 31, 1032), (5, 130, 264), (2, 16, 65608), (129, 16, 136)]
FWD_V3 = [(1, 32, 8), (32, 128, 128), (31, 48, 136), (5, 128, 840), (33, 64, 392), (64, 128, 2440), (129, 96, 264), (200, 32, 904),
          (17, 96, 32904), (3, 128, 65544)]
DX_RT = [(1, 1, 8), (7, 5, 72), (17, 16, 136), (40, 24, 2056), (3, 8, 16392)]
DX_V2 = [(1, 32, 8), (32, 128, 256), (31, 48, 264), (5, 128, 840), (17, 96, 131080), (33, 64, 520), (72, 128, 264)]
WG_F32 = [(1, 1, 8), (7, 5, 72), (64, 17, 2056), (32, 128, 8192)]
WG_B16 = [(16, 24, 4096), (64, 128, 2048), (7, 40, 1000), (33, 100, 136), (16, 32, 65672), (70, 128, 1024)]
ONE_PASS = [(1, 8, 8), (32, 128, 128), (7, 128, 1032), (32, 16, 4096), (31, 120, 392)]
TALL = [(1, 8, 8), (32, 128, 128), (33, 8, 136), (72, 16, 704), (95, 120, 392), (256, 128, 264)]
F32_FWD = [((1, 1, 1), "small"), ((3, 6, 64), "small"), ((4, 7, 37), "small"), ((41, 41, 133), "small"), ((5, 128, 1000), "small"),
           ((32, 64, 4096), "small"), ((257, 256, 8), "tile"), ((9, 9, 4100), "tile"), ((2, 16, 34816), "tile"),
           ((8, 8, 8196), "partial_misaligned"), ((9, 3, 4097), "partial"), ((2, 5, 16390), "partial"), ((3, 5, 65540), "gemm")]
F32_BWD_SMALL = [(1, 1, 1), (41, 41, 133), (40, 9, 257), (5, 128, 1000)]
F32_BWD_SEP = [((2, 16, 34816), True), ((33, 41, 4100), True), ((5, 128, 1000), False)]
F32_WGRAD_ADAM = [(5, 24, 1032), (40, 17, 136), (32, 128, 8192)]
SKINNY = [(1, 8, 65536), (32, 128, 65536), (5, 100, 65664)]
ADAM_SIZES = [1, 3, 1027, 4101]
ADAM_CASES = [(step, scale) for step in (1, 2, 1000) for scale in (1.0, 0.125)]
REJECT = [(7, 16, 72), (17, 24, 136), (31, 48, 264)]          # contraction <= 128 in every direction, every k a multiple of 8


def _regimes(contraction):
    return [r for r in REGIMES if r == "zero_mean" or contraction <= POSITIVE_MAX]


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---- inputs and the float64 reference ------------------------------------------------------------------------------------------
def _edges(size, marks):
    idx = {0, size - 1}
    for e in marks:
        if 0 < e < size:
            idx |= {e - 1, e}
    return sorted(idx)


def _plant(t, values, col_marks):
    """The given values, in turn, at first and last row and column and either side of every tile edge."""
    rows, cols = _edges(t.shape[0], (8, 16, 32, 64, 128)), _edges(t.shape[1], col_marks)
    i = 0
    for r in rows:
        for c in cols:
            t[r, c] = values[i % len(values)]
            i += 1
    return t


class Problem:
    """Operands on the CPU (float32 holders; bf16 operands are already rounded) and their float64 references."""

    def __init__(self, m, n, k, regime, bf16, relu_x=False, dy_scale=1.0):
        g = torch.Generator().manual_seed(1000003 * m + 10007 * n + 101 * k + 7 * (regime == "positive") + bf16)
        x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
        bias, dy, y = torch.randn(n, generator=g), torch.randn(m, n, generator=g) * dy_scale, torch.randn(m, n, generator=g)
        if regime == "positive":
            x, w, bias, dy = x.abs(), w.abs(), bias.abs(), dy.abs()
        if relu_x:      # a ReLU output, with +0 and -0 where the gate's tiles begin and end
            x = x if regime == "positive" else x.relu()
            _plant(x, (0.0, -0.0), (8, 32, 64, 128, 256, k - 8))
        _plant(y, (0.0, -0.0, TINY), (8, 16, 32, 64, 96, 128))
        if bf16:
            x, w = _bf16(x), _bf16(w)
        self.m, self.n, self.k, self.regime, self.bf16 = m, n, k, regime, bf16
        self.x, self.w, self.bias, self.dy, self.y = x, w, bias, dy, y

    def dev(self, t, device):
        return t.to(torch.bfloat16).to(device) if self.bf16 else t.to(device)

    def g32(self, masked):
        return torch.where(self.y > 0, self.dy, torch.zeros(())) if masked else self.dy

    def fwd(self, bias, relu):
        c, s = self.x.double() @ self.w.double().t(), self.x.double().abs() @ self.w.double().abs().t()
        if bias:
            c, s = c + self.bias.double(), s + self.bias.double().abs()
        return (c.clamp_min(0) if relu else c), s

    def dx(self, masked, gate=False, w=None):
        g, w = self.g32(masked).double(), (self.w if w is None else w).double()
        c, s = g @ w, g.abs() @ w.abs()
        if gate:
            open_ = self.x > 0
            c, s = torch.where(open_, c, torch.zeros((), dtype=torch.float64)), torch.where(open_, s, torch.zeros((), dtype=torch.float64))
        return c, s

    def dw(self, masked, scale=1.0):
        g = self.g32(masked).double() * scale
        return g.t() @ self.x.double(), g.abs().t() @ self.x.double().abs()

    def db(self, masked):
        g = self.g32(masked).double()
        return g.sum(0), g.abs().sum(0)


@functools.lru_cache(maxsize=4)
def _problem(m, n, k, regime, bf16, relu_x=False, dy_scale=1.0):
    return Problem(m, n, k, regime, bf16, relu_x, dy_scale)


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def _bound(c64, s, c, bf16_out=False, pair=False):
    b = c * U32 * s
    if bf16_out:
        b = b + U16 * c64.abs()
    if pair:
        b = b + C_PAIR * UPAIR * s
    return b


def _ratio_to(got, c64, bound):
    got = got.detach().double().cpu()
    ratio = (got - c64).abs() / (bound + 1e-30)
    return float(torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).max()) if got.numel() else 0.0


WORST = {}      # family -> worst error / bound of a run (the MI355X figures of the docstring come from here)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the file's last test: the worst error / bound per kernel family (shown with -s)."""
    yield
    for family in sorted(WORST):
        if family != "cpu":
            print(f"worst error / bound, {family}: {WORST[family]:.3f}")


def _check_to(family, got, c64, bound, what):
    """|got - c64| <= bound, per element; prints the worst error / bound."""
    worst = _ratio_to(got, c64, bound)
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print(f"[{family}] {what}: error / bound {worst:.3f}")
    _within(got.detach().float(), c64, bound / U32, tol=U32, what=f"{family} {what}")
    return worst


def _check(family, got, c64, s, regime, what, bf16_out=False, pair=False):
    return _check_to(family, got, c64, _bound(c64, s, C[regime], bf16_out, pair), what)


def _rejected(got, c64, s, regime, what, bf16_out=False, pair=False):
    with pytest.raises(AssertionError, match="x the bound"):
        _check("cpu", got, c64, s, regime, what, bf16_out, pair)


# ---- Adam in float64 and float32 -----------------------------------------------------------------------------------------------
def _scalars(step, lr=LR, betas=BETAS, eps=EPS):
    """adam_scalars of adam.h: python floats (double), each narrowed to f32 -- returned as the doubles those f32 are."""
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    vals = (1.0 - betas[0], betas[1], 1.0 - betas[1], math.sqrt(bc2), eps, -(lr / bc1))
    return tuple(float(torch.tensor(v, dtype=torch.float64).float()) for v in vals)


def _adam_lines(p, m, v, g, sc, mutation=None):
    """adam_update of adam.h in the dtype of its arguments -> (p, m, v, S_p, S_m, S_v)."""
    a, b2, omb2, bc2s, eps, nss = sc
    m1 = m + a * (g - m)
    v1 = v * b2 + (omb2 * g) * g
    denom = (v1 / (bc2s * bc2s) + eps).sqrt() if mutation == "eps_inside" else v1.sqrt() / bc2s + eps
    upd = nss * ((m if mutation == "old_m" else m1) / denom)
    return (p + upd, m1, v1, p.abs() + upd.abs(), m.abs() + abs(a) * (g.abs() + m.abs()), (v * b2).abs() + ((omb2 * g) * g).abs())


def _adam64(p, m, v, g, sc):
    return _adam_lines(p.double(), m.double(), v.double(), g.double(), sc)


def _adam32(p, m, v, g, sc, mutation=None):
    return _adam_lines(p.float(), m.float(), v.float(), g.float(), sc, mutation)[:3]


def _dp_dg(p, m, v, g64, sc):
    g = g64.clone().requires_grad_(True)
    _adam_lines(p.double(), m.double(), v.double(), g, sc)[0].sum().backward()
    return g.grad.abs()


def _adam_state(n, k, seed=0):
    g = torch.Generator().manual_seed(77 + 13 * n + k + seed)
    return (torch.randn(n, k, generator=g) * 0.05, torch.randn(n, k, generator=g) * 1e-3, torch.rand(n, k, generator=g) * 1e-6 + 1e-8)


def _adam_check(family, got, ref, what):
    """got (p, m, v) against ref = _adam64(...): each within C_adam 2^-24 x its own line's sum of absolute terms."""
    for name, x, r, s in zip("pmv", got, ref[:3], ref[3:]):
        _check_to(family, x, r, C_ADAM[name] * U32 * s, f"{what} {name}")


def _fused_bounds(p0, m0, v0, g64, b_g, sc):
    """-> (ref, (bound_p, bound_m, bound_v)) of a kernel that applies Adam to a gradient known to within b_g."""
    ref = _adam_lines(p0.double(), m0.double(), v0.double(), g64, sc)
    a, _, omb2 = sc[0], sc[1], sc[2]
    bp = _dp_dg(p0, m0, v0, g64, sc) * b_g + C_ADAM["p"] * U32 * ref[3]
    bm = a * b_g + C_ADAM["m"] * U32 * ref[4]
    bv = omb2 * (2 * g64.abs() * b_g + b_g * b_g) + C_ADAM["v"] * U32 * ref[5]
    return ref, (bp, bm, bv)


def _fused_check(family, got, ref, bounds, what):
    for name, x, r, b in zip("pmv", got, ref[:3], bounds):
        _check_to(family, x, r, b, f"{what} {name}")


# ---- CPU emulation of the kernels' documented arithmetic -----------------------------------------------------------------------
def _fma_chain(a, b):
    """Vector-ALU kernels: acc = fma(a[:, c], b[c, :], acc), c in index order (exact product, one rounding per step)."""
    a, b = a.double(), b.double()
    acc = torch.zeros(a.shape[0], b.shape[1])
    for c in range(a.shape[1]):
        acc = (acc.double() + a[:, c:c + 1] * b[c:c + 1]).float()
    return acc


def _chain(terms, b, step=16):
    """Matrix cores: one f32 accumulator, updated once per `step`-deep slice of the contraction and per term, in the given order."""
    b = b.double()
    acc = torch.zeros(terms[0].shape[0], b.shape[1])
    for s in range(0, b.shape[0], step):
        for t in terms:
            acc = (acc.double() + t[:, s:s + step].double() @ b[s:s + step]).float()
    return acc


def _pair(g):
    hi = _bf16(g)
    return hi, _bf16(g - hi)


def _three(g):
    t0 = _bf16(g)
    r = g - t0
    t1 = _bf16(r)
    return t0, t1, _bf16(r - t1)


def _reduce_bf16path(slabs, bias=None, relu=False, drop_last=False):
    """linear_reduce_bf16path: group g of four takes slabs g, g + 4, ... into four running sums (sixteen / four / one at a time),
    (s0 + s1) + (s2 + s3), then (0 + 1) + (2 + 3), bias, ReLU."""
    ks = slabs.shape[0] - (1 if drop_last else 0)
    parts = []
    for grp in range(4):
        s = [torch.zeros_like(slabs[0]) for _ in range(4)]
        k = grp
        while k + 60 < ks:
            for j in range(16):
                s[j % 4] = s[j % 4] + slabs[k + 4 * j]
            k += 64
        while k + 12 < ks:
            for j in range(4):
                s[j] = s[j] + slabs[k + 4 * j]
            k += 16
        while k < ks:
            s[0] = s[0] + slabs[k]
            k += 4
        parts.append((s[0] + s[1]) + (s[2] + s[3]))
    t = (parts[0] + parts[1]) + (parts[2] + parts[3])
    if bias is not None:
        t = t + bias
    return t.clamp_min(0) if relu else t


def _split(blocks, cap):
    nwg = min(blocks, cap)
    per = -(-blocks // nwg)
    return -(-blocks // per), per


def _slabs(x, w, span, nwg, perm=None, step=16):
    """Workgroup i multiplies columns [i span, (i + 1) span) in `step`-deep steps into one f32 accumulator -> [nwg, m, n]."""
    m, k = x.shape
    n = w.shape[0]
    xp, wp = torch.zeros(m, nwg * span, dtype=torch.float64), torch.zeros(n, nwg * span, dtype=torch.float64)
    xp[:, :k], wp[:, :k] = x, w
    xs, ws = xp.view(m, nwg, span).permute(1, 0, 2), wp.view(n, nwg, span).permute(1, 2, 0)
    if perm is not None:
        xs, ws = xs[:, :, perm], ws[:, perm, :]
    acc = torch.zeros(nwg, m, n)
    for s in range(0, span, step):
        acc = (acc.double() + xs[:, :, s:s + step] @ ws[:, s:s + step, :]).float()
    return acc


def _emu_fwd_bf16(x, w, bias, relu, kind, drop_last=False):
    k = x.shape[1]
    if kind == "v3":      # 128-column tiles in index order, v3_split
        nwg, per = _split(-(-k // 128), 256)
        slabs = _slabs(x, w, 128 * per, nwg)
    else:                 # 64-deep blocks, step s = columns 8 s .. + 7 and 32 + 8 s .. + 7, bf16_fwd_split
        nwg, per = _split(-(-k // 64), 1024)
        one = torch.tensor([32 * h + 8 * s + j for s in range(4) for h in range(2) for j in range(8)])
        perm = torch.cat([one + 64 * b for b in range(per)])
        slabs = _slabs(x, w, 64 * per, nwg, perm)
    return _reduce_bf16path(slabs, bias, relu, drop_last)


def _emu_fwd_small(x, w):
    """linear_fwd_small_f32: sums s0..s3 over k = 4 i + e, the k % 4 tail into s0, (s0 + s1) + (s2 + s3)."""
    m, k = x.shape
    k4 = k - k % 4
    xs, ws = x[:, :k4].double().view(m, -1, 4), w[:, :k4].double().view(w.shape[0], -1, 4)
    s = torch.zeros(4, m, w.shape[0])
    for i in range(k4 // 4):
        s = (s.double() + xs[:, i].t().unsqueeze(2) * ws[:, i].t().unsqueeze(1)).float()
    s0 = s[0]
    for kk in range(k4, k):
        s0 = (s0.double() + x[:, kk:kk + 1].double() * w[:, kk].double()).float()
    return (s0 + s[1]) + (s[2] + s[3])


def _emu_fwd_lanes(x, w, vec):
    """linear_fwd_tile_f32 (vec 4) / linear_fwd_partial_f32 (vec 1): per chunk of 8192 columns thread t runs an fma chain over
    columns vec t + e + 256 vec r; 64 lanes through the shfl_down tree, the waves ((0 + 1) + 2) + 3, the chunks in order."""
    m, k = x.shape
    n = w.shape[0]
    y = torch.zeros(m, n)
    for k0 in range(0, k, 8192):
        xc, wc = x[:, k0:k0 + 8192].double(), w[:, k0:k0 + 8192].double()
        rows = -(-xc.shape[1] // (256 * vec))
        xp, wp = torch.zeros(m, rows * 256 * vec, dtype=torch.float64), torch.zeros(n, rows * 256 * vec, dtype=torch.float64)
        xp[:, :xc.shape[1]], wp[:, :wc.shape[1]] = xc, wc
        live = min(256, -(-xc.shape[1] // vec))      # threads that hold anything but zeros
        xp, wp = xp.view(m, rows, 256, vec)[:, :, :live], wp.view(n, rows, 256, vec)[:, :, :live]
        acc = torch.zeros(live, m, n)
        for r in range(rows):
            for e in range(vec):
                acc = (acc.double() + xp[:, r, :, e].t().unsqueeze(2) * wp[:, r, :, e].t().unsqueeze(1)).float()
        v = torch.zeros(256, m, n)
        v[:live] = acc
        v = v.view(4, 64, m, n)
        off = 32
        while off:
            v = _tree_step(v, off)
            off //= 2
        y = y + (((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])
    return y


def _tree_step(v, off):
    """v += __shfl_down(v, off): lane i takes lane i + off (only lanes below `off` matter afterwards)."""
    return v[:, :off] + v[:, off:2 * off]


def _emu_fwd_gemm(x, w):
    """pv_linear_fwd_f32's GEMM route: pv_gemm_f32 in ceil(k / 2048) splits (the GEMM file's emulation), linear_reduce_f32 in order."""
    from test_gpu_gemm_numerics import _chunk, _emulate
    k = x.shape[1]
    splits = -(-k // 2048)
    chunk = _chunk(k, splits)
    y = torch.zeros(x.shape[0], w.shape[0])
    for s in range(splits):
        y = y + _emulate(x, w.t(), kbeg=min(s * chunk, k), kend=min((s + 1) * chunk, k))
    return y


SKINNY_ORDER = [8 * u + t + 4 * h for u in range(8) for t in range(4) for h in range(2)]      # two-deep steps inside 64 columns


def _emu_fwd_skinny(x, w, direct):
    """linear_fwd_f32_skinny_lds_kernel (workgroup b of min(tiles, 256): tiles b, b + grid, ...; wave half kh its 64 columns of a
    tile -> slab 2 b + kh) or the direct kernel (64-column groups b, b + grid, ...): exact products, two-deep steps, then
    linear_fwd_f32_skinny_reduce_kernel: eight contiguous runs of slabs in order, the eight sums in order."""
    m, k = x.shape
    n = w.shape[0]
    groups = k // 64
    if direct:
        nwg, per = _split(groups, 512)
        owner = [[b + nwg * i for i in range(per) if b + nwg * i < groups] for b in range(nwg)]
    else:
        grid = min(k // 128, 256)
        owner = [[2 * t + kh for t in range(b, k // 128, grid)] for b in range(grid) for kh in range(2)]
    longest = max(len(o) for o in owner)
    idx = torch.full((len(owner), longest * 64), k, dtype=torch.long)      # k: a column of zeros
    order = torch.tensor(SKINNY_ORDER)
    for i, o in enumerate(owner):
        for j, grp in enumerate(o):
            idx[i, 64 * j:64 * j + 64] = 64 * grp + order
    xp, wp = torch.zeros(m, k + 1, dtype=torch.float64), torch.zeros(n, k + 1, dtype=torch.float64)
    xp[:, :k], wp[:, :k] = x, w
    xs, ws = xp[:, idx].permute(1, 0, 2), wp[:, idx].permute(1, 2, 0)
    acc = torch.zeros(len(owner), m, n)
    for s in range(0, longest * 64, 2):
        acc = (acc.double() + xs[:, :, s:s + 2] @ ws[:, s:s + 2, :]).float()
    per = -(-len(owner) // 8)
    total = None
    for g in range(8):
        t = torch.zeros(m, n)
        for slab in acc[g * per:(g + 1) * per]:
            t = t + slab
        total = t if total is None else total + t
    return total


# ---- the reference-only evaluations of every family ----------------------------------------------------------------------------
class Eval:
    """One reference-only evaluation: `got` (f32, before a bf16 store) approximates `exact` (c64, or for a pair kernel the exact
    product of the split g), which is within the split's error of c64."""

    def __init__(self, what, got, c64, s, exact=None, bf16_out=False, pair=False):
        self.what, self.got, self.c64, self.s, self.bf16_out, self.pair = what, got, c64, s, bf16_out, pair
        self.exact = c64 if exact is None else exact

    def r32(self):
        return _ratio_to(self.got, self.exact, U32 * self.s)

    def rpair(self):
        return _ratio_to(self.exact, self.c64, UPAIR * self.s) if self.pair else 0.0

    def final(self):
        return _bf16(self.got) if self.bf16_out else self.got


def _pair_exact(terms, b):
    return sum(t.double() for t in terms) @ b.double()


def _evals(family, shape, regime):
    m, n, k = shape
    ev = []
    if family in ("fwd_rt", "fwd_v3"):
        P = _problem(m, n, k, regime, True)
        c64, s = P.fwd(True, True)
        ev.append(Eval("float32 torch", (P.x @ P.w.t() + P.bias).clamp_min(0), c64, s))
        ev.append(Eval("emulation", _emu_fwd_bf16(P.x, P.w, P.bias, True, "v3" if family == "fwd_v3" else "rt"), c64, s))
    elif family in ("dx_rt", "dx_v2"):
        P = _problem(m, n, k, regime, True, True)
        g = P.g32(True)
        c64, s = P.dx(True)
        pair = family == "dx_v2"
        ev.append(Eval("float32 torch", g @ P.w, c64, s, bf16_out=True, pair=pair))
        if pair:
            hi, lo = _pair(g)
            ev.append(Eval("emulation", _chain([hi, lo], P.w), c64, s, _pair_exact([hi, lo], P.w), True, True))
        else:
            ev.append(Eval("emulation", _fma_chain(g, P.w), c64, s, bf16_out=True))
        c64, s = P.db(True)
        ev.append(Eval("db float32 torch", g.sum(0), c64, s))
        ev.append(Eval("db emulation", _fma_chain(torch.ones(1, m), g)[0], c64, s))
    elif family in ("wg_f32", "wg_b16_valu", "wg_b16_mfma", "one_pass", "tall"):
        scale = 0.125 if family == "tall" else 1.0
        fused = family in ("one_pass", "tall")
        P = _problem(m, n, k, regime, True, fused, 1e-2 if fused else 1.0)
        g = P.g32(True)
        c64, s = P.dw(True, scale)
        b16 = family.startswith("wg_b16")
        mfma = family == "wg_b16_mfma" and m <= 64
        ev.append(Eval("float32 torch", (g * scale).t() @ P.x, c64, s, bf16_out=b16, pair=mfma))
        if mfma:
            hi, lo = _pair(g.t())
            ev.append(Eval("emulation", _chain([lo, hi], P.x), c64, s, _pair_exact([lo, hi], P.x), True, True))
        elif family == "tall":
            t0, t1, t2 = _three(g.t())
            ev.append(Eval("emulation", _chain([t2, t1, t0], P.x) * scale, c64, s))
        else:
            ev.append(Eval("emulation", _fma_chain(g.t(), P.x), c64, s, bf16_out=b16))
        if fused:
            w16 = _bf16(_adam_state(n, k)[0])
            c64, s = P.dx(True, w=w16)
            hi, lo = _pair(g)
            ev.append(Eval("dx float32 torch", g @ w16, c64, s, bf16_out=True, pair=True))
            ev.append(Eval("dx emulation", _chain([lo, hi], w16), c64, s, _pair_exact([lo, hi], w16), True, True))
    elif family.startswith("f32_fwd"):
        P = _problem(m, n, k, regime, False)
        c64, s = P.fwd(False, False)
        ev.append(Eval("float32 torch", P.x @ P.w.t(), c64, s))
        kind = family.split(":")[1]
        emu = {"small": _emu_fwd_small, "tile": lambda a, b: _emu_fwd_lanes(a, b, 4), "partial": lambda a, b: _emu_fwd_lanes(a, b, 1),
               "partial_misaligned": lambda a, b: _emu_fwd_lanes(a, b, 1), "gemm": _emu_fwd_gemm,
               "skinny": lambda a, b: _emu_fwd_skinny(a, b, False), "skinny_direct": lambda a, b: _emu_fwd_skinny(a, b, True)}[kind]
        ev.append(Eval("emulation", emu(P.x, P.w), c64, s))
    elif family in ("f32_bwd", "f32_wgrad_adam", "skinny_dx"):
        P = _problem(m, n, k, regime, False, False, 1e-2 if family == "f32_wgrad_adam" else 1.0)
        g = P.g32(True)
        if family != "f32_wgrad_adam":
            c64, s = P.dx(True)
            ev.append(Eval("dx float32 torch", g @ P.w, c64, s))
            ev.append(Eval("dx emulation", _chain([g], P.w, step=2) if family == "skinny_dx" else _fma_chain(g, P.w), c64, s))
        if family != "skinny_dx":
            c64, s = P.dw(True)
            ev.append(Eval("dw float32 torch", g.t() @ P.x, c64, s))
            ev.append(Eval("dw emulation", _fma_chain(g.t(), P.x), c64, s))
    return ev


def _contraction(family, shape):
    m, n, k = shape
    if family.startswith("fwd") or family.startswith("f32_fwd"):
        return k
    if family in ("dx_rt", "dx_v2", "skinny_dx"):
        return max(n, m) if family != "skinny_dx" else n      # dx over n, its db over m
    if family in ("f32_bwd", "one_pass", "tall"):
        return max(m, n)                                       # dw over m and dx over n in one case
    return m


FAMILIES = ([("fwd_rt", s) for s in FWD_RT] + [("fwd_v3", s) for s in FWD_V3] + [("dx_rt", s) for s in DX_RT] + [("dx_v2", s) for s in DX_V2]
            + [("wg_f32", s) for s in WG_F32] + [("wg_b16_valu", s) for s in WG_B16] + [("wg_b16_mfma", s) for s in WG_B16]
            + [("one_pass", s) for s in ONE_PASS] + [("tall", s) for s in TALL] + [(f"f32_fwd:{kind}", s) for s, kind in F32_FWD]
            + [("f32_bwd", s) for s in F32_BWD_SMALL] + [("f32_bwd", s) for s, _ in F32_BWD_SEP[:2]] + [("f32_wgrad_adam", s) for s in F32_WGRAD_ADAM]
            + [(f"f32_fwd:{kind}", s) for s in SKINNY for kind in ("skinny", "skinny_direct")] + [("skinny_dx", s) for s in SKINNY])
TABLE_CASES = [(f, s, r) for f, s in FAMILIES for r in _regimes(_contraction(f, s))]


def _tid(case):
    return f"{case[0]}-{_sid(case[1])}-{case[2]}"


# ---- CPU: the checker accepts the reference-only evaluations -------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE_CASES, ids=_tid)
def test_checker_accepts_float32_torch_and_the_emulation(case):
    family, shape, regime = case
    for e in _evals(family, shape, regime):
        _check("cpu", e.final(), e.c64, e.s, regime, f"{_tid(case)} {e.what}", e.bf16_out, e.pair)


FUSED = [("one_pass", s) for s in ONE_PASS] + [("tall", s) for s in TALL] + [("f32_wgrad_adam", s) for s in F32_WGRAD_ADAM]


@pytest.mark.parametrize("case", [(f, s, r) for f, s in FUSED for r in _regimes(s[0])], ids=_tid)
def test_checker_accepts_float32_adam_on_both_gradients(case):
    """adam.h's lines in float32 on the float32 torch gradient and on the emulated gradient stay within the fused bounds."""
    family, (m, n, k), regime = case
    sc = _scalars(3)
    p0, m0, v0 = _adam_state(n, k)
    for e in _evals(family, (m, n, k), regime)[:2]:
        ref, bounds = _fused_bounds(p0, m0, v0, e.c64, C[regime] * U32 * e.s, sc)
        _fused_check("cpu", _adam32(p0, m0, v0, e.got, sc), ref, bounds, f"{_tid(case)} {e.what}")


def _adam_inputs(size, seed=0):
    g = torch.Generator().manual_seed(size + seed)
    p, m, v = torch.randn(size, generator=g) * 0.05, torch.randn(size, generator=g) * 1e-3, torch.rand(size, generator=g) * 1e-6 + 1e-8
    grad = torch.randn(size, generator=g) * 1e-2
    for i, val in zip((size // 2, size // 3, size - 1, 0), (1e4, 1e-12, -0.0, 0.0)):
        grad[i] = val
    return p, m, v, grad


@pytest.mark.parametrize("step,scale", ADAM_CASES)
def test_adam_checker_accepts_float32_and_rejects_a_wrong_order_and_eps_inside_the_root(step, scale):
    sc = _scalars(step)
    for size in ADAM_SIZES:
        p, m, v, grad = _adam_inputs(size)
        g = grad * scale
        ref = _adam64(p, m, v, g, sc)
        _adam_check("cpu", _adam32(p, m, v, g, sc), ref, f"float32 Adam, {size} elements, step {step}")
        if size > 3:
            for mutation in ("old_m", "eps_inside"):
                with pytest.raises(AssertionError, match="x the bound"):
                    _adam_check("cpu", _adam32(p, m, v, g, sc, mutation), ref, mutation)


# ---- CPU: the checker rejects what it must -------------------------------------------------------------------------------------
def _one_tile(good, bad, rows=slice(None), cols=slice(None)):
    out = good.clone()
    out[rows, cols] = bad[rows, cols]
    return out


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", REJECT, ids=_sid)
def test_checker_rejects_subtly_wrong_results(shape, regime):
    m, n, k = shape
    P = _problem(m, n, k, regime, True, True)
    last = (slice(m - 1, m), slice(n - 1, n))
    # forward: bias, last term, a missing slab
    F = _problem(m, n, k, regime, True)
    c64, s = F.fwd(True, False)
    good = _emu_fwd_bf16(F.x, F.w, F.bias, False, "rt")
    _check("cpu", good, c64, s, regime, "forward")
    _rejected(_one_tile(good, good + F.bias, *last), c64, s, regime, "bias added twice in one element")
    _rejected(_one_tile(good, good - F.bias, *last), c64, s, regime, "bias not added in one element")
    _rejected(_one_tile(good, _emu_fwd_bf16(F.x[:, :-1], F.w[:, :-1], F.bias, False, "rt"), *last), c64, s, regime, "last k term dropped")
    if k > 64:
        _rejected(_emu_fwd_bf16(F.x, F.w, F.bias, False, "rt", drop_last=True), c64, s, regime, "a split-K slab missing")
    # dx, f32 g (bf16 out) and pair (bf16 out)
    g, hi_lo = P.g32(True), _pair(P.g32(True))
    c64, s = P.dx(True)
    for pair, good in ((False, _bf16(_fma_chain(g, P.w))), (True, _bf16(_chain(list(hi_lo), P.w)))):
        kw = dict(bf16_out=True, pair=pair)
        _check("cpu", good, c64, s, regime, "dx", **kw)
        wrong_gate = torch.where(P.y >= 0, P.dy, torch.zeros(()))
        _rejected(_one_tile(good, _bf16(_fma_chain(wrong_gate, P.w)), slice(m - 1, m)), c64, s, regime, "gate taken as y >= 0 in the last row", **kw)
        off = torch.where(P.y.roll(1, 1) > 0, P.dy, torch.zeros(()))
        _rejected(_one_tile(good, _bf16(_fma_chain(off, P.w)), slice(m - 1, m)), c64, s, regime, "gate read one column off in the last row", **kw)
        r = int((g[:, n - 1] != 0).nonzero()[-1])      # the last row whose last gate is open
        _rejected(_one_tile(good, _bf16(_fma_chain(g[:, :-1], P.w[:-1])), slice(r, r + 1), slice(k - 8, k)), c64, s, regime,
                  "last n term dropped in the last chunk of a row", **kw)
        _rejected(_one_tile(good, torch.zeros_like(good), slice(m - 1, m), slice(k - 8, k)), c64, s, regime, "last 8-column chunk left at zero", **kw)
        _rejected(_one_tile(good, _bf16(_fma_chain(g.roll(1, 0), P.w)), slice(m - 1, m)), c64, s, regime, "last row from the previous row's g", **kw)
    # weight gradient: f32 out; the tall kernel's third term, seen in m
    c64, s = P.dw(True)
    good = _fma_chain(g.t(), P.x)
    _check("cpu", good, c64, s, regime, "dw")
    j = int((g[m - 1] != 0).nonzero()[-1])      # the last output whose gate is open in the last batch row
    _rejected(_one_tile(good, _fma_chain(g[:-1].t(), P.x[:-1]), slice(j, j + 1)), c64, s, regime, "last batch row dropped in one output")
    t0, t1, t2 = _three(g.t())
    sc = _scalars(3)
    p0, m0, v0 = _adam_state(n, k)
    ref, bounds = _fused_bounds(p0, m0, v0, c64, C[regime] * U32 * s, sc)
    _fused_check("cpu", _adam32(p0, m0, v0, _chain([t2, t1, t0], P.x), sc), ref, bounds, "tall, three terms")
    with pytest.raises(AssertionError, match="x the bound"):
        _check_to("cpu", _adam32(p0, m0, v0, _chain([t1, t0], P.x), sc)[1], ref[1], bounds[1], "tall, third term dropped: m")


def test_dropped_lo_term_is_below_the_bf16_rounding_of_most_elements():
    """What the checker cannot see.  (32, 128, 256), dx behind a bf16 store with g's lo term dropped.  The error is about 2^-9 of
    each product: measured 2^-12.1 S (median; 2^-9.7 S at most) for `zero_mean` and 2^-12.3 S for `positive`, against a bf16 rounding
    term 2^-8 |c64| of 2^-10.9 S (median) for `zero_mean` and 2^-8.0 S for `positive`, where nothing cancels.  So with `positive`
    operands the fault is invisible (0.2 % of the elements exceed the bound, the worst by 1.09); with `zero_mean` operands it is
    seen only where the sum cancels -- 26 % of the elements, the worst 30 x the bound: a whole tensor with the fault is rejected,
    the same fault confined to one element passes three times out of four."""
    m, n, k = 32, 128, 256
    for regime, least, most in (("positive", 0.0, 0.01), ("zero_mean", 0.1, 0.5)):
        P = _problem(m, n, k, regime, True, True)
        g = P.g32(True)
        c64, s = P.dx(True)
        hi, _ = _pair(g)
        bad = _bf16(_chain([hi], P.w))
        ratio = (bad.double() - c64).abs() / (_bound(c64, s, C[regime], True, True) + 1e-30)
        seen = float((ratio > 1).double().mean())
        print(f"lo term dropped, {regime}: worst error / bound {float(ratio.max()):.2f}, fraction of elements seen {seen:.4f}")
        assert least <= seen <= most, "the docstring's statement about the blind spot no longer holds"
        assert float(ratio.median()) < 1.0


# ---- GPU helpers ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


class Guarded:
    """`numel` elements inside a sentinel-filled buffer."""

    def __init__(self, shape, dtype, device, init=None):
        numel = math.prod(shape)
        self.sent = torch.tensor([SENTINEL]).to(dtype)
        self.buf = self.sent.to(device).repeat(numel + 2 * GUARD)
        self.t = self.buf[GUARD:GUARD + numel].view(*shape)
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        b, want = _bits(self.buf.cpu()), _bits(self.sent)
        return bool((b[:GUARD] == want).all() and (b[-GUARD:] == want).all())


def _shadow_is_rounded_p(shadow, p):
    return torch.equal(_bits(shadow), _bits(p.to(torch.bfloat16)))


def _masks(P, device):
    return [(False, None), (True, P.y.to(device))]


# ---- GPU 1, 2: bf16 forward ----------------------------------------------------------------------------------------------------
def _forward_case(family, shape, device):
    K = _ops()
    m, n, k = shape
    for regime in _regimes(k):
        P = _problem(m, n, k, regime, True)
        xd, wd, bd = P.dev(P.x, device), P.dev(P.w, device), P.bias.to(device)
        for bias, relu in ((False, False), (True, False), (True, True)):
            c64, s = P.fwd(bias, relu)
            got = K.linear_fwd_bf16(xd, wd, bd if bias else None, relu=relu)
            _check(family, got, c64, s, regime, f"{_sid(shape)} {regime} bias {bias} relu {relu}")
            if relu and regime == "zero_mean" and m * n > 64:
                assert 0.05 < float((c64 == 0).double().mean()) < 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FWD_RT, ids=_sid)
def test_bf16_forward_register_tiled(shape, device):
    """linear_fwd_bf16_kernel<MT> + linear_reduce_bf16path."""
    assert not (32 <= shape[1] <= 128 and shape[1] % 16 == 0)
    _forward_case("bf16 fwd register-tiled", shape, device)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FWD_V3, ids=_sid)
def test_bf16_forward_v3(shape, device):
    """linear_fwd_bf16_v3_kernel<MB> + linear_reduce_bf16path over all row blocks."""
    assert 32 <= shape[1] <= 128 and shape[1] % 16 == 0
    _forward_case("bf16 fwd v3", shape, device)


# ---- GPU 3: bf16 dx and db -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", DX_RT + DX_V2, ids=_sid)
def test_bf16_dx_and_db(shape, device):
    """linear_bwd_dx_bf16_kernel / linear_bwd_dx_bf16_v2_kernel (+ gate_bf16_by_relu_kernel); db from the v2 kernel (m <= 32 on
    its shapes) or linear_bwd_db_bf16path."""
    K = _ops()
    m, n, k = shape
    v2 = 32 <= n <= 128 and n % 16 == 0
    assert v2 == (shape in DX_V2)
    family = "bf16 dx v2" if v2 else "bf16 dx register-tiled"
    for regime in _regimes(max(m, n)):
        P = _problem(m, n, k, regime, True, True)
        xd, wd, dyd = P.dev(P.x, device), P.dev(P.w, device), P.dy.to(device)
        for masked, yd in _masks(P, device):
            for gate in (False, True):
                dx, _, db = K.linear_bwd_bf16(xd, wd, dyd, yd, need_dx=True, need_dw=False, gate_dx_by_x=gate)
                c64, s = P.dx(masked, gate)
                _check(family, dx, c64, s, regime, f"{_sid(shape)} {regime} mask {masked} gate {gate}", bf16_out=True, pair=v2)
                if gate:
                    assert bool((dx.cpu()[~(P.x > 0)] == 0).all()), "dx is not an exact zero where x gates it"
                c64, s = P.db(masked)
                _check("bf16 db " + ("v2" if v2 and m <= 32 else "db_bf16path"), db, c64, s, regime, f"{_sid(shape)} {regime} mask {masked}")


# ---- GPU 4: bf16 weight gradient -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", WG_F32, ids=_sid)
def test_bf16_weight_gradient_f32_out(shape, device):
    """linear_bwd_dw_bf16_kernel<0>."""
    K = _ops()
    m, n, k = shape
    for regime in _regimes(m):
        P = _problem(m, n, k, regime, True)
        for masked, yd in _masks(P, device):
            _, dw, _ = K.linear_bwd_bf16(P.dev(P.x, device), P.dev(P.w, device), P.dy.to(device), yd, need_dx=False, need_db=False)
            c64, s = P.dw(masked)
            _check("bf16 dw f32 out", dw, c64, s, regime, f"{_sid(shape)} {regime} mask {masked}")


@pytest.mark.gpu
@pytest.mark.parametrize("valu", [True, False], ids=["valu", "mfma"])
@pytest.mark.parametrize("shape", WG_B16, ids=_sid)
def test_bf16_weight_gradient_bf16_out(shape, valu, device, monkeypatch):
    """linear_bwd_dw_bf16_kernel<2> (PV_WGRAD_BF16OUT_VALU=1, or m > 64) and linear_wgrad_bf16out_mfma_kernel."""
    K = _ops()
    m, n, k = shape
    if valu:
        monkeypatch.setenv("PV_WGRAD_BF16OUT_VALU", "1")
    mfma = not valu and m <= 64
    for regime in _regimes(m):
        P = _problem(m, n, k, regime, True)
        for masked, yd in _masks(P, device):
            dw = K.linear_wgrad_bf16out(P.dev(P.x, device), P.dy.to(device), yd, n)
            c64, s = P.dw(masked)
            _check("bf16 dw bf16 out " + ("mfma" if mfma else "valu"), dw, c64, s, regime, f"{_sid(shape)} {regime} mask {masked}",
                   bf16_out=True, pair=mfma)


# ---- GPU 5: the one-pass backward ----------------------------------------------------------------------------------------------
def _state(n, k, device):
    p0, m0, v0 = _adam_state(n, k)
    return [t.clone().to(device) for t in (p0, m0, v0)] + [p0.to(torch.bfloat16).to(device)]


def _same(a, b, what):
    for name, x, y in zip(("p", "m", "v", "shadow", "dx", "db"), a, b):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ONE_PASS, ids=_sid)
def test_one_pass_backward(shape, device, monkeypatch):
    """linear_bwd_dw_dx_adam_kernel with host and device scalars: dx, db, p, m, v, shadow against float64; bitwise: the fused
    kernel, the two-pass form, device scalars, tiled moments, the PV_FC1_FETCH schedules."""
    K = _ops()
    m, n, k = shape
    step, sc = 3, _scalars(3)
    p0, m0, v0 = _adam_state(n, k)
    w16 = _bf16(p0)
    for regime in _regimes(max(m, n)):
        P = _problem(m, n, k, regime, True, True, 1e-2)
        xd, dyd = P.dev(P.x, device), P.dy.to(device)
        for masked, yd in _masks(P, device):
            g64, sg = P.dw(masked)
            ref, bounds = _fused_bounds(p0, m0, v0, g64, C[regime] * U32 * sg, sc)
            what = f"{_sid(shape)} {regime} mask {masked}"
            results = {}
            for gate in (False, True):
                st = _state(n, k, device)
                dx, db = K.linear_wgrad_dx_adam_bf16(xd, dyd, yd, *st, step, need_db=True, gate_dx_by_x=gate)
                results[gate] = st + [dx, db]
                c64, s = P.dx(masked, gate, w=w16)
                _check("one-pass dx", dx, c64, s, regime, f"{what} gate {gate}", bf16_out=True, pair=True)
                if gate:
                    assert bool((dx.cpu()[~(P.x > 0)] == 0).all()), "dx is not an exact zero where x gates it"
            st, dx, db = results[True][:4], results[True][4], results[True][5]
            c64, s = P.db(masked)
            _check("one-pass db", db, c64, s, regime, what)
            _fused_check("one-pass Adam", st[:3], ref, bounds, what)
            assert _shadow_is_rounded_p(st[3], st[0])
            _same(results[False][:4], st, "gate_dx_by_x changed the update")
            # bitwise relations
            fu = _state(n, k, device)
            K.linear_wgrad_adam_bf16(xd, dyd, yd, *fu, step)
            _same(fu, st, "one-pass != fused")
            _fused_check("fused wgrad + Adam", fu[:3], ref, bounds, what)
            tp = _state(n, k, device)
            _, dw, _ = K.linear_bwd_bf16(xd, fu[3], dyd, yd, need_dx=False, need_db=False)
            K.adam_step(tp[0], dw, tp[1], tp[2], step, bf16_shadow=tp[3])
            _same(tp, st, "fused != two-pass")
            scal, step_t = torch.zeros(6, device=device), torch.tensor([step - 1], dtype=torch.int32, device=device)
            K.adam_scalars_advance(scal, step_t)
            dv = _state(n, k, device)
            dxv, dbv = K.linear_wgrad_dx_adam_dev_bf16(xd, dyd, yd, *dv, scal, need_db=True, gate_dx_by_x=True)
            _same(dv + [dxv, dbv], st + [dx, db], "dev scalars != host scalars")
            if k % 128 == 0:
                tl = _state(n, k, device)
                tl[1], tl[2] = K.moments_to_tiled(tl[1]), K.moments_to_tiled(tl[2])
                dxt, dbt = K.linear_wgrad_dx_adam_bf16(xd, dyd, yd, *tl, step, need_db=True, gate_dx_by_x=True, moments_tiled=True)
                tl[1], tl[2] = K.moments_to_rows(tl[1]), K.moments_to_rows(tl[2])
                _same(tl + [dxt, dbt], st + [dx, db], "tiled moments != row-major")
            for variant in ("late", "early1", "early2"):
                monkeypatch.setenv("PV_FC1_FETCH", variant)
                va = _state(n, k, device)
                dxa, dba = K.linear_wgrad_dx_adam_bf16(xd, dyd, yd, *va, step, need_db=True, gate_dx_by_x=True)
                monkeypatch.delenv("PV_FC1_FETCH")
                _same(va + [dxa, dba], st + [dx, db], f"PV_FC1_FETCH={variant} != default")


# ---- GPU 6: the K-sharded (tall) backward --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", TALL, ids=_sid)
def test_tall_backward(shape, device):
    """tall_split_g_kernel + linear_bwd_dw_dx_adam_tall_kernel: grad_scale 0.125, with and without gate_dx_by_x, tiled moments."""
    K = _ops()
    m, n, k = shape
    step, sc, scale = 3, _scalars(3), 0.125
    p0, m0, v0 = _adam_state(n, k)
    w16 = _bf16(p0)
    for regime in _regimes(max(m, n)):
        P = _problem(m, n, k, regime, True, True, 1e-2)
        xd, gd = P.dev(P.x, device), P.g32(True).to(device)
        g64, sg = P.dw(True, scale)
        ref, bounds = _fused_bounds(p0, m0, v0, g64, C[regime] * U32 * sg, sc)
        what = f"{_sid(shape)} {regime}"
        results = {}
        for gate in (False, True):
            st = _state(n, k, device)
            dx = K.linear_wgrad_dx_adam_tall_bf16(xd, gd, *st, step, grad_scale=scale, gate_dx_by_x=gate)
            results[gate] = st + [dx]
            c64, s = P.dx(True, gate, w=w16)
            _check("tall dx", dx, c64, s, regime, f"{what} gate {gate}", bf16_out=True, pair=True)
            if gate:
                assert bool((dx.cpu()[~(P.x > 0)] == 0).all()), "dx is not an exact zero where x gates it"
            _fused_check("tall Adam", st[:3], ref, bounds, f"{what} gate {gate}")
            assert _shadow_is_rounded_p(st[3], st[0])
        _same(results[False][:4], results[True][:4], "gate_dx_by_x changed the update")
        if k % 128 == 0:
            tl = _state(n, k, device)
            tl[1], tl[2] = K.moments_to_tiled(tl[1]), K.moments_to_tiled(tl[2])
            dxt = K.linear_wgrad_dx_adam_tall_bf16(xd, gd, *tl, step, grad_scale=scale, gate_dx_by_x=True, moments_tiled=True)
            tl[1], tl[2] = K.moments_to_rows(tl[1]), K.moments_to_rows(tl[2])
            _same(tl + [dxt], results[True], "tiled moments != row-major")


# ---- GPU 7: the f32 dense head -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", F32_FWD, ids=[f"{_sid(s)}-{kind}" for s, kind in F32_FWD])
def test_f32_forward(shape, kind, device):
    """linear_fwd_small_f32 / linear_fwd_tile_f32 / linear_fwd_partial_f32 + linear_reduce_f32 / the GEMM route."""
    K = _ops()
    m, n, k = shape
    for regime in _regimes(k):
        P = _problem(m, n, k, regime, False)
        xd, wd, bd = P.x.to(device), P.w.to(device), P.bias.to(device)
        if kind == "partial_misaligned":      # x one element into its buffer
            buf = torch.full((m * k + 8,), float("nan"), device=device)
            xd = buf[1:1 + m * k].view(m, k)
            xd.copy_(P.x.to(device))
            assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
        for bias, relu in ((False, False), (True, True)):
            c64, s = P.fwd(bias, relu)
            got = K.linear_fwd_f32(xd, wd, bd if bias else None, relu=relu)
            _check(f"f32 fwd {kind.split('_')[0]}", got, c64, s, regime, f"{_sid(shape)} {regime} bias {bias} relu {relu}")


def _f32_backward(family, shape, need_dx, device):
    K = _ops()
    m, n, k = shape
    for regime in _regimes(max(m, n)):
        P = _problem(m, n, k, regime, False)
        for masked, yd in _masks(P, device):
            dx, dw, db = K.linear_bwd_f32(P.x.to(device), P.w.to(device), P.dy.to(device), yd, need_dx=need_dx)
            what = f"{_sid(shape)} {regime} mask {masked}"
            if need_dx:
                _check(family + " dx", dx, *P.dx(masked), regime, what)
            else:
                assert dx is None
            _check(family + " dw", dw, *P.dw(masked), regime, what)
            _check(family + " db", db, *P.db(masked), regime, what)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", F32_BWD_SMALL, ids=_sid)
def test_f32_backward_in_one_launch(shape, device):
    """linear_bwd_small_f32: linear_bwd_dx_body, linear_bwd_dw_body and linear_bwd_db_body selected by block index."""
    assert shape[2] <= 4096 and shape[0] * shape[1] <= 65536
    _f32_backward("f32 bwd small", shape, True, device)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,need_dx", F32_BWD_SEP, ids=[f"{_sid(s)}-dx{int(d)}" for s, d in F32_BWD_SEP])
def test_f32_backward_separate_kernels(shape, need_dx, device):
    """linear_bwd_dx_f32, linear_bwd_dw_f32, linear_bwd_db_f32: k > 4096, or a head-sized first layer (need_dx=False)."""
    assert shape[2] > 4096 or not need_dx
    _f32_backward("f32 bwd separate", shape, need_dx, device)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", F32_WGRAD_ADAM, ids=_sid)
def test_f32_wgrad_adam(shape, device):
    """linear_bwd_dw_bf16_kernel<1, float>: exact f32 products, Adam in the same pass; bitwise the separate kernels + adam_step
    where the separate weight gradient adds in the same order (it does: both are fma chains over the rows)."""
    K = _ops()
    m, n, k = shape
    step, sc = 3, _scalars(3)
    p0, m0, v0 = _adam_state(n, k)
    for regime in _regimes(m):
        P = _problem(m, n, k, regime, False, False, 1e-2)
        for masked, yd in _masks(P, device):
            g64, sg = P.dw(masked)
            ref, bounds = _fused_bounds(p0, m0, v0, g64, C[regime] * U32 * sg, sc)
            st = _state(n, k, device)[:3]
            K.linear_wgrad_adam_f32(P.x.to(device), P.dy.to(device), yd, *st, step)
            _fused_check("f32 wgrad + Adam", st, ref, bounds, f"{_sid(shape)} {regime} mask {masked}")


# ---- GPU 8: the f32 skinny kernels ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SKINNY, ids=_sid)
def test_f32_skinny(shape, device, monkeypatch):
    """linear_fwd_f32_skinny_lds_kernel, linear_fwd_f32_skinny_kernel (PV_LINEAR_F32_SKINNY_DIRECT=1), both through
    linear_fwd_f32_skinny_reduce_kernel, and linear_dx_f32_skinny_kernel."""
    K = _ops()
    m, n, k = shape
    assert K.linear_f32_skinny_covers(m, n, k)
    P = _problem(m, n, k, "zero_mean", False)
    xd, wd, bd = P.x.to(device), P.w.to(device), P.bias.to(device)
    for bias, relu in ((False, False), (True, True)):
        c64, s = P.fwd(bias, relu)
        _check("f32 skinny fwd lds", K.linear_fwd_f32_skinny(xd, wd, bd if bias else None, relu=relu), c64, s, "zero_mean", f"{_sid(shape)} bias {bias}")
        monkeypatch.setenv("PV_LINEAR_F32_SKINNY_DIRECT", "1")
        got = K.linear_fwd_f32_skinny(xd, wd, bd if bias else None, relu=relu)
        monkeypatch.delenv("PV_LINEAR_F32_SKINNY_DIRECT")
        _check("f32 skinny fwd direct", got, c64, s, "zero_mean", f"{_sid(shape)} bias {bias}")
    for regime in _regimes(n):
        Q = _problem(m, n, k, regime, False)
        g = Q.g32(True)
        _check("f32 skinny dx", K.linear_dx_f32_skinny(g.to(device), Q.w.to(device)), *Q.dx(True), regime, f"{_sid(shape)} {regime}")


# ---- GPU 9: Adam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("step,scale", ADAM_CASES)
def test_adam_forms(step, scale, device):
    """adam_step, adam_step_multi, adam_step_multi_dev, adam_step_bf16grad at every size, with and without shadow."""
    K = _ops()
    sc = _scalars(step)
    cases = [_adam_inputs(size) for size in ADAM_SIZES]
    refs = [_adam64(p, m, v, g * scale, sc) for p, m, v, g in cases]
    scal, step_t = torch.zeros(6, device=device), torch.tensor([step - 1], dtype=torch.int32, device=device)
    K.adam_scalars_advance(scal, step_t)
    assert int(step_t) == step
    for shadow in (False, True):
        def fresh(grad16=False):
            out = []
            for p, m, v, g in cases:
                gd = g.to(torch.bfloat16).to(device) if grad16 else g.to(device)
                out.append((p.to(device), gd, m.to(device), v.to(device), torch.zeros(p.numel(), dtype=torch.bfloat16, device=device) if shadow else None))
            return out

        def verify(form, items, want):
            for (p, _, m, v, sh), ref, size in zip(items, want, ADAM_SIZES):
                _adam_check(f"Adam {form}", (p, m, v), ref, f"{size} elements, step {step}, scale {scale}, shadow {shadow}")
                if shadow:
                    assert _shadow_is_rounded_p(sh, p), f"{form}: shadow is not p rounded"

        single = fresh()
        for p, g, m, v, sh in single:
            K.adam_step(p, g, m, v, step, bf16_shadow=sh, grad_scale=scale)
        verify("single", single, refs)
        multi = fresh()
        K.adam_step_multi(multi, step, grad_scale=scale)
        verify("multi", multi, refs)
        dev = fresh()
        K.adam_step_multi_dev(dev, scal, grad_scale=scale)
        verify("multi-dev", dev, refs)
        for a, b in zip(single, multi):
            for i in (0, 2, 3):
                assert torch.equal(_bits(a[i]), _bits(b[i])), "multi != single"
        g16 = fresh(grad16=True)
        refs16 = [_adam64(p, m, v, _bf16(g) * scale, sc) for p, m, v, g in cases]
        for p, g, m, v, sh in g16:
            K.adam_step_bf16grad(p, g, m, v, step, bf16_shadow=sh, grad_scale=scale)
        verify("bf16 gradient", g16, refs16)


# ---- GPU 10: sentinels around every output, through the C ABI ------------------------------------------------------------------
@pytest.mark.gpu
def test_outputs_leave_their_surroundings_alone(device, monkeypatch):
    """One ragged shape per entry point: y, dx, dw, bf16 dw, db, p / m / v / shadow inside buffers filled with 1.2345678e30."""
    K = _ops()
    lib, ptr, stream = K.get_lib(), K.ptr, K.current_stream_ptr
    f32, b16 = torch.float32, torch.bfloat16

    keep = []

    def held(t):      # an operand made for one call: alive until the test ends, not until its pointer has been taken
        keep.append(t)
        return ptr(t)

    def guards(*gs):
        torch.cuda.synchronize()
        assert all(g.intact() for g in gs), "written outside the result"

    # bf16 forward: register-tiled and v3
    for (m, n, k), family in (((33, 5, 72), "bf16 fwd register-tiled"), ((33, 48, 136), "bf16 fwd v3")):
        P = _problem(m, n, k, "zero_mean", True)
        need = ctypes.c_size_t(0)
        K.check(lib.pv_linear_bf16_workspace_bytes(m, n, k, ctypes.byref(need)), "workspace")
        ws = torch.empty(need.value, dtype=torch.uint8, device=device)
        y = Guarded((m, n), f32, device)
        K.check(lib.pv_linear_fwd_bf16(held(P.dev(P.x, device)), held(P.dev(P.w, device)), held(P.bias.to(device)), ptr(y.t), m, n, k, 1, ptr(ws),
                                       ws.numel(), stream()), "pv_linear_fwd_bf16")
        guards(y)
        _check(family, y.t, *P.fwd(True, True), "zero_mean", f"{m}x{n}x{k} guarded")
    # bf16 backward: register-tiled dx and v2 dx, dw, db
    for (m, n, k), v2 in (((17, 5, 72), False), ((31, 48, 264), True)):
        P = _problem(m, n, k, "zero_mean", True, True)
        dx, dw, db = Guarded((m, k), b16, device), Guarded((n, k), f32, device), Guarded((n,), f32, device)
        K.check(lib.pv_linear_bwd_bf16(held(P.dev(P.x, device)), held(P.dev(P.w, device)), held(P.dy.to(device)), held(P.y.to(device)), ptr(dx.t),
                                       ptr(dw.t), ptr(db.t), m, n, k, 1, stream()), "pv_linear_bwd_bf16")
        guards(dx, dw, db)
        _check("bf16 dx v2" if v2 else "bf16 dx register-tiled", dx.t, *P.dx(True, True), "zero_mean", f"{m}x{n}x{k} guarded", bf16_out=True, pair=v2)
        _check("bf16 dw f32 out", dw.t, *P.dw(True), "zero_mean", f"{m}x{n}x{k} guarded")
        _check("bf16 db", db.t, *P.db(True), "zero_mean", f"{m}x{n}x{k} guarded")
        for valu in (True, False):
            if valu:
                monkeypatch.setenv("PV_WGRAD_BF16OUT_VALU", "1")
            dw16 = Guarded((n, k), b16, device)
            K.check(lib.pv_linear_wgrad_bf16out(held(P.dev(P.x, device)), held(P.dy.to(device)), held(P.y.to(device)), ptr(dw16.t), m, n, k, stream()),
                    "pv_linear_wgrad_bf16out")
            guards(dw16)
            monkeypatch.delenv("PV_WGRAD_BF16OUT_VALU", raising=False)
            _check("bf16 dw bf16 out " + ("valu" if valu else "mfma"), dw16.t, *P.dw(True), "zero_mean", f"{m}x{n}x{k} guarded", bf16_out=True, pair=not valu)
    # one-pass and tall: p, m, v, shadow, dx, db
    m, n, k = 31, 120, 392
    P = _problem(m, n, k, "zero_mean", True, True, 1e-2)
    p0, m0, v0 = _adam_state(n, k)
    sc = _scalars(3)
    scal, step_t = torch.zeros(6, device=device), torch.tensor([2], dtype=torch.int32, device=device)
    K.adam_scalars_advance(scal, step_t)
    for form in ("host", "dev", "tall"):
        tall = form == "tall"
        st = [Guarded((n, k), f32, device, t) for t in (p0, m0, v0)] + [Guarded((n, k), b16, device, p0.to(b16))]
        dx, db = Guarded((m, k), b16, device), Guarded((n,), f32, device)
        args = [ptr(g.t) for g in st]
        if tall:
            need = ctypes.c_size_t(0)
            K.check(lib.pv_linear_wgrad_dx_adam_tall_bf16_workspace_bytes(m, ctypes.byref(need)), "workspace")
            ws = torch.empty(need.value, dtype=torch.uint8, device=device)
            K.check(lib.pv_linear_wgrad_dx_adam_tall_bf16(held(P.dev(P.x, device)), held(P.g32(True).to(device)), *args, ptr(dx.t), m, n, k, LR, *BETAS,
                                                          EPS, 3, 1.0, 1, 0, ptr(ws), need.value, stream()), "pv_linear_wgrad_dx_adam_tall_bf16")
            guards(dx, *st)
        elif form == "dev":
            K.check(lib.pv_linear_wgrad_dx_adam_dev_bf16(held(P.dev(P.x, device)), held(P.dy.to(device)), held(P.y.to(device)), *args, ptr(dx.t), ptr(db.t),
                                                         m, n, k, ptr(scal), 1, 0, stream()), "pv_linear_wgrad_dx_adam_dev_bf16")
            guards(dx, db, *st)
        else:
            K.check(lib.pv_linear_wgrad_dx_adam_bf16(held(P.dev(P.x, device)), held(P.dy.to(device)), held(P.y.to(device)), *args, ptr(dx.t), ptr(db.t),
                                                     m, n, k, LR, *BETAS, EPS, 3, 1, 0, stream()), "pv_linear_wgrad_dx_adam_bf16")
            guards(dx, db, *st)
        g64, sg = P.dw(True)
        ref, bounds = _fused_bounds(p0, m0, v0, g64, C["zero_mean"] * U32 * sg, sc)
        _fused_check("tall Adam" if tall else "one-pass Adam", [g.t for g in st[:3]], ref, bounds, f"{m}x{n}x{k} guarded")
        assert _shadow_is_rounded_p(st[3].t, st[0].t)
        _check("tall dx" if tall else "one-pass dx", dx.t, *P.dx(True, True, w=_bf16(p0)), "zero_mean", f"{m}x{n}x{k} guarded", bf16_out=True, pair=True)
    # fused weight gradient + Adam, bf16 and f32 activations
    for bf16 in (True, False):
        P = _problem(7, 17, 136, "zero_mean", bf16, False, 1e-2)
        p0, m0, v0 = _adam_state(17, 136)
        st = [Guarded((17, 136), f32, device, t) for t in (p0, m0, v0)]
        if bf16:
            sh = Guarded((17, 136), b16, device, p0.to(b16))
            K.check(lib.pv_linear_wgrad_adam_bf16(held(P.dev(P.x, device)), held(P.dy.to(device)), held(P.y.to(device)), *[ptr(g.t) for g in st], ptr(sh.t),
                                                  7, 17, 136, LR, *BETAS, EPS, 3, stream()), "pv_linear_wgrad_adam_bf16")
            guards(sh, *st)
        else:
            K.check(lib.pv_linear_wgrad_adam_f32(held(P.x.to(device)), held(P.dy.to(device)), held(P.y.to(device)), *[ptr(g.t) for g in st],
                                                 7, 17, 136, LR, *BETAS, EPS, 3, stream()), "pv_linear_wgrad_adam_f32")
            guards(*st)
        g64, sg = P.dw(True)
        ref, bounds = _fused_bounds(p0, m0, v0, g64, C["zero_mean"] * U32 * sg, sc)
        _fused_check("fused wgrad + Adam" if bf16 else "f32 wgrad + Adam", [g.t for g in st], ref, bounds, "7x17x136 guarded")
    # f32 forward (small, tile, partial) and backward (one launch, separate)
    for m, n, k in ((41, 41, 133), (9, 9, 4100), (9, 3, 4097)):
        P = _problem(m, n, k, "zero_mean", False)
        need = ctypes.c_size_t(0)
        K.check(lib.pv_linear_workspace_bytes(m, n, k, ctypes.byref(need)), "workspace")
        ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=device)
        y = Guarded((m, n), f32, device)
        K.check(lib.pv_linear_fwd_f32(held(P.x.to(device)), held(P.w.to(device)), held(P.bias.to(device)), ptr(y.t), m, n, k, 0, ptr(ws), ws.numel(), stream()),
                "pv_linear_fwd_f32")
        guards(y)
        _check("f32 fwd guarded", y.t, *P.fwd(True, False), "zero_mean", f"{m}x{n}x{k}")
        dx, dw, db = Guarded((m, k), f32, device), Guarded((n, k), f32, device), Guarded((n,), f32, device)
        K.check(lib.pv_linear_bwd_f32(held(P.x.to(device)), held(P.w.to(device)), held(P.dy.to(device)), held(P.y.to(device)), ptr(dx.t), ptr(dw.t), ptr(db.t),
                                      m, n, k, stream()), "pv_linear_bwd_f32")
        guards(dx, dw, db)
        _check("f32 bwd guarded dx", dx.t, *P.dx(True), "zero_mean", f"{m}x{n}x{k}")
        _check("f32 bwd guarded dw", dw.t, *P.dw(True), "zero_mean", f"{m}x{n}x{k}")
    # f32 skinny
    m, n, k = 5, 100, 65664
    P = _problem(m, n, k, "zero_mean", False)
    ws = torch.empty(int(lib.pv_linear_fwd_f32_skinny_workspace_bytes(n)), dtype=torch.uint8, device=device)
    y, dx = Guarded((m, n), f32, device), Guarded((m, k), f32, device)
    K.check(lib.pv_linear_fwd_f32_skinny(held(P.x.to(device)), held(P.w.to(device)), None, ptr(y.t), m, n, k, 0, ptr(ws), ws.numel(), stream()),
            "pv_linear_fwd_f32_skinny")
    K.check(lib.pv_linear_dx_f32_skinny(held(P.dy.to(device)), held(P.w.to(device)), ptr(dx.t), m, n, k, stream()), "pv_linear_dx_f32_skinny")
    guards(y, dx)
    _check("f32 skinny fwd lds", y.t, *P.fwd(False, False), "zero_mean", "5x100x65664 guarded")
    _check("f32 skinny dx", dx.t, *P.dx(False), "zero_mean", "5x100x65664 guarded")
    # Adam, 1027 elements, every form
    p, mm, v, g = _adam_inputs(1027)
    for form in ("single", "multi", "multi-dev", "bf16 gradient"):
        st = [Guarded((1027,), f32, device, t) for t in (p, mm, v)] + [Guarded((1027,), b16, device, p.to(b16))]
        gd = g.to(b16).to(device) if form == "bf16 gradient" else g.to(device)
        item = [(st[0].t, gd, st[1].t, st[2].t, st[3].t)]
        if form == "single":
            K.adam_step(st[0].t, gd, st[1].t, st[2].t, 3, bf16_shadow=st[3].t)
        elif form == "multi":
            K.adam_step_multi(item, 3)
        elif form == "multi-dev":
            K.adam_step_multi_dev(item, scal)
        else:
            K.adam_step_bf16grad(st[0].t, gd, st[1].t, st[2].t, 3, bf16_shadow=st[3].t)
        guards(*st)
        _adam_check(f"Adam {form}", [t.t for t in st[:3]], _adam64(p, mm, v, _bf16(g) if form == "bf16 gradient" else g, sc), "1027 elements guarded")
        assert _shadow_is_rounded_p(st[3].t, st[0].t)


# ---- the table in the module docstring -----------------------------------------------------------------------------------------
def _measure():
    worst = {r: [0.0, 0.0] for r in REGIMES}
    worst_pair = 0.0
    per_family = {}
    for family, shape, regime in TABLE_CASES:
        for e in _evals(family, shape, regime):
            r32, rp = e.r32(), e.rpair()
            col = 0 if "float32 torch" in e.what else 1
            worst[regime][col] = max(worst[regime][col], r32)
            worst_pair = max(worst_pair, rp)
            key = (family.split(":")[0] if family.startswith("f32_fwd") else family, regime)
            cur = per_family.setdefault(key, [0.0, 0.0, 0.0])
            cur[col], cur[2] = max(cur[col], r32), max(cur[2], rp)
            print(f"    {family:<22} {_sid(shape):<14} {regime:<10} {e.what:<18} {r32:6.2f} x 2^-24 S" + (f"   split {rp:5.2f} x 2^-16 S" if e.pair else ""))
    print()
    for (family, regime), (t32, emu, rp) in sorted(per_family.items()):
        print(f"    {family:<16} {regime:<10} {t32:5.2f} / {emu:5.2f}" + (f"   split {rp:4.2f}" if rp else ""))
    for regime in REGIMES:
        print(f"worst {regime}: float32 torch {worst[regime][0]:.2f}, emulation {worst[regime][1]:.2f} -> C = {4 * max(worst[regime]):.1f}")
    print(f"worst split: {worst_pair:.3f} -> C_pair = {4 * worst_pair:.2f}")
    adam = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step, scale in ADAM_CASES:
        sc = _scalars(step)
        for size in ADAM_SIZES:
            p, m, v, g = _adam_inputs(size)
            ref = _adam64(p, m, v, g * scale, sc)
            for name, x, r, s in zip("pmv", _adam32(p, m, v, g * scale, sc), ref[:3], ref[3:]):
                adam[name] = max(adam[name], _ratio_to(x, r, U32 * s))
    for family, (m, n, k) in FUSED:
        p0, m0, v0 = _adam_state(n, k)
        P = _problem(m, n, k, "zero_mean", family != "f32_wgrad_adam", family != "f32_wgrad_adam", 1e-2)
        g32 = (P.g32(True).t() @ P.x)
        ref = _adam64(p0, m0, v0, g32, _scalars(3))
        for name, x, r, s in zip("pmv", _adam32(p0, m0, v0, g32, _scalars(3)), ref[:3], ref[3:]):
            adam[name] = max(adam[name], _ratio_to(x, r, U32 * s))
    for name in "pmv":
        print(f"worst Adam line {name}: {adam[name]:.3f} -> C_adam[{name}] = {4 * adam[name]:.2f}")


if __name__ == "__main__":
    _measure()
