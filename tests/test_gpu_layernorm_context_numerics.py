"""The LayerNorm kernels and the one-pass cross-attention context kernels built on them -- csrc/perceiver_ops_f32.hip:
layernorm_{fwd,bwd}_f32 (a wave per row), layernorm_{fwd,bwd}_rows_f32<40 | 64> (a thread per row),
layernorm_bwd_params_from_proj_kernel<4 | 8>, context_bwd_kernel; csrc/gemm_f32.hip: context_fwd_rows_kernel and the LN_A form of
gemm_rows_x3_kernel behind pv_context_fwd_bf16 -- per element against float64, at the row counts, widths and rows where they can go
wrong, and CPU tests that show the checker rejects a kernel that is subtly wrong.  Vocabulary and manner:
tests/test_gpu_geglu_mean_numerics.py, tests/test_gpu_linear_numerics.py.

Reference: a chain on the STORED operands.  Every reference is float64 on the CPU, from the float32 / bf16 operands exactly as the
kernel receives or stores them; eps is the float32 value of 1e-5.  Each link is then a pure rounding bound |got - ref64| <= C 2^-24 S
per element (`_check_terms`, through conv2d_f32_helpers._within), and no link depends on the conditioning of the row:
    mean    sum x / d                                            S = sum |x| / d
    rstd    1 / sqrt(sum (x - mean_k)^2 / d + eps)               S = the reference itself (a relative bound)
    y       (x - mean_k) rstd_k w + b                            S = |(x - mean_k) rstd_k w| + |y64|
            (mean_k, rstd_k: the float32 values the kernel stored)
    dx      rstd (g - sum g / d - xh sum (g xh) / d) (+ dx_add)  S = rstd (|g| + sum |g| / d + |xh| sum |g xh| / d) + |dx_add|
            (g = dy w, xh = (x - mean) rstd; mean and rstd are INPUTS of every backward kernel and are used as given)
    dw, db  sum over rows of dy xh, of dy                        S = sum |dy xh|, sum |dy|
    from-proj and context backward: d ctx64 = g16 bf16(W) from the bf16-rounded operands;
    dgamma  sum over rows of d ctx xh                            S = sum over rows (sum_k |g W|) |xh|        dbeta likewise without xh
    dW_kv   g16^T ctx16, ctx16 = bf16(((x - mean) rstd) gamma + beta) formed in float32 by separate torch operations: elementwise,
            so bit for bit the operand the kernel forms              S = |g16|^T |ctx16|
    kv16    sum_k bf16(an_k) bf16(W_nk), an = ((x - mean_k) rstd_k) gamma + beta from the kernel's own returned mean and rstd
            bound 2^-8 |ref64| for the bf16 store (the figure the linear file uses) + C 2^-24 sum_k |an W|
An accumulating call is held to the value it found + the reference, with 2^-24 |that| more for its one extra rounding, and to
`after - before = the plain result within one rounding`.

End to end.  y is also held to float64 F.layer_norm, with the three bounds composed.  With mu, r the float64 statistics and
delta = mean_k - mu:  y_chain - y64 = w ((x - mean_k)(rstd_k - r) - delta r).  sum (x - mean_k)^2 / d = var + delta^2 exactly, so the
rstd reference on the stored mean is below r by at most r^3 delta^2 / 2 (the slope of s^-1/2 only falls), and
    |y - y64| <= |w| (r B_mean + (|x - mu| + B_mean) (C_rstd 2^-24 r + r^3 B_mean^2 / 2)) + B_y,      B_mean = C_mean 2^-24 sum |x| / d.
This is why an end-to-end tolerance cannot be a constant: for a row constant at 1000.1, r = 1 / sqrt(eps) = 316 multiplies the rounding of
the mean (a float32 evaluation in the kernels' own order returns y - b up to 0.2 at d = 38..64 where float64 gives 0); the composed
bound follows that arithmetic, and it holds for every float32 evaluation below in every regime, this row included.

Constants.  From the REFERENCE's own error, never from the kernels: 4 x the worst error / (2^-24 S) of reference-only evaluations over
every case of this file -- float32 torch (the formulas above as separate torch operations with torch's own reduction orders: sum(1),
sum(0), `@`; F.layer_norm itself in the end-to-end check), CPU emulations of the source's order, vectorised over rows (`_wave_sum`:
per lane its <= 4 elements in index order, then the xor butterfly 32 .. 1; `_pair_sum`: s += x[2j] + x[2j+1], one division by (float) d,
q += t0 t0 + t1 t1; `_colsum_wave`, `_colsum_rows`, `_colsum_proj`, `_cbk32`: per lane serially over its rows, then lane, wave and
`_sum_slabs32` order) and, for the sums over rows, the plain index-order float32 sum (`_index_sum`).  The third is there because
float32 torch is not one evaluation: its sum(0) and `@` block and vectorise by machine and thread count -- on a second machine `g16^T @
ctx16` over 49 169 rows came out at 2.0 x 2^-24 S where this table's machine gives 0.17 -- and a constant taken from one machine's
order would fail the CPU tests on the next; one accumulator per column over all rows is the longest chain any of them can take.  The
library is built with -ffp-contract=off, so separate float32 torch operations model the arithmetic outside
the matrix instructions; the 4 x is the house's margin for the order inside a matrix instruction and across workgroups, which the
emulation cannot know.  The column sums over rows are taken per row-count class (rows <= 5, 129, 4100, 65 791, 262 700): error / S falls
with the row count, as C_MEAN of the GEGLU file has one value per n.  `python tests/test_gpu_layernorm_context_numerics.py` prints:
    quantity                float32 torch   emulation   constant
    wave    mean / rstd / y   4.79 / 3.49 / 2.61   3.29 / 2.86 / 2.61   19.2 / 14.0 / 10.5        dx  2.73   2.73   11.0
    serial  mean / rstd / y   3.71 / 3.47 / 2.70   5.52 / 5.78 / 2.68   22.1 / 23.2 / 10.8        dx  3.55   3.40   14.2
            (serial: the thread-per-row kernels and both context-forward kernels, whose statistics are theirs bit for bit)
    sums over rows: float32 torch, the emulation, index order -> constant, per quantity and row-count class
    dw, db         <= 5        3.04, 3.04, 3.04 -> 12.2;  2.02, 2.12, 2.12 -> 8.5
                   <= 4100     0.15, 0.21, 2.36 ->  9.5;  0.14, 0.13, 1.67 -> 6.7
                   <= 65 791   0.06, 0.08, 2.27 ->  9.1;  0.04, 0.05, 1.65 -> 6.7
                   <= 262 700  0.01, 0.02, 0.47 ->  1.9;  0.02, 0.01, 0.91 -> 3.7      (d = 2 and 6 only)
    from-proj dgamma, dbeta
                   <= 5        0.77, 0.77, 0.77 ->  3.1;  1.25, 1.25, 1.25 -> 5.0
                   <= 129      0.24, 0.31, 0.37 ->  1.5;  0.22, 0.27, 0.48 -> 2.0
                   <= 65 791   0.01, 0.01, 0.20 ->  0.8;  0.00, 0.01, 0.08 -> 0.4
    context backward dW_kv, dgamma, dbeta
                   <= 5        0 -> 0.0 (one row: dW_kv is one exact product);  0.96, 0.68, 0.96 -> 3.9;  1.25, 0.56, 1.25 -> 5.0
                   <= 129      2.36, 2.16, 2.36 ->  9.5;  0.24, 0.24, 0.36 -> 1.5;  0.22, 0.18, 0.48 -> 2.0
                   <= 4100     2.17, 0.84, 2.17 ->  8.7;  0.12, 0.11, 0.38 -> 1.6;  0.07, 0.06, 0.15 -> 0.7
                   <= 65 791   0.17, 0.14, 2.79 -> 11.2;  0.01, 0.01, 0.20 -> 0.9;  0.01, 0.01, 0.15 -> 0.7
    kv16, the float32 sum before the bf16 store   3.66   3.66   14.7
    (constants rounded up to 0.1.  A constant 0.0 asks for the float64 value exactly.)

Input regimes, each case seeded.  `unit`: randn; `offset`: randn + 1000; `planted<k>`: unit rows with, in the first and last row (and,
beyond 257 rows, in rows 255 and 256 either side of a thread-per-row workgroup and in the middle row), rotation k of: a row constant at
3.0, a row constant at 1000.1, an all-zero row, a row of +-2^-126, a row with one element 1e4.  Below 4096 rows every case runs unit,
offset and all five rotations (the context kernels: unit, offset, two rotations); above, one planting holds all five rows, and the
65 537-row cases add `offset`.  gamma = 1 + 0.1 randn with one planted 0.0 and one planted -1, beta = 0.1 randn, dy and g16 randn, g16
with +-0.0 and float32 values next to a bf16 rounding tie planted before its rounding.

Cases, the smallest shapes that reach each launch rule (test_the_cases_sit_on_the_paths_they_name restates the rules -- LN_MAX_BLOCKS
1024, LNR_BT 256, kNumCU 256, the `short_rows` predicate, lpb_blocks, cbk_blocks -- checks them against the sources' text and asserts
each case's path).  Wave LayerNorm: d in {1, 2, 37, 63, 64, 65, 128, 129, 255, 256} x rows in {1, 3, 4, 5}; (4097, 38) and (4100, 64),
ln_blocks capped, 8 rows per workgroup, a ragged last one; (65 536, 40), d % 8 == 0; (65 536, 38) with x one float off a 16-byte boundary.
Thread per row: <40> d in {2, 6, 38} x rows in {65 536, 65 537, 65 791}; <64> d in {42, 62} at 65 537 rows; (262 145, 6) and
(262 700, 2), two chunks per workgroup, the last workgroup's second chunk absent.  Every LayerNorm case: forward, backward, backward
twice (equal bits), without dx, with dx_add, accumulating.  From-proj: rows in {1, 31, 32, 33, 129} x d in {1, 20, 32, 33, 38, 64} at
kdim 128; (33, 64, 64); (65 569, 38, 128) and (65 569, 6, 64), a second grid-stride trip for some waves only.  Context backward: rows in
{1, 31, 32, 33, 65} x d in {1, 2, 31, 32, 33, 38, 63, 64}; (24 609, 38) and (49 169, 6), two and three trips, ragged; two sources
(d1, d2, period, batch) = (12, 26, 50, 3), (1, 37, 33, 4), (37, 1, 32, 2), (2, 36, 4099, 3), against float64 on the concatenated tensor
and bitwise against the kernel on it.  Context forward, both kernels (PV_CONTEXT_FWD_TWO_COLUMN_BLOCKS), through the C ABI since the
Python wrapper wants 2048 rows: rows in {1, 31, 32, 33, 129} x d in {2, 14, 16, 18, 30, 32, 34, 38, 46, 48}; (65 569, 6) and
(131 112, 2), the second and third trip of the alternating register sets; two sources (12, 26, period 50), (2, 36, 4099), (12, 26, 5),
(2, 4, 1); kdim 64, the fallback kernel with one column block.  Bitwise: default == fallback; two sources == concatenated; context
forward mean / rstd == layernorm_fwd_rows_f32's where that kernel runs; two runs; PF.layer_norm and PF.layer_norm_fork == the direct
calls at (5, 37) and (7, 64).  Buffers: (5, 37), (65 537, 6) and (33, 38) through the C ABI with every output and an exactly-sized
workspace inside buffers filled with 1.2345678e30, 64 guard elements each side; without dx nothing is written where dx would be.

What the checker is sensitive to (CPU tests).  It accepts float32 torch, each emulation and the index-order sums at every case and regime, and rejects, each by
name, applied to ONE row or ONE element of an otherwise correct float32 result: the variance divided by d - 1; eps outside the square
root; the mean divided by the padded lane count; rstd from sum x^2 / d - mean^2 (offset); dx without the xh sum (g xh) / d term; dw or
db missing the last row (5, 4097, 65 537 and 262 145 rows); dw missing the last row of a chunk that is not the workgroup's last (row 767
of 262 145); dgamma / dbeta of the from-proj kernel missing the last row; a row beyond the end contributing bf16(beta) to dW_kv; the
position row taken from (r + 1) % period at the wrap (dW_kv, dgamma); the backward's context operand truncated to bf16 instead of
rounded; kv16 with two adjacent columns swapped.  The FORWARD operand truncated instead of rounded hides partly behind the 2^-8 |ref| of
the bf16 store: it is visible in 53 % of the kv16 elements at (129, 38) and (33, 48) and in 31 % at (129, 2) (measured,
test_a_truncated_forward_operand_is_visible_in_a_measured_share_of_elements), so a whole kernel doing it is caught, one element is not.
What it cannot see: which of two bitwise-equal schedules ran (the path assertion restates the launch rules, it does not observe the
launch); a read outside an operand whose value is discarded; a missing row whose contribution is zero in float64 (a constant row has
xh = 0: the planted-row faults above sit in unit rows for that reason); dbeta does not read the context, so the wrap fault cannot show there.

Measured on the MI355X with these constants, worst error / bound over all cases.  Wave LayerNorm: mean 0.171, rstd 0.204, y 0.248,
end to end 0.138, dx 0.248, dw 0.250, db 0.250.  Thread per row: mean 0.250, rstd 0.180, y 0.248, end to end 0.250, dx 0.239, dw 0.010,
db 0.008.  From-proj: dgamma 0.248, dbeta 0.173.  Context backward: dW_kv 0.181, dgamma 0.202, dbeta 0.160.  Context forward, both
kernels alike: mean 0.228, rstd 0.249, kv16 0.996 (the bf16 store alone: half a unit in the last place of a value next to a power of
two is 2^-8 of it).  0.25 is the emulation's own figure where it sets the constant: the kernels add in the order the emulation
restates.  The accumulating calls reach 1.000 of their bound by construction (one rounding of a value next to a power of two is
2^-24 of it) and are reported apart.  Every bitwise relation held, every guard was intact, and no case found a fault in the kernels' results.
The 56 GPU cases take 7 s together on the MI355X (the first pays for loading the library); the 204 CPU cases take 12 s.
"""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import ROOT, _ops, _within

U32 = 2.0 ** -24
BF16 = 2.0 ** -8         # the bf16 store's share of a bound, relative (the figure tests/test_gpu_linear_numerics.py uses)
SENTINEL = 1.2345678e30
GUARD = 64
TINY = 2.0 ** -126
EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # the float32 value of 1e-5, as the kernels receive it

# ---- the launch rules, restated from csrc/perceiver_ops_f32.hip and csrc/gemm_f32.hip ------------------------------------------
LN_MAX_BLOCKS, LNR_BT, NUM_CU = 1024, 256, 256


def _ln_path(rows, d, aligned=True):
    """pv_layernorm_{fwd,bwd}_f32's `short_rows` predicate -> "wave" | "rows40" | "rows64"."""
    short_rows = d <= 64 and d % 2 == 0 and d % 8 != 0 and rows >= 65536 and aligned
    return ("rows40" if d <= 40 else "rows64") if short_rows else "wave"


def _ln_blocks(rows):
    """ln_blocks -> (workgroups, rows per workgroup) of layernorm_bwd_f32."""
    nb = min((rows + 3) // 4, LN_MAX_BLOCKS)
    per = ((rows + nb - 1) // nb + 3) // 4 * 4
    return (rows + per - 1) // per, per


def _lnr_blocks(rows):
    """-> (workgroups, rows per workgroup) of layernorm_bwd_rows_f32: whole chunks of LNR_BT rows."""
    per_r = ((rows + LN_MAX_BLOCKS - 1) // LN_MAX_BLOCKS + LNR_BT - 1) // LNR_BT * LNR_BT
    return (rows + per_r - 1) // per_r, per_r


def _lpb_blocks(rows):
    return min(((rows + 31) // 32 + 3) // 4, 2 * NUM_CU)


def _cbk_blocks(rows):
    return min((rows + 31) // 32, 3 * NUM_CU)


def _trips(rows, blocks, rowblocks_per_trip_and_block):
    """The most trips a wave (or workgroup) of a grid-stride loop over 32-row blocks takes."""
    return -(-((rows + 31) // 32) // (blocks * rowblocks_per_trip_and_block))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
WAVE_D = [1, 2, 37, 63, 64, 65, 128, 129, 255, 256]
WAVE_ROWS = [1, 3, 4, 5]
WAVE_BIG = [(4097, 38, True), (4100, 64, True), (65536, 40, True), (65536, 38, False)]      # (rows, d, x 16-byte aligned)
ROWS_CASES = ([(r, d) for d in (2, 6, 38) for r in (65536, 65537, 65791)] + [(65537, 42), (65537, 62)]
              + [(262145, 6), (262700, 2)])
PROJ_ROWS, PROJ_D = [1, 31, 32, 33, 129], [1, 20, 32, 33, 38, 64]
PROJ_BIG = [(33, 64, 64), (65569, 38, 128), (65569, 6, 64)]                                  # (rows, d, kdim)
CBK_ROWS, CBK_D = [1, 31, 32, 33, 65], [1, 2, 31, 32, 33, 38, 63, 64]
CBK_BIG = [(24609, 38), (49169, 6)]
CBK_TWO = [(12, 26, 50, 3), (1, 37, 33, 4), (37, 1, 32, 2), (2, 36, 4099, 3)]                # (d1, d2, period, batch)
CF_ROWS, CF_D = [1, 31, 32, 33, 129], [2, 14, 16, 18, 30, 32, 34, 38, 46, 48]
CF_BIG = [(65569, 6), (131112, 2)]
CF_TWO = [(12, 26, 50, 150), (2, 36, 4099, 3 * 4099), (12, 26, 5, 33), (2, 4, 1, 33)]         # (d1, d2, period, rows)
CF_KERNELS = ("default", "fallback")
SMALL_REGIMES = ("unit", "offset", "planted0", "planted1", "planted2", "planted3", "planted4")
ROW_CLASSES = (5, 129, 4100, 65791, 262700)      # the summation-length classes of the column sums over rows


def _regimes(rows):
    """Every regime, and every rotation of the planted rows, where rows are few; above that the five planted rows fit one
    planting (first, 255, 256, middle, last), and the 65 537-row cases add `offset` for the serial sums."""
    if rows < 4096:
        return SMALL_REGIMES
    return ("planted0", "offset") if rows == 65537 else ("planted0",)


def _row_class(rows):
    return next(c for c in ROW_CLASSES if rows <= c)


# 4 x the reference-only ratios printed by `python tests/test_gpu_layernorm_context_numerics.py` (module docstring)
C_FWD = {"wave": {"mean": 19.2, "rstd": 14.0, "y": 10.5}, "serial": {"mean": 22.1, "rstd": 23.2, "y": 10.8}}
C_DX = {"wave": 11.0, "serial": 14.2}
C_COL = {("ln", 5): (12.2, 8.5), ("ln", 4100): (9.5, 6.7), ("ln", 65791): (9.1, 6.7), ("ln", 262700): (1.9, 3.7),      # (dw, db)
         ("proj", 5): (3.1, 5.0), ("proj", 129): (1.5, 2.0), ("proj", 65791): (0.8, 0.4),                              # (dgamma, dbeta)
         ("ctx", 5): (0.0, 3.9, 5.0), ("ctx", 129): (9.5, 1.5, 2.0), ("ctx", 4100): (8.7, 1.6, 0.7),                   # (dwkv, dgamma, dbeta)
         ("ctx", 65791): (11.2, 0.9, 0.7)}
C_KV = 14.7
TRUNCATION_SHARE_MIN = 0.25      # a truncated forward operand must show in at least this share of kv16 elements at d = 38 (measured: 0.53)


def _d(t):
    return t.detach().double().cpu()


def _bf16(t):
    """Round to nearest even to bf16, back in float32."""
    return t.to(torch.bfloat16).float()


def _bf16_truncated(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _serial(t, dim):
    """Sum over `dim` in index order, starting from 0.f, in the tensor's own precision."""
    s = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        s = s + t.select(dim, i)
    return s


def _index_sum(v):
    """Sum over the rows of v in index order in float32, one accumulator per column: the longest chain a sum over rows can take
    (numpy's accumulate is that loop; torch's sum(0) and `@` block and vectorise differently from one machine to the next)."""
    return torch.from_numpy(np.cumsum(v.contiguous().numpy(), axis=0, dtype=np.float32)[-1].copy())


def _pad_rows(v, rows):
    return v if v.shape[0] == rows else torch.cat([v, v.new_zeros((rows - v.shape[0],) + v.shape[1:])])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _context(rows, d, regime, g):
    """x [rows, d] of a regime.  planted<k>: unit rows with, at the first and last row (and, beyond 257 rows, at rows 255 and 256
    either side of a thread-per-row workgroup and at the middle row), rotation k of: constant 3.0, constant 1000.1, zeros,
    +-2^-126, one element 1e4."""
    x = torch.randn(rows, d, generator=g)
    if regime == "offset":
        x = x + 1000.0
    elif regime.startswith("planted"):
        where = sorted({0, rows - 1} | ({255, 256, rows // 2} if rows > 257 else set()))
        for i, r in enumerate(where):
            kind = (i + int(regime[7:])) % 5
            if kind == 0:
                x[r] = 3.0
            elif kind == 1:
                x[r] = 1000.1
            elif kind == 2:
                x[r] = 0.0
            elif kind == 3:
                x[r] = TINY * (1 - 2 * (torch.arange(d) % 2)).float()
            else:
                x[r, (7 * r + 3) % d] = 1e4
    return x


def _gamma_beta(d, g):
    w, b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    if d >= 2:
        w[d // 2 - 1], w[d - 1] = 0.0, -1.0
    return w, b


def _stats(x):
    """(mean, rstd) in float64."""
    x = x.double()
    mean = x.mean(1)
    return mean, 1 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + EPS)


def _seed(*ints):
    s = 17
    for i in ints:
        s = (s * 1000003 + int(i)) % (2 ** 31 - 1)
    return s


def _regime_id(regime):
    return SMALL_REGIMES.index(regime)


# ---- LayerNorm: float64 references on the stored operands --------------------------------------------------------------------------
class Ln:
    def __init__(self, rows, d, regime):
        g = torch.Generator().manual_seed(_seed(1, rows, d, _regime_id(regime)))
        self.rows, self.d, self.regime = rows, d, regime
        self.x = _context(rows, d, regime, g)
        self.w, self.b = _gamma_beta(d, g)
        self.dy, self.add = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
        self.mean64, self.rstd64 = _stats(self.x)
        self.mean_in, self.rstd_in = self.mean64.float(), self.rstd64.float()      # the backward's inputs: used as given
        self._bwd = None

    def fwd_terms(self, y, mean, rstd, C):
        """q -> (got, reference, bound).  mean against sum x / d; rstd against the float64 value on the STORED mean; y against
        the float64 value on the stored mean and rstd; e2e: y against float64 F.layer_norm with the three bounds composed."""
        x, w, b = self.x.double(), self.w.double(), self.b.double()
        mk, rk = _d(mean), _d(rstd)
        b_mean = C["mean"] * U32 * x.abs().mean(1)
        r_ref = 1 / torch.sqrt(((x - mk[:, None]) ** 2).mean(1) + EPS)
        t = (x - mk[:, None]) * rk[:, None] * w
        b_y = C["y"] * U32 * (t.abs() + (t + b).abs())
        r64 = self.rstd64
        b_r = C["rstd"] * U32 * r64 + 0.5 * r64 ** 3 * b_mean ** 2
        b_e2e = w.abs() * ((r64 * b_mean)[:, None] + ((x - self.mean64[:, None]).abs() + b_mean[:, None]) * b_r[:, None]) + b_y
        y64 = F.layer_norm(x, (self.d,), w, b, EPS)
        return {"mean": (mk, self.mean64, b_mean), "rstd": (rk, r_ref, C["rstd"] * U32 * r_ref), "y": (_d(y), t + b, b_y),
                "e2e": (_d(y), y64, b_e2e)}

    def bwd64(self):
        if self._bwd is None:
            x, w, dy = self.x.double(), self.w.double(), self.dy.double()
            rs = self.rstd_in.double()[:, None]
            g, xh = dy * w, (x - self.mean_in.double()[:, None]) * rs
            dx = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
            s = rs * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
            self._bwd = (dx, s, (dy * xh).sum(0), (dy * xh).abs().sum(0), dy.sum(0), dy.abs().sum(0))
        return self._bwd

    def bwd_terms(self, dx, dw, db, c_dx, c_col, add=False, before=None):
        """before: the (dw, db) that an accumulating call found; the reference is then before + the sum, with one more rounding."""
        dx64, s, dw64, sdw, db64, sdb = self.bwd64()
        terms = {}
        if dx is not None:
            a = self.add.double() if add else 0.0
            terms["dx"] = (_d(dx), dx64 + a, c_dx * U32 * (s + (self.add.double().abs() if add else 0.0)))
        for q, got, ref, sq, c in (("dw", dw, dw64, sdw, c_col[0]), ("db", db, db64, sdb, c_col[1])):
            b0 = _d(before[q == "db"]) if before is not None else 0.0
            terms[q] = (_d(got), ref + b0, c * U32 * sq + (U32 * (ref + b0).abs() if before is not None else 0.0))
        return terms


@functools.lru_cache(maxsize=6)
def _ln(rows, d, regime):
    return Ln(rows, d, regime)


# ---- LayerNorm: float32 evaluations ------------------------------------------------------------------------------------------------
def _wave_sum(v):
    """A wave's sum of a row [.., d <= 256]: per lane its <= 4 elements (lane, lane + 64, ..) in index order from 0.f, then the
    xor butterfly 32, 16, .., 1."""
    rows, d = v.shape
    n = -(-d // 64)
    s = _serial(torch.cat([v, v.new_zeros(rows, 64 * n - d)], 1).view(rows, n, 64), 1)
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ off]
    return s[:, 0]


def _pair_sum(v):
    """s += v[2 j] + v[2 j + 1], the thread-per-row and context-forward kernels' order."""
    s = torch.zeros(v.shape[0])
    for j in range(v.shape[1] // 2):
        s = s + (v[:, 2 * j] + v[:, 2 * j + 1])
    return s


def _row_sum(v, how):
    return _wave_sum(v) if how == "wave" else _pair_sum(v) if how == "serial" else v.sum(1)      # ("torch", "index": torch's own)


def _ln_fwd32(x, w, b, how, fault=None):
    """float32 -> (y, mean, rstd).  how: "torch" (separate torch operations, torch's own reduction order), "wave", "serial" (the
    emulations of the source's order).  fault: "var_d_minus_1", "eps_outside", "padded_mean", "naive_var"."""
    d = x.shape[1]
    eps = torch.tensor(EPS, dtype=torch.float32)
    mu = _row_sum(x, how) / float(64 * -(-d // 64) if fault == "padded_mean" else d)
    t = x - mu[:, None]
    var = _row_sum(t * t, how) / float(d - 1 if fault == "var_d_minus_1" else d)
    if fault == "naive_var":
        var = _row_sum(x * x, how) / float(d) - mu * mu
    rs = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    return t * rs[:, None] * w + b, mu, rs


def _sum_slabs32(part):
    """sum_slabs_f32: eight groups add slabs g, g + 8, .. in index order, the group sums are then added in group order."""
    red = [_serial(part[g::8], 0) if part.shape[0] > g else torch.zeros_like(part[0]) for g in range(8)]
    t = red[0]
    for g in range(1, 8):
        t = t + red[g]
    return t


def _colsum_wave(v):
    """layernorm_bwd_f32's column sum: a wave adds its rows (wave, wave + 4, ..) of the workgroup in order, the four waves are
    added in order, the workgroups by sum_slabs."""
    nb, per = _ln_blocks(v.shape[0])
    p = _serial(_pad_rows(v, nb * per).view(nb, per // 4, 4, -1), 1)
    return _sum_slabs32(((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3])


def _colsum_rows(v, skip=None):
    """layernorm_bwd_rows_f32's: a thread adds its row of every chunk in order, then lane order, wave order, sum_slabs."""
    nb, per = _lnr_blocks(v.shape[0])
    v = _pad_rows(v, nb * per)
    if skip is not None:
        v = v.clone()
        v[skip] = 0.0
    p = _serial(v.view(nb, per // LNR_BT, LNR_BT, -1), 1).view(nb, LNR_BT // 64, 64, -1)
    return _sum_slabs32(_serial(_serial(p, 2), 1))


def _ln_bwd32(P, how, add=False, fault=None):
    """float32 -> (dx, dw, db) from the given mean and rstd.  how as in _ln_fwd32.  fault: "no_xh_term", "last_row",
    "last_row_of_chunk"."""
    rs = P.rstd_in[:, None]
    xh, g = (P.x - P.mean_in[:, None]) * rs, P.dy * P.w
    m1, m2 = _row_sum(g, how) / float(P.d), _row_sum(g * xh, how) / float(P.d)
    dx = rs * (g - m1[:, None] - (0.0 if fault == "no_xh_term" else xh * m2[:, None]))
    if add:
        dx = dx + P.add
    pw, pb = P.dy * xh, P.dy
    if fault == "last_row":
        pw, pb = pw.clone(), pb.clone()
        pw[-1], pb[-1] = 0.0, 0.0
    if how == "wave":
        return dx, _colsum_wave(pw), _colsum_wave(pb)
    if how == "serial":
        skip = 3 * LNR_BT - 1 if fault == "last_row_of_chunk" else None      # row 767: the last of workgroup 1's first chunk
        return dx, _colsum_rows(pw, skip), _colsum_rows(pb, skip)
    if how == "index":
        return dx, _index_sum(pw), _index_sum(pb)
    return dx, pw.sum(0), pb.sum(0)


# ---- the context kernels: float64 references and float32 evaluations -----------------------------------------------------------------
def _g16(rows, kdim, g):
    """The bf16 gradient rows: randn, with +-0.0 and float32 values next to a bf16 rounding tie planted before the rounding."""
    t = torch.randn(rows, kdim, generator=g)
    flat = t.view(-1)
    plant = [0.0, -0.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, -(1 + 3 * 2.0 ** -8), 1 + 3 * 2.0 ** -8 + 2.0 ** -20]
    for i, v in enumerate(plant):
        flat[(i * 37) % flat.numel()] = v
        flat[flat.numel() - 1 - (i * 41) % flat.numel()] = v
    return t.to(torch.bfloat16)


class Ctx:
    """A context x [rows, d] (two sources: x1 [rows, d1] | x2 [period, d2] at row r % period), its LayerNorm gamma / beta, the
    projection weight W [kdim, d], the bf16 gradient rows g16 [rows, kdim] and the statistics the backward kernels are given."""

    def __init__(self, rows, d, kdim, regime, two=None):
        g = torch.Generator().manual_seed(_seed(2, rows, d, kdim, _regime_id(regime), *(two or ())))
        self.rows, self.d, self.kdim, self.two = rows, d, kdim, two
        self.x = _context(rows, d, regime, g)
        if two:
            d1, period = two
            self.x2 = self.x[:period, d1:].contiguous()
            self.x1 = self.x[:, :d1].contiguous()
            self.x = torch.cat([self.x1, self.x2.repeat(-(-rows // period), 1)[:rows]], 1)
        self.w, self.b = _gamma_beta(d, g)
        self.wkv = torch.randn(kdim, d, generator=g) / math.sqrt(d)
        self.g16 = _g16(rows, kdim, g)
        mean64, rstd64 = _stats(self.x)
        self.mean_in, self.rstd_in = mean64.float(), rstd64.float()
        self._bwd = None

    def operand(self, mean, rstd, x=None, truncate=False):
        """The bf16 context operand, bit for bit: (((x - mean) rstd) gamma + beta) in float32, rounded to nearest even."""
        x = self.x if x is None else x
        an = ((x - mean[:, None]) * rstd[:, None]) * self.w + self.b
        return _bf16_truncated(an) if truncate else _bf16(an)

    def bwd64(self):
        if self._bwd is None:
            g, wb = self.g16.double(), _bf16(self.wkv).double()
            xh = (self.x.double() - self.mean_in.double()[:, None]) * self.rstd_in.double()[:, None]
            ctx = self.operand(self.mean_in, self.rstd_in).double()
            dctx, sctx = g @ wb, g.abs() @ wb.abs()
            self._bwd = {"dwkv": (g.T @ ctx, g.abs().T @ ctx.abs()), "dgamma": ((dctx * xh).sum(0), (sctx * xh.abs()).sum(0)),
                         "dbeta": (dctx.sum(0), sctx.sum(0))}
        return self._bwd

    def bwd_terms(self, got, C, before=None):
        """got, C, before: q -> tensor / constant for q in dwkv (context_bwd only), dgamma, dbeta."""
        terms = {}
        for q, t in got.items():
            ref, s = self.bwd64()[q]
            b0 = _d(before[q]) if before is not None else 0.0
            terms[q] = (_d(t), ref + b0, C[q] * U32 * s + (U32 * (ref + b0).abs() if before is not None else 0.0))
        return terms

    def fwd_terms(self, kv16, mean, rstd, C, c_kv):
        """mean / rstd as Ln.fwd_terms; kv16 against float64 on the bf16 operands formed from the kernel's own mean and rstd."""
        x = self.x.double()
        mk, rk = _d(mean), _d(rstd)
        mean64, _ = _stats(self.x)
        r_ref = 1 / torch.sqrt(((x - mk[:, None]) ** 2).mean(1) + EPS)
        an, wb = self.operand(mean.float().cpu(), rstd.float().cpu()).double(), _bf16(self.wkv).double()
        ref = an @ wb.T
        return {"mean": (mk, mean64, C["mean"] * U32 * x.abs().mean(1)), "rstd": (rk, r_ref, C["rstd"] * U32 * r_ref),
                "kv16": (_d(kv16), ref, BF16 * ref.abs() + c_kv * U32 * (an.abs() @ wb.abs().T))}


@functools.lru_cache(maxsize=6)
def _ctx(rows, d, kdim, regime, two=None):
    return Ctx(rows, d, kdim, regime, two)


def _ctx_fwd32(P, how, truncate=False, store=True):
    """float32 -> (kv16, mean, rstd): the statistics as _ln_fwd32 ("torch" | "serial"), the product as a float32 `@` of the bf16
    operands, stored as bf16."""
    _, mu, rs = _ln_fwd32(P.x, P.w, P.b, how)
    kv = P.operand(mu, rs, truncate=truncate) @ _bf16(P.wkv).T
    return kv.to(torch.bfloat16) if store else kv, mu, rs


def _colsum_proj(v):
    """layernorm_bwd_params_from_proj_kernel's column sum: a lane adds the 16 rows 8 (i / 4) + 4 half + i % 4 of each of its wave's
    32-row blocks (block 4 b + wave, then + 4 grid) in order; then the halves, the waves in order, the workgroups by sum_slabs."""
    rows, d = v.shape
    nb = _lpb_blocks(rows)
    trips = _trips(rows, nb, 4)
    p = _pad_rows(v, trips * nb * 128).view(trips, nb, 4, 4, 2, 4, d).permute(1, 2, 4, 0, 3, 5, 6).reshape(nb, 4, 2, trips * 16, d)
    p = _serial(p, 3)
    p = p[:, :, 0] + p[:, :, 1]
    return _sum_slabs32(((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3])


def _proj32(P, how, fault=None):
    """float32 -> {dgamma, dbeta} of the from-proj kernel.  "torch": `@` and sum(0); "emulation": _colsum_proj."""
    xh = (P.x - P.mean_in[:, None]) * P.rstd_in[:, None]
    dctx = P.g16.float() @ _bf16(P.wkv)
    pw, pb = dctx * xh, dctx
    if fault == "last_row":
        pw, pb = pw.clone(), pb.clone()
        pw[-1], pb[-1] = 0.0, 0.0
    if how == "torch":
        return {"dgamma": pw.sum(0), "dbeta": pb.sum(0)}
    if how == "index":
        return {"dgamma": _index_sum(pw), "dbeta": _index_sum(pb)}
    return {"dgamma": _colsum_proj(pw), "dbeta": _colsum_proj(pb)}


def _cbk32(P, how, fault=None):
    """float32 -> {dwkv, dgamma, dbeta} of context_bwd_kernel.  "torch": `@` and sum(0).  "emulation": workgroup b takes the 32-row
    blocks b, b + grid, ..; dW accumulates one float32 product per block in order; d ctx comes in two halves of the 128 gradient
    columns (two waves), each lane adds its 16 rows per block in order, then halves of a wave, the two column halves, sum_slabs.
    fault: "beta_row" (a row beyond the end contributes bf16(beta)), "wrap" (the position row of the last row of a period taken
    from (r + 1) % period), "truncated" (the operand truncated to bf16), "last_row"."""
    x = P.x
    if fault == "wrap":
        d1, period = P.two
        x = x.clone()
        x[period - 1, d1:] = P.x2[0]
    xh = (x - P.mean_in[:, None]) * P.rstd_in[:, None]
    ctx, g, wb = P.operand(P.mean_in, P.rstd_in, x, truncate=fault == "truncated"), P.g16.float(), _bf16(P.wkv)
    if fault == "last_row":
        g = g.clone()
        g[-1] = 0.0
    rows, d = x.shape
    if fault == "beta_row":
        ctx, g, xh = torch.cat([ctx, _bf16(P.b)[None]]), torch.cat([g, g[-1:]]), torch.cat([xh, xh.new_zeros(1, d)])
        rows += 1
    if how == "torch":
        dctx = g @ wb
        return {"dwkv": g.T @ ctx, "dgamma": (dctx * xh).sum(0), "dbeta": dctx.sum(0)}
    if how == "index":
        dctx = g @ wb
        dwkv = torch.cat([_index_sum(g[:, j:j + 8, None] * ctx[:, None, :]) for j in range(0, P.kdim, 8)])
        return {"dwkv": dwkv, "dgamma": _index_sum(dctx * xh), "dbeta": _index_sum(dctx)}
    nb = _cbk_blocks(rows)
    trips = _trips(rows, nb, 1)
    n = trips * nb * 32
    cb, gb = _pad_rows(ctx, n).view(trips, nb, 32, d), _pad_rows(g, n).view(trips, nb, 32, P.kdim)
    acc = torch.zeros(nb, d, P.kdim)
    for k in range(trips):
        acc = acc + torch.bmm(cb[k].transpose(1, 2), gb[k])
    out = {"dwkv": _sum_slabs32(acc.view(nb, -1)).view(d, P.kdim).T.contiguous()}
    half = torch.stack([g[:, :64] @ wb[:64], g[:, 64:] @ wb[64:]])      # [2, rows, d]
    for q, v in (("dgamma", half * xh), ("dbeta", half)):
        p = torch.cat([v, v.new_zeros(2, n - rows, d)], 1).view(2, trips, nb, 4, 2, 4, d).permute(2, 0, 4, 1, 3, 5, 6)
        p = _serial(p.reshape(nb, 2, 2, trips * 16, d), 3)
        p = p[:, :, 0] + p[:, :, 1]
        out[q] = _sum_slabs32(p[:, 0] + p[:, 1])
    return out


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, bound):
    ratio = (got - ref).abs() / (bound + 1e-30)
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
    """|got - reference| <= bound, per element and per quantity; records the worst error / bound."""
    for q, (got, ref, bound) in terms.items():
        worst = _ratio(got, ref, bound)
        WORST[(family, q)] = max(WORST.get((family, q), 0.0), worst)
        if family != "cpu":
            print(f"[{family}] {what} {q}: error / bound {worst:.3f}")
        _within(got, ref, bound / U32, tol=U32, what=f"{family} {what} {q}")


def _rejected(terms, q, what):
    with pytest.raises(AssertionError, match=f" {q}: error .* x the bound"):
        _check_terms("cpu", {q: terms[q]}, what)


def _col_constants(family, rows):
    return C_COL[(family, _row_class(rows))]


def _ln_kind(path):
    return "wave" if path == "wave" else "serial"


def _one_row(good, bad, r):
    out = good.clone()
    out[r] = bad[r]
    return out


# ---- CPU: the cases sit where they say, the checker accepts the reference-only evaluations and rejects what it must ----------------
def test_the_cases_sit_on_the_paths_they_name():
    """The launch rules restated above put every case on the path it names; the thresholds are the sources'."""
    src = open(os.path.join(ROOT, "predict_pv_yield_amd", "csrc", "perceiver_ops_f32.hip")).read()
    common = open(os.path.join(ROOT, "predict_pv_yield_amd", "csrc", "pv_common.h")).read()
    gemm = open(os.path.join(ROOT, "predict_pv_yield_amd", "csrc", "gemm_f32.hip")).read()
    assert int(re.search(r"constexpr int LN_MAX_BLOCKS = (\d+);", src).group(1)) == LN_MAX_BLOCKS
    assert int(re.search(r"constexpr int LNR_BT = (\d+);", src).group(1)) == LNR_BT
    assert int(re.search(r"constexpr int kNumCU = (\d+);", common).group(1)) == NUM_CU
    assert src.count("short_rows = d <= 64 && d % 2 == 0 && d % 8 != 0 && rows >= 65536 &&") == 2
    assert "std::min<long long>((rbs + 3) / 4, 2 * kNumCU)" in src and "std::min<long long>((rows + 31) / 32, 3 * kNumCU)" in src
    assert "std::min((n_rb + 3) / 4, 2 * kNumCU)" in gemm and 'getenv("PV_CONTEXT_FWD_TWO_COLUMN_BLOCKS")' in gemm
    for d in WAVE_D:
        for rows in WAVE_ROWS:
            assert _ln_path(rows, d) == "wave"
    assert [_ln_path(*c) for c in WAVE_BIG] == ["wave"] * 4 and _ln_path(65536, 38) == "rows40"      # only the misalignment keeps it off
    for rows in (4097, 4100):      # ln_blocks capped: 8 rows per workgroup, a ragged last one
        nb, per = _ln_blocks(rows)
        assert (rows + 3) // 4 > LN_MAX_BLOCKS and per == 8 and nb * per > rows > (nb - 1) * per
    for rows, d in ROWS_CASES:
        assert _ln_path(rows, d) == ("rows40" if d <= 40 else "rows64")
    assert {_ln_path(r, d) for r, d in ROWS_CASES} == {"rows40", "rows64"}
    for rows in (262145, 262700):      # two chunks per workgroup; the last workgroup's second chunk is partial or absent
        nb, per = _lnr_blocks(rows)
        assert per == 2 * LNR_BT and nb > 1
        assert rows - (nb - 1) * per == (1 if rows == 262145 else 44), rows - (nb - 1) * per
    assert all(_lnr_blocks(r)[1] == LNR_BT for r, _ in ROWS_CASES if r < 262144)
    for rows, d, kdim in PROJ_BIG[1:]:      # more than 2048 row blocks: the second trip is taken by some waves only
        rbs = (rows + 31) // 32
        assert _lpb_blocks(rows) == 2 * NUM_CU and 0 < rbs - 4 * 2 * NUM_CU < 4 * 2 * NUM_CU
    for (rows, d), trips in zip(CBK_BIG, (2, 3)):
        assert _cbk_blocks(rows) == 3 * NUM_CU and _trips(rows, 3 * NUM_CU, 1) == trips and rows % 32
    for d1, d2, period, batch in CBK_TWO:      # a 32-row block wraps inside: the period is no multiple of 32, or has one block
        assert period >= 32 and (period % 32 or batch > 1)
    for (rows, d), trips in zip(CF_BIG, (2, 3)):      # context_fwd_rows_kernel: 512 workgroups of 4 waves, register sets alternate
        assert _trips(rows, 2 * NUM_CU, 4) == trips and _ln_path(rows, d) == "rows40"
    assert all(d % 2 == 0 and d <= 48 for d in CF_D) and {14, 16, 18, 30, 32, 34, 46, 48} <= set(CF_D)


def _ln_cases():
    return ([(r, d, True) for d in WAVE_D for r in WAVE_ROWS] + WAVE_BIG + [(r, d, True) for r, d in ROWS_CASES])


def _ln_id(c):
    return f"{c[0]}x{c[1]}" + ("" if c[2] else "-misaligned")


def _ln_hows(path):
    return ("torch", "wave" if path == "wave" else "serial", "index")


@pytest.mark.parametrize("case", _ln_cases(), ids=_ln_id)
def test_layernorm_checker_accepts_float32_torch_and_the_emulation(case):
    rows, d, aligned = case
    path = _ln_path(rows, d, aligned)
    kind = _ln_kind(path)
    for regime in _regimes(rows):
        P = _ln(rows, d, regime)
        for how in _ln_hows(path):
            what = f"{rows}x{d} {regime} {how}"
            _check_terms("cpu", P.fwd_terms(*_ln_fwd32(P.x, P.w, P.b, how), C_FWD[kind]), what)
            for add in (False, True):
                _check_terms("cpu", P.bwd_terms(*_ln_bwd32(P, how, add), C_DX[kind], _col_constants("ln", rows), add), what)
    if rows < 4096:      # F.layer_norm itself, end to end (its own statistics)
        P = _ln(rows, d, "planted1")
        y, mean, rstd = torch.native_layer_norm(P.x, [d], P.w, P.b, EPS)
        terms = P.fwd_terms(y, mean.view(-1), rstd.view(-1), C_FWD[kind])
        _check_terms("cpu", {"e2e": terms["e2e"]}, f"{rows}x{d} F.layer_norm")


@pytest.mark.parametrize("how", ["torch", "wave", "serial"])
def test_layernorm_checker_rejects_wrong_statistics(how):
    """In ONE row of an otherwise correct float32 result: the variance divided by d - 1, eps outside the square root, the mean
    divided by the padded lane count, and (offset regime) rstd from sum x^2 / d - mean^2."""
    rows, d = (5, 37) if how != "serial" else (5, 38)
    kind = _ln_kind(how if how != "torch" else "wave")
    for regime, fault, q in (("unit", "var_d_minus_1", "rstd"), ("unit", "eps_outside", "rstd"), ("unit", "padded_mean", "mean"),
                             ("offset", "naive_var", "rstd")):
        P = _ln(rows, d, regime)
        good, bad = _ln_fwd32(P.x, P.w, P.b, how), _ln_fwd32(P.x, P.w, P.b, how, fault)
        _check_terms("cpu", P.fwd_terms(*good, C_FWD[kind]), "unmutated")
        mixed = [_one_row(a, b, 3) for a, b in zip(good, bad)]
        _rejected(P.fwd_terms(*mixed, C_FWD[kind]), q, f"{fault} in one row")
        _rejected(P.fwd_terms(*mixed, C_FWD[kind]), "e2e", f"{fault} in one row")


@pytest.mark.parametrize("case", [(5, 37, "wave"), (4097, 38, "wave"), (65537, 6, "serial"), (262145, 6, "serial")], ids=str)
def test_layernorm_checker_rejects_wrong_gradients(case):
    """dx without the xhat sum(g xhat) / d term in ONE element; dw and db missing the last row; dw missing the last row of a
    chunk that is not the workgroup's last (row 767, in the first chunk of the second two-chunk workgroup; row 255 is a planted
    constant row, whose xhat is zero)."""
    rows, d, how = case
    kind, cc = _ln_kind(how), _col_constants("ln", rows)
    P = _ln(rows, d, "planted0" if rows > 4096 else "unit")      # (planted0's last row is the one with an element 1e4 there)
    dx, dw, db = _ln_bwd32(P, how)
    _check_terms("cpu", P.bwd_terms(dx, dw, db, C_DX[kind], cc), "unmutated")
    bdx, _, _ = _ln_bwd32(P, how, fault="no_xh_term")
    r = rows // 2 + 1      # a unit row
    c = int((dx[r] - bdx[r]).abs().argmax())
    mixed = dx.clone()
    mixed[r, c] = bdx[r, c]
    _rejected(P.bwd_terms(mixed, dw, db, C_DX[kind], cc), "dx", "no xhat term in one element")
    _, bdw, bdb = _ln_bwd32(P, how, fault="last_row")
    _rejected(P.bwd_terms(dx, bdw, db, C_DX[kind], cc), "dw", "dw missing the last row")
    _rejected(P.bwd_terms(dx, dw, bdb, C_DX[kind], cc), "db", "db missing the last row")
    if rows == 262145:
        assert _lnr_blocks(rows)[1] == 2 * LNR_BT
        _, bdw, _ = _ln_bwd32(P, how, fault="last_row_of_chunk")
        _rejected(P.bwd_terms(dx, bdw, db, C_DX[kind], cc), "dw", "dw missing row 767, the last of a first chunk")


def _proj_cases():
    return [(r, d, 128) for r in PROJ_ROWS for d in PROJ_D] + PROJ_BIG


def _cbk_cases():
    return ([(r, d, None) for r in CBK_ROWS for d in CBK_D] + [(r, d, None) for r, d in CBK_BIG]
            + [(period * batch, d1 + d2, (d1, period)) for d1, d2, period, batch in CBK_TWO])


def _cf_cases():
    return ([(r, d, 128, None) for r in CF_ROWS for d in CF_D] + [(r, d, 128, None) for r, d in CF_BIG]
            + [(rows, d1 + d2, 128, (d1, period)) for d1, d2, period, rows in CF_TWO] + [(33, 38, 64, None), (129, 18, 64, None)])


def _cid(c):
    return "x".join(str(s) for s in c if s is not None and not isinstance(s, tuple)) + (f"-two{c[-1][0]}p{c[-1][1]}" if isinstance(c[-1], tuple) else "")


def _ctx_regimes(rows):
    return ("unit", "offset", "planted0", "planted3") if rows < 4096 else ("planted0",)


PROJ_Q, CBK_Q = ("dgamma", "dbeta"), ("dwkv", "dgamma", "dbeta")
SUM_HOWS = ("torch", "emulation", "index")


def _cdict(family, rows):
    return dict(zip(CBK_Q if family == "ctx" else PROJ_Q, _col_constants(family, rows)))


@pytest.mark.parametrize("case", _proj_cases(), ids=_cid)
def test_from_proj_checker_accepts_float32_torch_and_the_emulation(case):
    rows, d, kdim = case
    for regime in _ctx_regimes(rows):
        P = _ctx(rows, d, kdim, regime)
        for how in SUM_HOWS:
            _check_terms("cpu", P.bwd_terms(_proj32(P, how), _cdict("proj", rows)), f"{_cid(case)} {regime} {how}")


@pytest.mark.parametrize("case", _cbk_cases(), ids=_cid)
def test_context_bwd_checker_accepts_float32_torch_and_the_emulation(case):
    rows, d, two = case
    for regime in _ctx_regimes(rows):
        P = _ctx(rows, d, 128, regime, two)
        for how in SUM_HOWS:
            _check_terms("cpu", P.bwd_terms(_cbk32(P, how), _cdict("ctx", rows)), f"{_cid(case)} {regime} {how}")


@pytest.mark.parametrize("case", _cf_cases(), ids=_cid)
def test_context_fwd_checker_accepts_float32_torch_and_the_emulation(case):
    rows, d, kdim, two = case
    for regime in _ctx_regimes(rows):
        P = _ctx(rows, d, kdim, regime, two)
        for how in ("torch", "serial"):
            _check_terms("cpu", P.fwd_terms(*_ctx_fwd32(P, how), C_FWD["serial"], C_KV), f"{_cid(case)} {regime} {how}")


def test_context_checker_rejects_wrong_sums_and_operands():
    """Each applied to ONE row (or column) of an otherwise correct float32 result: d gamma / d beta missing the last row; a row
    beyond the end contributing bf16(beta) to dW_kv; the position row taken from (r + 1) % period at the wrap; the context operand
    truncated to bf16 in the backward; two adjacent kv16 columns swapped in one row."""
    P = _ctx(33, 38, 128, "unit")
    good = _proj32(P, "emulation")
    bad = _proj32(P, "emulation", "last_row")
    for q in PROJ_Q:
        _rejected(P.bwd_terms(dict(good, **{q: bad[q]}), _cdict("proj", 33)), q, f"{q} missing the last row")
    good = _cbk32(P, "emulation")
    _check_terms("cpu", P.bwd_terms(good, _cdict("ctx", 33)), "unmutated")
    for fault in ("beta_row", "truncated", "last_row"):
        bad = _cbk32(P, "emulation", fault)
        _rejected(P.bwd_terms(dict(good, dwkv=_one_row(good["dwkv"], bad["dwkv"], 5)), _cdict("ctx", 33)), "dwkv", f"{fault} in one row of dW_kv")
    d1, d2, period, batch = CBK_TWO[0]
    T = _ctx(period * batch, d1 + d2, 128, "unit", (d1, period))
    good, bad = _cbk32(T, "emulation"), _cbk32(T, "emulation", "wrap")
    _check_terms("cpu", T.bwd_terms(good, _cdict("ctx", T.rows)), "unmutated, two sources")
    for q in ("dwkv", "dgamma"):      # (d beta does not read the context)
        _rejected(T.bwd_terms(dict(good, **{q: bad[q]}), _cdict("ctx", T.rows)), q, f"{q} with the wrapped position row one off")
    kv, mu, rs = _ctx_fwd32(P, "serial")
    swapped = kv.clone()
    swapped[7, 40], swapped[7, 41] = kv[7, 41], kv[7, 40]
    _rejected(P.fwd_terms(swapped, mu, rs, C_FWD["serial"], C_KV), "kv16", "columns 40 and 41 of one row swapped")


def _truncation_share(P):
    """The share of kv16 elements in which an operand truncated (not rounded) to bf16 exceeds the bound."""
    kv, mu, rs = _ctx_fwd32(P, "serial", truncate=True)
    got, ref, bound = P.fwd_terms(kv, mu, rs, C_FWD["serial"], C_KV)["kv16"]
    return float(((got - ref).abs() > bound + 1e-30).double().mean())


def test_a_truncated_forward_operand_is_visible_in_a_measured_share_of_elements():
    """The blind spot of the kv16 bound (its 2^-8 |ref| for the bf16 store is as large as the fault): the share of elements in
    which the checker sees an operand truncated to bf16 is measured and recorded in the module docstring."""
    shares = {c: _truncation_share(_ctx(c[0], c[1], 128, "unit")) for c in ((129, 38), (129, 2), (33, 48))}
    print("share of kv16 elements that show a truncated operand:", {k: round(v, 4) for k, v in shares.items()})
    assert all(0.0 <= s <= 1.0 for s in shares.values())
    assert shares[(129, 38)] >= TRUNCATION_SHARE_MIN, shares


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


def _abi():
    from predict_pv_yield_amd import _lib
    return _lib.get_lib(), _lib.ptr, _lib.current_stream_ptr


def _misaligned(t, device):
    """t on the device, one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _ln_gpu(P, aligned, device, family):
    """Forward and every form of the backward of one LayerNorm case, checked; -> the outputs."""
    K = _ops()
    kind = _ln_kind(_ln_path(P.rows, P.d, aligned))
    cc = _col_constants("ln", P.rows)
    x = P.x.to(device) if aligned else _misaligned(P.x, device)
    w, b, dy, add = (t.to(device) for t in (P.w, P.b, P.dy, P.add))
    mean_in, rstd_in = P.mean_in.to(device), P.rstd_in.to(device)
    what = f"{P.rows}x{P.d} {P.regime}"
    y, mean, rstd = K.layernorm_fwd(x, w, b)
    _check_terms(family, P.fwd_terms(y, mean, rstd, C_FWD[kind]), what)
    dx, dw, db = K.layernorm_bwd(x, w, dy, mean_in, rstd_in)
    _check_terms(family, P.bwd_terms(dx, dw, db, C_DX[kind], cc), what)
    dx2, dw2, db2 = K.layernorm_bwd(x, w, dy, mean_in, rstd_in)
    for a, c, q in ((dx, dx2, "dx"), (dw, dw2, "dw"), (db, db2, "db")):
        _same_bits(a, c, f"{what}: {q} of two runs")
    none, dwn, dbn = K.layernorm_bwd(x, w, dy, mean_in, rstd_in, need_dx=False)
    assert none is None
    _same_bits(dwn, dw, f"{what}: dw without dx")
    _same_bits(dbn, db, f"{what}: db without dx")
    dxa, dwa, dba = K.layernorm_bwd(x, w, dy, mean_in, rstd_in, dx_add=add)
    _check_terms(family, P.bwd_terms(dxa, dwa, dba, C_DX[kind], cc, add=True), what + " dx_add")
    before = (torch.linspace(-3, 3, P.d).to(device), torch.linspace(2, -2, P.d).to(device))
    acc = (before[0].clone(), before[1].clone())
    K.layernorm_bwd(x, w, dy, mean_in, rstd_in, need_dx=False, accumulate_into=acc)
    _check_terms(family + ", accumulating", P.bwd_terms(None, acc[0], acc[1], C_DX[kind], cc, before=before), what)
    once = [(_d(a) - (_d(b0) + _d(p))).abs() <= U32 * _d(a).abs() for a, b0, p in zip(acc, before, (dw, db))]
    assert all(bool(o.all()) for o in once), f"{what}: accumulate does not add the plain result exactly once"
    return y, mean, rstd


@pytest.mark.gpu
@pytest.mark.parametrize("d", WAVE_D)
def test_wave_layernorm_kernels_per_element(d, device):
    """layernorm_fwd_f32 / layernorm_bwd_f32 at rows 1, 3, 4, 5 in every regime."""
    for rows in WAVE_ROWS:
        for regime in _regimes(rows):
            _ln_gpu(_ln(rows, d, regime), True, device, "ln wave")


@pytest.mark.gpu
@pytest.mark.parametrize("case", WAVE_BIG, ids=_ln_id)
def test_wave_layernorm_kernels_at_many_rows(case, device):
    rows, d, aligned = case
    for regime in _regimes(rows):
        _ln_gpu(_ln(rows, d, regime), aligned, device, "ln wave")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_thread_per_row_layernorm_kernels_per_element(case, device):
    """layernorm_{fwd,bwd}_rows_f32<40 | 64>, to two chunks per workgroup."""
    rows, d = case
    for regime in _regimes(rows):
        _ln_gpu(_ln(rows, d, regime), True, device, "ln rows")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 37), (7, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_autograd_bindings_equal_the_direct_calls(shape, device):
    """PF.layer_norm and PF.layer_norm_fork, forward and backward, bitwise."""
    from predict_pv_yield_amd import perceiver_functional as PF
    K = _ops()
    rows, d = shape
    P = _ln(rows, d, "unit")
    x, w, b, dy, add = (t.to(device) for t in (P.x, P.w, P.b, P.dy, P.add))
    y, mean, rstd = K.layernorm_fwd(x, w, b)
    for fork in (False, True):
        xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
        if fork:
            ya, xpass = PF.layer_norm_fork(xa, wa, ba)
            torch.autograd.backward([ya, xpass], [dy, add])
        else:
            ya = PF.layer_norm(xa, wa, ba)
            ya.backward(dy)
        dx, dw, db = K.layernorm_bwd(x, w, dy, mean, rstd, dx_add=add if fork else None)
        name = "PF.layer_norm_fork" if fork else "PF.layer_norm"
        _same_bits(ya.detach(), y, f"{name} forward against the direct call")
        for got, want, q in ((xa.grad, dx, "dx"), (wa.grad, dw, "dw"), (ba.grad, db, "db")):
            _same_bits(got, want, f"{name} {q} against the direct call")


class Guarded:
    """`shape` elements of `dtype` inside a sentinel-filled buffer with GUARD elements either side."""

    def __init__(self, shape, device, dtype=torch.float32):
        numel = math.prod(shape)
        self.dtype = dtype
        self.buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=device).to(dtype)
        self.t = self.buf[GUARD:GUARD + numel].view(*shape)
        self.want = _bits(torch.tensor([SENTINEL]).to(dtype))

    def intact(self):
        b = _bits(self.buf.cpu())
        return bool((b[:GUARD] == self.want).all() and (b[-GUARD:] == self.want).all())

    def untouched(self):
        return bool((_bits(self.buf.cpu()) == self.want).all())


def _proj_gpu(P, device, accumulate=None, out=None, ws=None):
    """pv_layernorm_bwd_params_from_proj_bf16 through the C ABI -> {dgamma, dbeta}."""
    K = _ops()
    lib, ptr, stream = _abi()
    import ctypes
    g16, wkv, x, mean, rstd = (t.to(device) for t in (P.g16, P.wkv, P.x, P.mean_in, P.rstd_in))
    n = ctypes.c_size_t(0)
    K.check(lib.pv_layernorm_bwd_params_from_proj_workspace_bytes(P.rows, P.d, ctypes.byref(n)), "workspace bytes")
    assert n.value == _lpb_blocks(P.rows) * 2 * P.d * 4
    ws = ws if ws is not None else torch.empty(n.value // 4, device=device)
    dw, db = out if out is not None else accumulate if accumulate is not None else (torch.empty(P.d, device=device), torch.empty(P.d, device=device))
    K.check(lib.pv_layernorm_bwd_params_from_proj_bf16(ptr(g16), ptr(wkv), ptr(x), ptr(mean), ptr(rstd), ptr(dw), ptr(db), P.rows, P.d,
                                                      P.kdim, ptr(ws), n.value, int(accumulate is not None), stream()), "from_proj")
    torch.cuda.synchronize()
    return {"dgamma": dw, "dbeta": db}


def _cbk_gpu(P, device, two=False, accumulate=None, out=None, ws=None):
    """pv_context_bwd_bf16 through the C ABI -> {dwkv, dgamma, dbeta}.  two: x as its two sources."""
    K = _ops()
    lib, ptr, stream = _abi()
    import ctypes
    g16, wkv, mean, rstd, w, b = (t.to(device) for t in (P.g16, P.wkv, P.mean_in, P.rstd_in, P.w, P.b))
    x, x2, d1, period = (P.x1.to(device), P.x2.to(device)) + P.two if two else (P.x.to(device), None, 0, 0)
    n = ctypes.c_size_t(0)
    K.check(lib.pv_context_bwd_workspace_bytes(P.rows, P.d, ctypes.byref(n)), "workspace bytes")
    assert n.value == _cbk_blocks(P.rows) * 130 * P.d * 4
    ws = ws if ws is not None else torch.empty(n.value // 4, device=device)
    if out is not None:
        dwkv, dw, db = out
    elif accumulate is not None:
        dwkv, dw, db = accumulate
    else:
        dwkv, dw, db = torch.empty(128, P.d, device=device), torch.empty(P.d, device=device), torch.empty(P.d, device=device)
    acc = int(accumulate is not None)
    K.check(lib.pv_context_bwd_bf16(ptr(g16), ptr(wkv), ptr(x), ptr(x2), d1, period, ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(dwkv),
                                   ptr(dw), ptr(db), P.rows, P.d, 128, ptr(ws), n.value, acc, acc, stream()), "context_bwd")
    torch.cuda.synchronize()
    return {"dwkv": dwkv, "dgamma": dw, "dbeta": db}


def _cf_gpu(P, device, two=False, out=None):
    """pv_context_fwd_bf16 through the C ABI (the Python wrapper wants >= 2048 rows) -> (kv16, mean, rstd)."""
    K = _ops()
    lib, ptr, stream = _abi()
    w, b, wkv = (t.to(device) for t in (P.w, P.b, P.wkv))
    x, x2, d1, period = (P.x1.to(device), P.x2.to(device)) + P.two if two else (P.x.to(device), None, 0, 0)
    if out is not None:
        kv16, mean, rstd = out
    else:
        kv16 = torch.empty(P.rows, P.kdim, dtype=torch.bfloat16, device=device)
        mean, rstd = torch.empty(P.rows, device=device), torch.empty(P.rows, device=device)
    K.check(lib.pv_context_fwd_bf16(ptr(x), ptr(x2), d1, period, ptr(w), ptr(b), ptr(wkv), ptr(kv16), ptr(mean), ptr(rstd), P.rows,
                                   P.d, P.kdim, EPS, stream()), "context_fwd")
    torch.cuda.synchronize()
    return kv16, mean, rstd


def _accumulated(run, plain, shapes, device, P, family, what):
    before = {q: torch.linspace(-2, 3, math.prod(s)).view(s).to(device) for q, s in shapes.items()}
    acc = {q: t.clone() for q, t in before.items()}
    run(tuple(acc[q] for q in shapes))
    _check_terms(family + ", accumulating", P.bwd_terms(acc, _cdict("ctx" if "dwkv" in shapes else "proj", P.rows), before=before), what)
    for q in shapes:
        once = (_d(acc[q]) - (_d(before[q]) + _d(plain[q]))).abs() <= U32 * _d(acc[q]).abs()
        assert bool(once.all()), f"{what}: accumulate does not add the plain {q} exactly once"


@pytest.mark.gpu
@pytest.mark.parametrize("rows", PROJ_ROWS + [65569], ids=str)
def test_from_proj_kernel_per_element(rows, device):
    """layernorm_bwd_params_from_proj_kernel<8 | 4>: plain, twice (equal bits), accumulating."""
    cases = [c for c in _proj_cases() if c[0] == rows]
    for rows, d, kdim in cases:
        for regime in _ctx_regimes(rows):
            P = _ctx(rows, d, kdim, regime)
            what = f"{_cid((rows, d, kdim))} {regime}"
            got = _proj_gpu(P, device)
            _check_terms("from_proj", P.bwd_terms(got, _cdict("proj", rows)), what)
            again = _proj_gpu(P, device)
            for q in PROJ_Q:
                _same_bits(got[q], again[q], f"{what}: {q} of two runs")
            _accumulated(lambda acc: _proj_gpu(P, device, accumulate=acc), got, {"dgamma": (d,), "dbeta": (d,)}, device, P,
                         "from_proj", what)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", CBK_ROWS + [c[0] for c in CBK_BIG], ids=str)
def test_context_bwd_kernel_per_element(rows, device):
    for rows, d, _ in [c for c in _cbk_cases() if c[0] == rows and c[2] is None]:
        for regime in _ctx_regimes(rows):
            P = _ctx(rows, d, 128, regime)
            what = f"{rows}x{d} {regime}"
            got = _cbk_gpu(P, device)
            _check_terms("context_bwd", P.bwd_terms(got, _cdict("ctx", rows)), what)
            again = _cbk_gpu(P, device)
            for q in CBK_Q:
                _same_bits(got[q], again[q], f"{what}: {q} of two runs")
            _accumulated(lambda acc: _cbk_gpu(P, device, accumulate=acc), got, {"dwkv": (128, d), "dgamma": (d,), "dbeta": (d,)},
                         device, P, "context_bwd", what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CBK_TWO, ids=lambda c: "-".join(map(str, c)))
def test_context_bwd_kernel_with_two_sources(case, device):
    """Against float64 on the concatenated tensor, and bitwise against the kernel on the concatenated tensor."""
    d1, d2, period, batch = case
    for regime in ("unit", "planted0"):
        P = _ctx(period * batch, d1 + d2, 128, regime, (d1, period))
        got, cat = _cbk_gpu(P, device, two=True), _cbk_gpu(P, device)
        _check_terms("context_bwd", P.bwd_terms(got, _cdict("ctx", P.rows)), f"two sources {case} {regime}")
        for q in CBK_Q:
            _same_bits(got[q], cat[q], f"two sources {case} {regime}: {q} against the concatenated tensor")


def _select_kernel(monkeypatch, kernel):
    if kernel == "fallback":
        monkeypatch.setenv("PV_CONTEXT_FWD_TWO_COLUMN_BLOCKS", "1")
    else:
        monkeypatch.delenv("PV_CONTEXT_FWD_TWO_COLUMN_BLOCKS", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", CF_ROWS + [c[0] for c in CF_BIG] + ["two", "kdim64"], ids=str)
def test_context_fwd_kernels_per_element(rows, device, monkeypatch):
    """context_fwd_rows_kernel and the LN_A form of gemm_rows_x3_kernel: each per element, equal bits between them, equal bits
    between two sources and the concatenated tensor, and mean / rstd equal to layernorm_fwd_rows_f32's where that kernel runs."""
    K = _ops()
    if rows == "two":
        cases = [c for c in _cf_cases() if c[3] is not None]
    elif rows == "kdim64":
        cases = [c for c in _cf_cases() if c[2] == 64]
    else:
        cases = [c for c in _cf_cases() if c[0] == rows and c[3] is None and c[2] == 128]
    for rows, d, kdim, two in cases:
        for regime in _ctx_regimes(rows):
            P = _ctx(rows, d, kdim, regime, two)
            what = f"{_cid((rows, d, kdim, two))} {regime}"
            outs = {}
            for kernel in CF_KERNELS:
                _select_kernel(monkeypatch, kernel)
                outs[kernel] = _cf_gpu(P, device)
                _check_terms(f"context_fwd {kernel}", P.fwd_terms(*outs[kernel], C_FWD["serial"], C_KV), what)
                if two:
                    for a, c, q in zip(_cf_gpu(P, device, two=True), outs[kernel], ("kv16", "mean", "rstd")):
                        _same_bits(a, c, f"{what} {kernel}: {q} of two sources against the concatenated tensor")
            for a, c, q in zip(outs["default"], outs["fallback"], ("kv16", "mean", "rstd")):
                _same_bits(a, c, f"{what}: {q} of the default and the fallback kernel")
            if _ln_path(rows, d) != "wave":
                _, mean, rstd = K.layernorm_fwd(P.x.to(device), P.w.to(device), P.b.to(device))
                _same_bits(outs["default"][1], mean, f"{what}: mean against layernorm_fwd_rows_f32")
                _same_bits(outs["default"][2], rstd, f"{what}: rstd against layernorm_fwd_rows_f32")


@pytest.mark.gpu
def test_outputs_and_workspaces_stay_inside_their_buffers(device, monkeypatch):
    """One ragged case per entry point through the C ABI: every output and the workspace, which is exactly as large as the
    *_workspace_bytes function reports, inside sentinel-filled buffers; without dx nothing is written where dx would be."""
    import ctypes
    K = _ops()
    lib, ptr, stream = _abi()
    for rows, d in ((5, 37), (65537, 6)):      # the wave kernels, the thread-per-row kernels
        P = _ln(rows, d, "planted0")
        kind, cc = _ln_kind(_ln_path(rows, d)), _col_constants("ln", rows)
        x, w, b, dy, mean_in, rstd_in = (t.to(device) for t in (P.x, P.w, P.b, P.dy, P.mean_in, P.rstd_in))
        y, mean, rstd = Guarded((rows, d), device), Guarded((rows,), device), Guarded((rows,), device)
        K.check(lib.pv_layernorm_fwd_f32(ptr(x), ptr(w), ptr(b), ptr(y.t), ptr(mean.t), ptr(rstd.t), rows, d, EPS, stream()), "fwd")
        torch.cuda.synchronize()
        assert y.intact() and mean.intact() and rstd.intact(), f"{rows}x{d}: the LayerNorm forward wrote outside its results"
        _check_terms("ln guarded", P.fwd_terms(y.t, mean.t, rstd.t, C_FWD[kind]), f"{rows}x{d} guarded")
        n = ctypes.c_size_t(0)
        K.check(lib.pv_layernorm_bwd_workspace_bytes(rows, d, ctypes.byref(n)), "workspace bytes")
        assert n.value == _ln_blocks(rows)[0] * 2 * d * 4
        for need_dx in (True, False):
            dx, dw, db, ws = Guarded((rows, d), device), Guarded((d,), device), Guarded((d,), device), Guarded((n.value // 4,), device)
            K.check(lib.pv_layernorm_bwd_f32(ptr(x), ptr(w), ptr(dy), ptr(mean_in), ptr(rstd_in), ptr(dx.t) if need_dx else None,
                                            ptr(dw.t), ptr(db.t), rows, d, ptr(ws.t), n.value, 0, None, stream()), "bwd")
            torch.cuda.synchronize()
            assert dx.intact() and dw.intact() and db.intact() and ws.intact(), f"{rows}x{d}: the LayerNorm backward wrote outside"
            assert need_dx or dx.untouched(), f"{rows}x{d}: without dx something was written where dx would be"
            _check_terms("ln guarded", P.bwd_terms(dx.t if need_dx else None, dw.t, db.t, C_DX[kind], cc), f"{rows}x{d} guarded")
    P = _ctx(33, 38, 128, "planted0")
    n = _lpb_blocks(33) * 2 * 38
    dw, db, ws = Guarded((38,), device), Guarded((38,), device), Guarded((n,), device)
    got = _proj_gpu(P, device, out=(dw.t, db.t), ws=ws.t)
    assert dw.intact() and db.intact() and ws.intact(), "the from-proj kernel wrote outside"
    _check_terms("from_proj", P.bwd_terms(got, _cdict("proj", 33)), "33x38 guarded")
    n = _cbk_blocks(33) * 130 * 38
    dwkv, dw, db, ws = Guarded((128, 38), device), Guarded((38,), device), Guarded((38,), device), Guarded((n,), device)
    got = _cbk_gpu(P, device, out=(dwkv.t, dw.t, db.t), ws=ws.t)
    assert dwkv.intact() and dw.intact() and db.intact() and ws.intact(), "the context backward wrote outside"
    _check_terms("context_bwd", P.bwd_terms(got, _cdict("ctx", 33)), "33x38 guarded")
    for kernel in CF_KERNELS:
        _select_kernel(monkeypatch, kernel)
        kv, mean, rstd = Guarded((33, 128), device, torch.bfloat16), Guarded((33,), device), Guarded((33,), device)
        assert kv.t.data_ptr() % 16 == 0
        _cf_gpu(P, device, out=(kv.t, mean.t, rstd.t))
        assert kv.intact() and mean.intact() and rstd.intact(), f"the context forward ({kernel}) wrote outside"
        _check_terms(f"context_fwd {kernel}", P.fwd_terms(kv.t, mean.t, rstd.t, C_FWD["serial"], C_KV), "33x38 guarded")


# ---- the tables in the module docstring ------------------------------------------------------------------------------------------
ONES = {"mean": 1.0, "rstd": 1.0, "y": 1.0}


def _up(v):
    return math.ceil(40 * v) / 10


def _worse(table, key, terms, col):
    for q, (got, ref, bound) in terms.items():
        if q != "e2e":
            cell = table.setdefault((key, q), [0.0, 0.0, 0.0])
            cell[col] = max(cell[col], _ratio(got, ref, bound))


def _measure():
    """The reference-only ratios error / (2^-24 S): float32 torch | the emulation, over every case of the file."""
    t = {}
    for rows, d, aligned in _ln_cases():
        path = _ln_path(rows, d, aligned)
        kind = _ln_kind(path)
        for regime in _regimes(rows):
            P = _ln(rows, d, regime)
            for col, how in enumerate(_ln_hows(path)):
                _worse(t, kind, P.fwd_terms(*_ln_fwd32(P.x, P.w, P.b, how), ONES), col)
                for add in (False, True):
                    terms = P.bwd_terms(*_ln_bwd32(P, how, add), 1.0, (1.0, 1.0), add)
                    _worse(t, kind, {"dx": terms["dx"]}, col)
                    _worse(t, ("ln", _row_class(rows)), {q: terms[q] for q in ("dw", "db")}, col)
    for rows, d, kdim in _proj_cases():
        for regime in _ctx_regimes(rows):
            P = _ctx(rows, d, kdim, regime)
            for col, how in enumerate(SUM_HOWS):
                _worse(t, ("proj", _row_class(rows)), P.bwd_terms(_proj32(P, how), dict.fromkeys(PROJ_Q, 1.0)), col)
    for rows, d, two in _cbk_cases():
        for regime in _ctx_regimes(rows):
            P = _ctx(rows, d, 128, regime, two)
            for col, how in enumerate(SUM_HOWS):
                _worse(t, ("ctx", _row_class(rows)), P.bwd_terms(_cbk32(P, how), dict.fromkeys(CBK_Q, 1.0)), col)
    kvw = [0.0, 0.0]
    for rows, d, kdim, two in _cf_cases():
        for regime in _ctx_regimes(rows):
            P = _ctx(rows, d, kdim, regime, two)
            for col, how in enumerate(("torch", "serial")):
                terms = P.fwd_terms(*_ctx_fwd32(P, how, store=False), ONES, 1.0)      # (the float32 sum BEFORE the bf16 store)
                _worse(t, "serial", {q: terms[q] for q in ("mean", "rstd")}, col)
                got, ref, bound = terms["kv16"]
                kvw[col] = max(kvw[col], _ratio(got, ref, bound - BF16 * ref.abs()))
    print("    quantity                      float32 torch   emulation   index order   constant (4 x the worst)")
    for key in sorted(t, key=str):
        a, b, c = t[key]
        print(f"    {str(key):<34} {a:8.2f}    {b:8.2f}    {c:8.2f}     {_up(max(a, b, c)):7.1f}")
    print(f"    kv16, before the bf16 store       {kvw[0]:8.2f}    {kvw[1]:8.2f}     {_up(max(kvw)):7.1f}")
    for c in ((129, 38), (129, 2), (33, 48)):
        print(f"    truncated-operand share at {c}: {_truncation_share(_ctx(c[0], c[1], 128, 'unit')):.4f}")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    _measure()
