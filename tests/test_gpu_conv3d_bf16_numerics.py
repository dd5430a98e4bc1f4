"""The bf16 Conv3D family -- conv3d_bf16.hip (the v1 marching kernel, CPAD 16 / 32, with and without a gate, both epilogues;
the packers), conv3d_bf16_v3.hip (the input-stationary 32 -> 32 kernel), conv3d_bf16_first.hip (the loader-wave first layer) and
conv3d_wgrad_bf16_v2.hip (the weight gradient and its slab reduce) -- per element against a float64 convolution, at the shapes
where each of their paths begins and ends; and CPU tests that show the checker rejects a convolution that is subtly wrong.

Reference.  Operands rounded once to bf16 (nearest even), everything else in float64 on the CPU (`_problem`):
  forward   y64 = conv3d(x, w) + bias, S = conv3d(|x|, |w|) + |bias|; under ReLU relu(y64) with the same S;
  dgrad     dx64 = conv_transpose3d(g * (y64 > 0), w), S = conv_transpose3d(|g| * (y64 > 0), |w|); the kernel is handed a gate
            image that is 1 where y64 > 0 and exactly +0 elsewhere (or g gated that way beforehand);
  wgrad     dw64[co, ci, tap] = sum over voxels of x[voxel + tap, ci] g[voxel, co] (g gated as above), S = the same sum of
            |x g| -- written as one einsum over the 27 shifted views of x (`_unfold`), which a CPU test compares with
            torch.nn.grad.conv3d_weight in float64;
  db        db64 = sum g, S = sum |g|.
Bound, per element, never a norm (`_check`, through conv2d_f32_helpers._within):
    |got - ref64| <= C 2^-24 S                               f32 outputs (dW, db)
    |got - ref64| <= C (1 + 2^-8) 2^-24 S + 2^-8 |ref64|     bf16 outputs (y, dx)
2^-8 is bfloat16's unit roundoff (tests/test_gpu_gemm_numerics.py says why it is not 2^-9); rounding an accumulator that is
itself off by C 2^-24 S adds 2^-8 of that.  Padded channels (y[..., c_out:], dx[..., c_in:]) must be exactly zero.

Regimes (seeded, on the CPU): `zero_mean` x randn, w randn / sqrt(27 ci), bias 0.1 randn, g randn; `relu_input` x = relu(randn)
(exact zeros, nothing negative: what every layer after the first sees), the rest as before.

Constants.  From the REFERENCE's own error, never from the kernels: worst err / (2^-24 S) over every (shape, regime) of this file
of (a) float32 torch (F.conv3d, its autograd gradients; for db torch's float32 sum and a plain one, voxel after voxel) on the
rounded operands and (b) the arithmetic the
kernel sources document (`_emulate_conv`: one f32 accumulator per output that starts from the bias and is updated once per
matrix-instruction k-step -- 16 channels of a tap for the 32x32x16 kernels, 32 for v3's 16x16x32 -- in the kernels' tap order
kt, kw, [channel half,] kh; `_emulate_wgrad`: per-workgroup slabs over (sample, row block, time chunk) as wgrad_v2_grid cuts them,
each an f32 accumulator updated once per 16 voxels walking column tile, slice, row, 16-column group; `_reduce_slabs`: 16 groups
take slabs g, g + 16, ... into four alternating partial sums, (s0 + s1) + (s2 + s3), then the pairwise tree), times 4 (the
margin for the unknown summation order inside a matrix instruction).  `python tests/test_gpu_conv3d_bf16_numerics.py` prints
the table; its summary (worst err / (2^-24 S): float32 torch / emulation):
    output extent, channels, padding        zero_mean                                   relu_input
    v3 2x1x1 b1 pad 000                     y 0.35 / 0.33                               y 0.26 / 0.46
    v3 3x8x31, 5x9x32 (100), 7x9x33         y <= 1.34 / 1.23                            y <= 1.10 / 1.41
    v3 8x8x64, 3x9x65 (222), b2 7x8x65      y <= 1.21 / 1.26                            y <= 1.36 / 1.87
    v3 b3 2x1x33 (111)                      y 0.81 / 0.92                               y 0.80 / 0.92
    v1 1 -> 32 1x8x61, 3 -> 32 2x9x62       y <= 1.73 / 1.53                            y <= 1.92 / 1.79
    v1 11 -> 32 3x9x63, 16 -> 32 2x8x124    y <= 1.83 / 1.32                            y <= 1.42 / 1.66
    v1 11 -> 4 b2 3x9x125, 16 -> 16 3x9x63  y <= 2.02 / 1.05                            y <= 1.37 / 1.29
    v1 32 -> 32 1x9x125, b2 1x8x62          y <= 1.20 / 1.11                            y <= 1.02 / 1.50
    v1 gated 11 -> 32 2x9x63, 32 -> 32      y <= 2.05 / 1.25                            y <= 1.72 / 1.60
    first 1 -> 32 2x8x62, 11 -> 32 3x9x63   y <= 1.94 / 1.75                            y <= 2.07 / 1.59
    first 16 -> 32 3x9x62, 11 -> 32 1x8x63  y <= 2.45 / 1.03                            y <= 1.44 / 1.48
    first 11 -> 32 2x9x126, 16 -> 16        y <= 1.93 / 1.38                            y <= 2.12 / 1.88
    dgrad cases (dx of 3x9x63 ... 2x9x125)  dx <= 1.30 / 1.58  dW <= 1.33 / 0.80        dx <= 1.68 / 2.00  dW <= 1.13 / 1.12
    wgrad ci 1, 3, 11, 12                   dx <= 0.97 / 1.32  dW <= 0.97 / 0.97        dx <= 1.00 / 1.79  dW <= 0.99 / 0.99
    wgrad ci 13, 16, 17, 32, 32             dx <= 1.50 / 1.70  dW <= 2.24 / 0.48        dx <= 1.27 / 1.62  dW <= 1.70 / 0.92
    wgrad b130 (260 slabs), b129            dx <= 1.52 / 1.31  dW <= 0.75 / 0.27        dx <= 1.42 / 1.22  dW <= 0.72 / 0.45
    db, every backward case                 <= 0.10 / 0.09                              <= 0.13 / 0.13
    worst y / dx: zero_mean 2.45 / 1.75 -> C["y"] = 9.8, relu_input 2.12 / 2.00 -> 8.5
    worst dW:     zero_mean 2.24 / 0.97 -> C["dw"] = 8.9, relu_input 1.70 / 1.12 -> 6.8
    worst db:     zero_mean 0.10 / 0.09 -> C["db"] = 0.4, relu_input 0.13 / 0.13 -> 0.5
(db is a sum of 8-bit numbers in a 24-bit accumulator: next to nothing is lost.  The float32 column of db is the larger of torch's
sum and the voxel-after-voxel one.)

What the checker is sensitive to (CPU tests below, on the small cases, where S has not outgrown the error).  Taking the float64
result, applying the mutation and rounding as the kernel would, the checker rejects: one tap dropped at the last valid column
of a ragged tile, the bias added twice or not at all, the output truncated to bf16 instead of rounded, the operands truncated
instead of rounded, a value leaking through a padded input channel (c_in = 11), dgrad gated on y >= 0 instead of y > 0 (with
exact zeros in y), dW without its last output column / its last time slice / one slab / one single voxel (at the largest N of
the file), db without one voxel, db from the ungated g.  The check of tests/test_gpu_conv.py (rtol 1e-2, atol 2e-3 for y and
dx; 2e-3 max|ref| + 1e-4 over the whole tensor for dW, db) lets through the truncated output and the padded-channel leak, which
these tests assert too; it does see the other mutations at these sizes (a missing voxel is |x g| ~ 1 against 2e-3 max|dW| ~ 0.1 at
N = 3 510: it would slip through only at sizes far beyond any test here).

GPU cases.  Tiles from the sources: v1 and first layer TR = 8 rows x TW_VALID = 62 columns, v3 8 x 32, wgrad 8 (or fewer:
rows-per-block rule) x 32.  Output extents (to, ho, wo) below.
  1 v3      V3_CASES, 32 -> 32 without a gate, to >= 2: wo 1, 31, 32, 33, 64, 65; ho 1, 8, 9; to 2, 3, 5 (chunks 3 + 2), 7 (a
            single-slice remainder folded into 4 + 3), 8 (2 + 2 + 2 + 2) -- `_v3_chunks` restates v3_grid and a CPU test asserts
            these cuts; padding (0,0,0), (1,0,0), (2,2,2), (1,1,1); ReLU on and off; NDHWC and NCDHW (wo % 8 == 0: v3's own
            epilogue; otherwise the launch falls to v1).
  2 v1      V1_CASES: CPAD 16 with ci 1, 3, 11, 16 -> 32 and c_out 4, 16; 32 -> 32 with to = 1; a gate handed over with ci 11
            (CPAD 16) and 32; wo 61, 62, 63, 124, 125; ho 8, 9; to 1, 2, 3; every padding 0 .. 2 on every axis; both epilogues.
  3 dgrad   DGRAD_CASES: transpose_flip weights, padding 2 - p, dx of ci 11 and 32 channels whose extent has ragged last tiles
            for both kernels; once with the gate as a bf16 tensor (v1, HAS_GATE) and once with g gated beforehand (v3).
  4 wgrad   WGRAD_CASES: ci 1, 3, 11, 12 (three pieces per tap), 13, 16 (paired), 17, 32; wo 1, 31, 32, 33, 65; ho 8, 9, 16, 17;
            to 1, 2, 5 at batch 1 (chunks 2 + 2 + 1); every padding 0 .. 2; g gated outside and a gate handed over.  At a small
            batch the rows-per-block rule always adds its block (ho 8 -> 2 x 4, 9 -> 3 x 3, 16 -> 3 x 6, 17 -> 4 x 5 with a last
            block of 2); batch 129 x ho 8 (one block of 8, 129 slabs) and batch 130 x ho 9 (two blocks of 5, 260 slabs: the
            reduce's outer loop takes a second trip) are the cases where it cannot.  Every case asserts its slab count, from
            `_wgrad_grid` (wgrad_v2_grid restated), against pv_conv3d_bwd_weight_bf16_workspace_bytes.
  5 first   FIRST_CASES through conv3d_fwd_bf16_f32in: w % 4 == 0 (loader waves) and w % 4 != 0 (v1's X_F32 form), ci 1, 11, 16,
            wo 62, 63, 126, t / h padding 0 .. 2; y against float64 of the ROUNDED x, the returned NDHWC image bit for bit
            x.to(bfloat16) with zero padded channels.
  6 packers pack_ncdhw_f32_to_ndhwc_bf16 and repack_gate_ncdhw_to_ndhwc_bf16 at t h w % 4 == 0 and != 0, bit for bit, on
            values that tell nearest-even from truncation and from round-half-up (`_special_f32`), +-0 in data and gate.
  7 exact homogeneity, one per family: x (and the bias) times 2^+-20 gives the unscaled bits times that power of two.

Measured on the MI355X with these constants, worst error / bound over all cases of a family:
  v3 0.995, v3 NCDHW 0.995, v1 0.995, v1 NCDHW 0.995, v1 gated 0.994, dgrad through v1 with a gate 0.995, dgrad through v3 0.995,
  first layer (loader waves) 0.995, first layer (v1's X_F32 form) 0.994 -- each of them the bf16 rounding term alone: a value half
  a step from both neighbours at the bottom of its binade; dW 0.146 ((1, 1 -> 32, 1x8x1) relu_input), db 0.259 ((2, 3 -> 32,
  2x9x31) relu_input: 0.13 x 2^-24 S, the emulation's own figure).  Every homogeneity and bit-for-bit case holds.  No case found
  a fault in the kernels.  The 94 GPU cases of this file take 3.6 s together, the slowest (v3 2x1x1, the first launch) 0.17 s.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _ops, _within

U32 = 2.0 ** -24
U16 = 2.0 ** -8          # unit roundoff of bfloat16 (8 significant bits)

# 4 x the reference-only ratios of the module docstring, per output kind and regime
C = {"y": {"zero_mean": 9.8, "relu_input": 8.5},          # y and dx
     "dw": {"zero_mean": 8.9, "relu_input": 6.8},
     "db": {"zero_mean": 0.4, "relu_input": 0.5}}
REGIMES = ("zero_mean", "relu_input")

Case = namedtuple("Case", "b ci co t h w pad")      # input extents; co output channels


def _c(b, ci, co, to, ho, wo, pad):
    """A case from its OUTPUT extent."""
    return Case(b, ci, co, to + 2 - 2 * pad[0], ho + 2 - 2 * pad[1], wo + 2 - 2 * pad[2], pad)


def _out(c):
    return c.t + 2 * c.pad[0] - 2, c.h + 2 * c.pad[1] - 2, c.w + 2 * c.pad[2] - 2


def _id(c):
    to, ho, wo = _out(c)
    return f"b{c.b}-{c.ci}to{c.co}-out{to}x{ho}x{wo}-pad{''.join(map(str, c.pad))}"


V3_CASES = [_c(1, 32, 32, 2, 1, 1, (0, 0, 0)), _c(1, 32, 32, 3, 8, 31, (0, 0, 0)), _c(1, 32, 32, 5, 9, 32, (1, 0, 0)),
            _c(1, 32, 32, 7, 9, 33, (0, 0, 0)), _c(1, 32, 32, 8, 8, 64, (2, 2, 2)), _c(1, 32, 32, 3, 9, 65, (2, 2, 2)),
            _c(2, 32, 32, 7, 8, 65, (1, 0, 0)), _c(3, 32, 32, 2, 1, 33, (1, 1, 1))]
V3_CHUNKS = {2: [2], 3: [3], 5: [3, 2], 7: [4, 3], 8: [2, 2, 2, 2]}      # at these batch sizes (few tiles)
V1_CASES = [_c(1, 1, 32, 1, 8, 61, (0, 0, 0)), _c(1, 3, 32, 2, 9, 62, (1, 1, 1)), _c(1, 11, 32, 3, 9, 63, (2, 2, 2)),
            _c(1, 16, 32, 2, 8, 124, (0, 1, 2)), _c(2, 11, 4, 3, 9, 125, (1, 0, 0)), _c(1, 16, 16, 3, 9, 63, (2, 1, 0)),
            _c(1, 32, 32, 1, 9, 125, (0, 0, 0)), _c(2, 32, 32, 1, 8, 62, (1, 2, 1))]
V1_GATED_CASES = [_c(1, 11, 32, 2, 9, 63, (1, 1, 1)), _c(1, 32, 32, 3, 9, 63, (0, 0, 0))]
# dgrad: the forward layer's case; dx has its INPUT extent (t, h, w)
DGRAD_CASES = [Case(1, 11, 32, 3, 9, 63, (0, 0, 0)), Case(1, 32, 32, 5, 9, 33, (1, 0, 0)), Case(2, 32, 32, 4, 10, 65, (1, 1, 1)),
               Case(1, 11, 32, 2, 9, 125, (2, 2, 2))]
WGRAD_CASES = [_c(1, 1, 32, 1, 8, 1, (0, 0, 0)), _c(2, 3, 32, 2, 9, 31, (1, 1, 1)), _c(1, 11, 32, 5, 8, 32, (2, 2, 2)),
               _c(1, 12, 32, 2, 16, 33, (0, 0, 0)), _c(2, 13, 32, 1, 17, 65, (0, 1, 2)), _c(1, 16, 32, 5, 9, 33, (1, 0, 0)),
               _c(3, 17, 32, 2, 9, 65, (0, 0, 0)), _c(1, 32, 32, 5, 17, 33, (1, 1, 1)), _c(2, 32, 32, 3, 16, 31, (2, 0, 1)),
               Case(130, 3, 32, 3, 11, 6, (0, 0, 0)), _c(129, 1, 32, 1, 8, 1, (0, 0, 0))]
# (sample, row block, time chunk) slabs and rows per block that wgrad_v2_grid is expected to form for WGRAD_CASES
WGRAD_SLABS = [(2, 4), (2 * 3 * 1, 3), (2 * 3, 4), (3, 6), (2 * 4, 5), (3 * 3, 3), (3 * 3, 3), (4 * 3, 5), (2 * 3 * 2, 6), (260, 5), (129, 8)]
FIRST_CASES = [_c(1, 1, 32, 2, 8, 62, (0, 0, 0)), _c(2, 11, 32, 3, 9, 63, (1, 2, 0)), _c(1, 16, 32, 3, 9, 62, (2, 1, 0)),
               _c(1, 11, 32, 1, 8, 63, (0, 1, 0)), _c(1, 11, 32, 2, 9, 126, (1, 0, 0)), _c(1, 16, 16, 2, 9, 63, (0, 0, 0))]
# the small cases of the mutation tests
REJECT_FWD = [V1_CASES[2], V1_CASES[5], V3_CASES[3], FIRST_CASES[1]]
REJECT_WGRAD = [WGRAD_CASES[1], WGRAD_CASES[5], WGRAD_CASES[6]]
LARGEST_N = WGRAD_CASES[6]      # 3 x 2 x 9 x 65 = 3510 voxels


def _with_regimes(cases):
    return [(c, r) for c in cases for r in REGIMES]


def _cid(cr):
    return f"{_id(cr[0])}-{cr[1]}"


# ---- inputs and the float64 reference --------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)      # nearest even


def _trunc16(t):
    """float32 -> the bf16 value below it in magnitude (the low 16 bits cleared)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _raw_inputs(c, regime):
    """x, w, bias, g in float32 BEFORE rounding (bias is handed to the kernels as float32 and is not rounded)."""
    to, ho, wo = _out(c)
    seed = sum(v * q for v, q in zip(tuple(c[:6]) + c.pad, (1000003, 100003, 10007, 1009, 101, 11, 5, 3, 2)))
    gen = torch.Generator().manual_seed(2 * seed + (regime == "relu_input"))
    x = torch.randn(c.b, c.ci, c.t, c.h, c.w, generator=gen)
    if regime == "relu_input":
        x = x.clamp_min(0)
    w = torch.randn(c.co, c.ci, 3, 3, 3, generator=gen) / (27 * c.ci) ** 0.5
    bias = 0.1 * torch.randn(c.co, generator=gen)
    g = torch.randn(c.b, c.co, to, ho, wo, generator=gen)
    return x, w, bias, g


def _unfold(x64, pad):
    """[b, c, t, h, w] -> the 27 shifted views [b, to, ho, wo, c, 27] of the zero-padded tensor, tap = 9 kt + 3 kh + kw."""
    xp = F.pad(x64, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    to, ho, wo = xp.shape[2] - 2, xp.shape[3] - 2, xp.shape[4] - 2
    views = [xp[:, :, kt:kt + to, kh:kh + ho, kw:kw + wo] for kt in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(views, dim=-1).permute(0, 2, 3, 4, 1, 5)


def _cl(t):
    """NCDHW -> NDHWC."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _fwd_ref(x, w, bias, pad):
    """(y64 before the ReLU, S), NDHWC, of float32 operands taken as they are."""
    y = F.conv3d(x.double(), w.double(), None if bias is None else bias.double(), padding=pad)
    s = F.conv3d(x.double().abs(), w.double().abs(), None if bias is None else bias.double().abs(), padding=pad)
    return _cl(y), _cl(s)


def _dgrad_ref(gg, w, pad):
    """(dx64, S), NDHWC, of an already gated g [b, co, to, ho, wo]."""
    dx = F.conv_transpose3d(gg.double(), w.double(), padding=pad)
    s = F.conv_transpose3d(gg.double().abs(), w.double().abs(), padding=pad)
    return _cl(dx), _cl(s)


def _wgrad_ref(x, gg, pad):
    """(dw64 [co, ci, 3, 3, 3], S, db64 [co], S) of an already gated g."""
    u, gl = _unfold(x.double(), pad), _cl(gg.double())
    dw = torch.einsum("bthwo,bthwcq->ocq", gl, u)
    s = torch.einsum("bthwo,bthwcq->ocq", gl.abs(), u.abs())
    shape = (gg.shape[1], x.shape[1], 3, 3, 3)
    return dw.reshape(shape), s.reshape(shape), gl.sum((0, 1, 2, 3)), gl.abs().sum((0, 1, 2, 3))


Problem = namedtuple("Problem", "x w bias g y64 sy gate gg dx64 sdx dw64 sdw db64 sdb")


@functools.lru_cache(maxsize=None)
def _problem(c, regime):
    """Rounded operands (float32 tensors holding bf16 values; bias float32) and every float64 reference of a case.  Shared by the
    tests that need it and never written to."""
    x, w, bias, g = _raw_inputs(c, regime)
    x, w, g = _bf16(x), _bf16(w), _bf16(g)
    y64, sy = _fwd_ref(x, w, bias, c.pad)
    gate = (y64 > 0).permute(0, 4, 1, 2, 3)      # NCDHW, like g
    gg = g * gate
    dx64, sdx = _dgrad_ref(gg, w, c.pad)
    dw64, sdw, db64, sdb = _wgrad_ref(x, gg, c.pad)
    return Problem(x, w, bias, g, y64, sy, gate, gg, dx64, sdx, dw64, sdw, db64, sdb)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def _ratio(got, ref64, s, c, bf16_out=False):
    """Worst error / bound over the elements (a non-finite result counts as infinite)."""
    got = got.detach().double().cpu()
    bound = (c * (1 + U16) * U32 * s + U16 * ref64.abs() if bf16_out else c * U32 * s) + 1e-30
    ratio = (got - ref64).abs() / bound
    return float(torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).max())


def _check(family, got, ref64, s, c, what, bf16_out=False):
    """|got - ref64| <= c 2^-24 S for an f32 result, c (1 + 2^-8) 2^-24 S + 2^-8 |ref64| for a bf16 one, per element; prints the
    worst error / bound."""
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    worst = _ratio(got, ref64, s, c, bf16_out)
    print(f"[{family}] {what}: error / bound {worst:.3f}")
    absref = (1 + U16) * s + (U16 / (c * U32)) * ref64.abs() if bf16_out else s          # tol * absref == the bound above
    _within(got.detach().float(), ref64, absref, tol=c * U32, what=f"{family} {what}")
    return worst


def _rejected(got, ref64, s, c, what, bf16_out=False):
    with pytest.raises(AssertionError, match="x the bound"):
        _check("cpu", got, ref64, s, c, what, bf16_out)


def _old_y_check(got, ref32):
    """tests/test_gpu_conv.py's check of y and dx: assert_close(rtol=1e-2, atol=2e-3) against float32 torch."""
    return bool(((got.double() - ref32.double()).abs() <= 2e-3 + 1e-2 * ref32.double().abs()).all())


def _old_norm_check(got, ref32):
    """tests/test_gpu_conv.py's check of dW and db: max |got - ref| <= 2e-3 max |ref| + 1e-4 against float32 torch."""
    return float((got.double() - ref32.double()).abs().max()) <= 2e-3 * float(ref32.abs().max()) + 1e-4


# ---- CPU emulation of the kernels' documented arithmetic -------------------------------------------------------------------
def _emulate_conv(x, w, bias, pad, kstep, taps=range(27), skip=None):
    """The marching kernels as their sources state them: one f32 accumulator per output, initialised with the bias, updated once
    per matrix-instruction k-step (exact bf16 products, summed here in float64 and rounded once into the accumulator): kstep = 16
    channels of a tap (conv3d_fwd_bf16_kernel, conv3d_first_f32in_kernel) or 32 (v3) in the order kt, kw, channel half, kh.
    skip = (tap, column): that tap adds nothing at that output column (a mutation).  -> float32 NDHWC before ReLU / rounding."""
    co, ci = w.shape[:2]
    u = _unfold(x.double(), pad)
    w64 = w.double().reshape(co, ci, 27)
    acc = (torch.zeros(co) if bias is None else bias.float()).expand(*u.shape[:4], co).contiguous()
    for kt in range(3):
        for kw in range(3):
            for k0 in range(0, ci, kstep):
                for kh in range(3):
                    tap = 9 * kt + 3 * kh + kw
                    if tap not in taps:
                        continue
                    term = torch.einsum("bthwc,oc->bthwo", u[..., k0:k0 + kstep, tap], w64[:, k0:k0 + kstep, tap])
                    if skip is not None and skip[0] == tap:
                        term[:, :, :, skip[1]] = 0
                    acc = (acc.double() + term).float()
    return acc


def _flip(w):
    """The dgrad operator's weights, W'[ci, co, tap] = W[co, ci, 26 - tap] (conv3d_pack_weight_bf16(transpose_flip=True))."""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def _emulate_dgrad(gg, w, pad, kstep):
    return _emulate_conv(gg, _flip(w), None, tuple(2 - p for p in pad), kstep)


def _store_bf16(acc, relu):
    """The epilogue: ReLU, one rounding to bf16."""
    return _bf16(acc.clamp_min(0) if relu else acc)


def _wgrad_grid(b, to, ho, wo):
    """wgrad_v2_grid of conv3d_wgrad_bf16_v2.hip: (row blocks, column tiles, time chunks, slices per chunk, rows per block)."""
    nrb = (ho + 7) // 8
    if b * nrb < 256 and b * (nrb + 1) <= 256 and (ho + nrb) // (nrb + 1) < (ho + nrb - 1) // nrb:
        nrb += 1
    rpb = (ho + nrb - 1) // nrb
    tiles, best, ntc = b * nrb, -1, 1
    for k in range(1, max((to + 1) // 2, 1) + 1):
        if tiles * k > 16 * 256:
            break
        tch = (to + k - 1) // k
        nch = (to + tch - 1) // tch
        cost = ((tiles * nch + 255) // 256) * (tch + 2)
        if best < 0 or cost < best:
            best, ntc = cost, nch
    tch = (to + ntc - 1) // ntc
    return nrb, (wo + 31) // 32, (to + tch - 1) // tch, tch, rpb


def _v3_chunks(b, to, ho, wo):
    """v3_grid of conv3d_bf16_v3.hip: the output slices per time chunk, or None when the launch falls to v1."""
    if to < 2:
        return None
    tiles, best, n = b * ((ho + 7) // 8) * ((wo + 31) // 32), -1, 1
    for k in range(1, max(to // 2, 1) + 1):
        if tiles * k > 8 * 512:
            break
        tch = (to + k - 1) // k
        nch = (to + tch - 1) // tch
        cost = ((tiles * nch + 511) // 512) * (2 * tch + 3)
        if best < 0 or cost < best:
            best, n = cost, nch
    tch = (to + n - 1) // n
    n = (to + tch - 1) // tch
    if to - (n - 1) * tch < 2:
        tch += 1
        n = (to + tch - 1) // tch
        if to - (n - 1) * tch < 2:
            return None
    return [min(tch, to - i * tch) for i in range(n)]


def _emulate_wgrad_slabs(x, gg, pad):
    """conv3d_wgrad_bf16_v2_kernel: -> (dW slabs [n_slabs, co, ci, 27], db slabs [n_slabs, co]) in float32, slab index = (sample x
    time chunks + chunk) x row blocks + row block.  A slab is an f32 accumulator that starts at zero and is updated once per
    16 voxels (exact products, summed in float64 and rounded once): column tiles of 32, inside a tile the chunk's slices, inside
    a slice its rows, inside a row two groups of 16 columns.  (The samples' slabs have one structure and are walked together.)"""
    b, co = gg.shape[:2]
    ci = x.shape[1]
    u, gl = _unfold(x.double(), pad), _cl(gg.double())
    to, ho, wo = u.shape[1:4]
    nrb, ncb, ntc, tch, rpb = _wgrad_grid(b, to, ho, wo)
    dw = torch.zeros(b, ntc, nrb, co, ci, 27)
    db = torch.zeros(b, ntc, nrb, co)
    for tc in range(ntc):
        for rb in range(nrb):
            acc, accb = torch.zeros(b, co, ci, 27), torch.zeros(b, co)
            for cb in range(ncb):
                for t in range(tc * tch, min((tc + 1) * tch, to)):
                    for row in range(rb * rpb, min((rb + 1) * rpb, ho)):
                        for c0 in range(32 * cb, min(32 * cb + 32, wo), 16):
                            gs, us = gl[:, t, row, c0:c0 + 16], u[:, t, row, c0:c0 + 16]
                            acc = (acc.double() + torch.einsum("bno,bncq->bocq", gs, us)).float()
                            accb = (accb.double() + gs.sum(1)).float()
            dw[:, tc, rb], db[:, tc, rb] = acc, accb
    return dw.reshape(-1, co, ci, 27), db.reshape(-1, co)


def _reduce_slabs(slabs):
    """conv3d_wgrad_reduce_kernel: group g of 16 adds slabs g, g + 16, ... in that order into four alternating partial sums,
    its sum is (s0 + s1) + (s2 + s3); the 16 group sums go through a pairwise tree.  All in float32."""
    parts = []
    for g in range(16):
        s = [torch.zeros_like(slabs[0]) for _ in range(4)]
        for j, slab in enumerate(slabs[g::16]):
            s[j % 4] = s[j % 4] + slab
        parts.append((s[0] + s[1]) + (s[2] + s[3]))
    while len(parts) > 1:
        parts = [parts[2 * q] + parts[2 * q + 1] for q in range(len(parts) // 2)]
    return parts[0]


def _emulate_wgrad(x, gg, pad, drop_slab=None):
    dws, dbs = _emulate_wgrad_slabs(x, gg, pad)
    if drop_slab is not None:
        keep = [i for i in range(len(dws)) if i != drop_slab]
        dws, dbs = dws[keep], dbs[keep]
    return _reduce_slabs(list(dws)).reshape(gg.shape[1], x.shape[1], 3, 3, 3), _reduce_slabs(list(dbs))


def _torch32(p, c, relu=True):
    """(a) of the module docstring: float32 torch on the rounded operands -> y, dx, dw (autograd), db (a float32 sum), NDHWC."""
    x, w, bias = p.x.clone().requires_grad_(True), p.w.clone().requires_grad_(True), p.bias.clone()
    y = F.conv3d(x, w, bias, padding=c.pad)
    y.backward(p.gg)
    return _cl((y.clamp_min(0) if relu else y).detach()), _cl(x.grad), w.grad, p.gg.sum((0, 2, 3, 4))


def _db_voxel_after_voxel(gg):
    """A plain float32 sum of g, one voxel after the other in memory order (numpy's cumsum adds sequentially)."""
    rows = _cl(gg).reshape(-1, gg.shape[1]).numpy()
    return torch.from_numpy(np.cumsum(rows, axis=0, dtype=np.float32)[-1].copy())


@functools.lru_cache(maxsize=None)
def _emu_fwd(c, regime, kstep):
    p = _problem(c, regime)
    return _emulate_conv(p.x, p.w, p.bias, c.pad, kstep)


@functools.lru_cache(maxsize=None)
def _emu_bwd(c, regime):
    """-> (dx with 16 channels a step, dx with 32, dW, db) of the emulations."""
    p = _problem(c, regime)
    return (_emulate_dgrad(p.gg, p.w, c.pad, 16), _emulate_dgrad(p.gg, p.w, c.pad, 32)) + _emulate_wgrad(p.x, p.gg, c.pad)


def _kstep(c, gated=False):
    """Channels per k-step of the kernel that serves the FORWARD of a case through conv3d_fwd_bf16."""
    to, ho, wo = _out(c)
    return 32 if c.ci > 16 and not gated and _v3_chunks(c.b, to, ho, wo) else 16


# ---- the table of the module docstring ---------------------------------------------------------------------------------------
FWD_TABLE = V3_CASES + V1_CASES + V1_GATED_CASES + FIRST_CASES
BWD_TABLE = DGRAD_CASES + WGRAD_CASES


@functools.lru_cache(maxsize=None)
def _table_row(c, regime, backward):
    """Worst err / (2^-24 S) of float32 torch and of the emulation: {"y": (a, b)} for a forward case, {"y" (dx), "dw", "db"} for
    a backward one."""
    p = _problem(c, regime)
    y32, dx32, dw32, db32 = _torch32(p, c, relu=False)
    if not backward:
        emu = max(_ratio(_emu_fwd(c, regime, k), p.y64, p.sy, 1.0) for k in (16, 32) if k == 16 or c.ci > 16)
        return {"y": (_ratio(y32, p.y64, p.sy, 1.0), emu)}
    dx16, dx32e, dw, db = _emu_bwd(c, regime)
    emu = max(_ratio(dx16, p.dx64, p.sdx, 1.0), _ratio(dx32e, p.dx64, p.sdx, 1.0))
    db_a = max(_ratio(db32, p.db64, p.sdb, 1.0), _ratio(_db_voxel_after_voxel(p.gg), p.db64, p.sdb, 1.0))
    return {"y": (_ratio(dx32, p.dx64, p.sdx, 1.0), emu), "dw": (_ratio(dw32, p.dw64, p.sdw, 1.0), _ratio(dw, p.dw64, p.sdw, 1.0)),
            "db": (db_a, _ratio(db, p.db64, p.sdb, 1.0))}


def _measure(verbose=True):
    """-> {kind: {regime: 4 x the worst ratio}}; prints the table."""
    worst = {k: {r: [0.0, 0.0] for r in REGIMES} for k in C}
    for cases, backward in ((FWD_TABLE, False), (BWD_TABLE, True)):
        for c in cases:
            for regime in REGIMES:
                for kind, (a, b) in _table_row(c, regime, backward).items():
                    w = worst[kind][regime]
                    w[0], w[1] = max(w[0], a), max(w[1], b)
                    if verbose:
                        name = {"y": "dx" if backward else "y"}.get(kind, kind)
                        print(f"    {_id(c):<38} {regime:<10} {name:<2}  float32 torch {a:6.2f}   emulation {b:6.2f}")
    consts = {k: {r: round(4 * max(worst[k][r]), 1) for r in REGIMES} for k in C}
    if verbose:
        for k in C:
            for r in REGIMES:
                print(f"worst {k:<2} {r:<10}: float32 torch {worst[k][r][0]:.2f}, emulation {worst[k][r][1]:.2f} -> C = {consts[k][r]}")
    return consts


# ---- CPU: the constants, the reference, the grid rules ---------------------------------------------------------------------
def test_the_table_reproduces_the_constants():
    assert _measure(verbose=False) == C


@pytest.mark.parametrize("cr", _with_regimes(FWD_TABLE), ids=_cid)
def test_checker_accepts_float32_torch_and_the_emulation_forward(cr):
    c, regime = cr
    p = _problem(c, regime)
    for relu in (False, True):
        ref = p.y64.clamp_min(0) if relu else p.y64
        y32 = _torch32(p, c, relu)[0]
        _check("cpu", y32, ref, p.sy, C["y"][regime], f"float32 torch y {_cid(cr)} relu {relu}")
        _check("cpu", _bf16(y32), ref, p.sy, C["y"][regime], f"float32 torch y, bf16 store {_cid(cr)} relu {relu}", bf16_out=True)
        for k in (16, 32) if c.ci > 16 else (16,):
            emu = _emu_fwd(c, regime, k)
            _check("cpu", _store_bf16(emu, relu), ref, p.sy, C["y"][regime], f"emulation, {k} channels a step {_cid(cr)} relu {relu}", bf16_out=True)


@pytest.mark.parametrize("cr", _with_regimes(BWD_TABLE), ids=_cid)
def test_checker_accepts_float32_torch_and_the_emulation_backward(cr):
    c, regime = cr
    p = _problem(c, regime)
    _, dx32, dw32, db32 = _torch32(p, c)
    _check("cpu", _bf16(dx32), p.dx64, p.sdx, C["y"][regime], f"float32 torch dx {_cid(cr)}", bf16_out=True)
    _check("cpu", dw32, p.dw64, p.sdw, C["dw"][regime], f"float32 torch dw {_cid(cr)}")
    _check("cpu", db32, p.db64, p.sdb, C["db"][regime], f"float32 torch db {_cid(cr)}")
    _check("cpu", _db_voxel_after_voxel(p.gg), p.db64, p.sdb, C["db"][regime], f"float32 db, voxel after voxel {_cid(cr)}")
    dx16, dx32e, dw, db = _emu_bwd(c, regime)
    for k, dx in ((16, dx16), (32, dx32e)):
        _check("cpu", _bf16(dx), p.dx64, p.sdx, C["y"][regime], f"dgrad emulation {k} {_cid(cr)}", bf16_out=True)
    _check("cpu", dw, p.dw64, p.sdw, C["dw"][regime], f"wgrad emulation {_cid(cr)}")
    _check("cpu", db, p.db64, p.sdb, C["db"][regime], f"db emulation {_cid(cr)}")


def test_the_einsum_weight_gradient_is_torchs_in_float64():
    """`_wgrad_ref` (27 shifted views, one einsum) against torch.nn.grad.conv3d_weight and conv3d's own autograd, and
    `_dgrad_ref` / the flipped-weight forward form of `_emulate_dgrad` against autograd, all in float64."""
    for c in (WGRAD_CASES[1], WGRAD_CASES[4], DGRAD_CASES[2]):
        p = _problem(c, "zero_mean")
        x, w = p.x.double().requires_grad_(True), p.w.double().requires_grad_(True)
        F.conv3d(x, w, p.bias.double(), padding=c.pad).backward(p.gg.double())
        tiny = 1e-12 * float(p.sdw.max())
        assert float((w.grad - p.dw64).abs().max()) <= tiny
        assert float((torch.nn.grad.conv3d_weight(p.x.double(), p.w.shape, p.gg.double(), padding=c.pad) - p.dw64).abs().max()) <= tiny
        assert float((_cl(x.grad) - p.dx64).abs().max()) <= 1e-12 * float(p.sdx.max())
        flipped = _fwd_ref(p.gg, _flip(p.w), None, tuple(2 - q for q in c.pad))[0]
        assert float((flipped - p.dx64).abs().max()) <= 1e-12 * float(p.sdx.max())


def test_the_cases_sit_on_the_paths_they_name():
    """The grid rules restated from the sources put the cases where the module docstring says."""
    for c in V3_CASES:
        to, ho, wo = _out(c)
        assert _v3_chunks(c.b, to, ho, wo) == V3_CHUNKS[to], (_id(c), _v3_chunks(c.b, to, ho, wo))
    assert {_out(c)[2] for c in V3_CASES} >= {1, 31, 32, 33, 64, 65} and {_out(c)[1] for c in V3_CASES} >= {1, 8, 9}
    for c in V1_CASES:
        to, ho, wo = _out(c)
        assert c.ci <= 16 or _v3_chunks(c.b, to, ho, wo) is None, _id(c)
    assert {_out(c)[2] for c in V1_CASES} >= {61, 62, 63, 124, 125}
    for axis in range(3):
        assert {c.pad[axis] for c in V1_CASES} == {0, 1, 2} and {c.pad[axis] for c in WGRAD_CASES} == {0, 1, 2}
    for c in DGRAD_CASES:      # dgrad without a gate is v3's: its output extent is the layer's input extent
        assert _v3_chunks(c.b, c.t, c.h, c.w) is not None, _id(c)
    for c, (slabs, rpb) in zip(WGRAD_CASES, WGRAD_SLABS):
        nrb, ncb, ntc, tch, rows = _wgrad_grid(c.b, *_out(c))
        assert (c.b * nrb * ntc, rows) == (slabs, rpb), (_id(c), nrb, ntc, rows)
    assert _wgrad_grid(1, 5, 9, 33)[2:4] == (3, 2)      # to = 5 at batch 1: chunks 2 + 2 + 1
    assert _wgrad_grid(32, 14, 16, 16)[0] == 3           # 16 rows at batch 32: three blocks
    for c in FIRST_CASES:
        assert c.pad[2] == 0 and c.ci <= 16
    assert {c.w % 4 == 0 for c in FIRST_CASES} == {True, False}


# ---- CPU: the checker rejects what it must ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cr", _with_regimes(REJECT_FWD), ids=_cid)
def test_checker_rejects_subtly_wrong_forward_results(cr):
    c, regime = cr
    p = _problem(c, regime)
    k = _kstep(c)
    cy = C["y"][regime]
    to, ho, wo = _out(c)
    ref = p.y64.clamp_min(0)
    y32 = _torch32(p, c)[0]
    good = _emulate_conv(p.x, p.w, p.bias, c.pad, k)
    _check("cpu", _store_bf16(good, True), ref, p.sy, cy, "the emulation as it is", bf16_out=True)
    assert _old_y_check(_store_bf16(good, True), y32)
    tile = 32 if k == 32 else 62
    assert wo % tile, "the last tile is expected to be ragged"
    for tap in (0, 12, 24):      # kw = 0: with padding 2 the last column's other taps read padding only
        _rejected(_store_bf16(_emulate_conv(p.x, p.w, p.bias, c.pad, k, skip=(tap, wo - 1)), True), ref, p.sy, cy,
                  f"tap {tap} dropped at the last valid column", bf16_out=True)
    _rejected(_store_bf16(good + p.bias, True), ref, p.sy, cy, "bias added twice", bf16_out=True)
    _rejected(_store_bf16(good - p.bias, True), ref, p.sy, cy, "bias not added", bf16_out=True)
    truncated = _trunc16(good.clamp_min(0))
    _rejected(truncated, ref, p.sy, cy, "output truncated to bf16 instead of rounded", bf16_out=True)
    assert _old_y_check(truncated, y32), "the rtol 1e-2 / atol 2e-3 check is expected to let a truncated output through"
    xr, wr, _, _ = _raw_inputs(c, regime)
    t_ops = _store_bf16(_emulate_conv(_trunc16(xr), _trunc16(wr), p.bias, c.pad, k), True)
    _rejected(t_ops, ref, p.sy, cy, "operands truncated instead of rounded", bf16_out=True)


@pytest.mark.parametrize("regime", REGIMES)
def test_checker_rejects_a_leak_through_a_padded_input_channel(regime):
    """c_in = 11 in an image of 16 channels: channel 11 of the image holds 2^-9 at every voxel instead of zero and meets a weight
    fragment whose row 11 is a copy of row 0 instead of zeros: y moves by 2^-9 sum_taps w[:, 0] -- below 2e-3."""
    c = V1_CASES[2]
    p = _problem(c, regime)
    y32 = _torch32(p, c)[0]
    x16 = torch.cat([p.x, torch.full_like(p.x[:, :1], 2.0 ** -9)], dim=1)
    w16 = torch.cat([p.w, p.w[:, :1]], dim=1)
    leak = _store_bf16(_emulate_conv(x16, w16, p.bias, c.pad, 16), True)
    assert float((leak - _store_bf16(_emulate_conv(p.x, p.w, p.bias, c.pad, 16), True)).abs().max()) > 0
    _rejected(leak, p.y64.clamp_min(0), p.sy, C["y"][regime], "a padded input channel leaks", bf16_out=True)
    assert _old_y_check(leak, y32), "the rtol 1e-2 / atol 2e-3 check is expected to let the leak through"


@pytest.mark.parametrize("regime", REGIMES)
def test_checker_rejects_dgrad_gated_on_y_greater_or_equal_zero(regime):
    """Exact zeros in y: x zero over the first 3 x 3 x 3 voxels and a zero bias in channel 0 give y64[0, 0, 0, 0, 0] == 0 exactly."""
    c = DGRAD_CASES[0]
    x, w, bias, g = (t.clone() for t in _problem(c, regime)[:4])
    x[:, :, :3, :3, :3] = 0
    bias[0] = 0
    y64, _ = _fwd_ref(x, w, bias, c.pad)
    assert float(y64[0, 0, 0, 0, 0]) == 0.0 and float(g[0, 0, 0, 0, 0]) != 0.0
    ncdhw = y64.permute(0, 4, 1, 2, 3)
    dx64, sdx = _dgrad_ref(g * (ncdhw > 0), w, c.pad)
    _check("cpu", _bf16(_emulate_dgrad(g * (ncdhw > 0), w, c.pad, 16)), dx64, sdx, C["y"][regime], "gated on y > 0", bf16_out=True)
    _rejected(_bf16(_emulate_dgrad(g * (ncdhw >= 0), w, c.pad, 16)), dx64, sdx, C["y"][regime], "gated on y >= 0", bf16_out=True)


@pytest.mark.parametrize("cr", _with_regimes(REJECT_WGRAD), ids=_cid)
def test_checker_rejects_subtly_wrong_weight_gradients(cr):
    c, regime = cr
    p = _problem(c, regime)
    cw, cb = C["dw"][regime], C["db"][regime]
    to, ho, wo = _out(c)
    n_slabs = c.b * _wgrad_grid(c.b, to, ho, wo)[0] * _wgrad_grid(c.b, to, ho, wo)[2]
    dw, db = _emulate_wgrad(p.x, p.gg, c.pad)
    _check("cpu", dw, p.dw64, p.sdw, cw, "the emulation as it is")
    _check("cpu", db, p.db64, p.sdb, cb, "the emulation as it is (db)")

    def without(mask):      # float64 result without the voxels of `mask` [b, to, ho, wo], rounded to f32
        gm = p.gg * (~mask).unsqueeze(1)
        dw64, _, db64, _ = _wgrad_ref(p.x, gm, c.pad)
        return dw64.float(), db64.float()

    m = torch.zeros(c.b, to, ho, wo, dtype=torch.bool)
    last_col, last_t, slab = m.clone(), m.clone(), m.clone()
    last_col[..., wo - 1] = True
    last_t[:, to - 1] = True
    rpb = _wgrad_grid(c.b, to, ho, wo)[4]
    slab[c.b - 1, :_wgrad_grid(c.b, to, ho, wo)[3], :rpb] = True      # the first chunk's first row block of the last sample
    _rejected(without(last_col)[0], p.dw64, p.sdw, cw, "dW without its last output column")
    _rejected(without(last_t)[0], p.dw64, p.sdw, cw, "dW without its last time slice")
    _rejected(without(slab)[0], p.dw64, p.sdw, cw, "dW without one slab")
    _rejected(_emulate_wgrad(p.x, p.gg, c.pad, drop_slab=n_slabs - 1)[0], p.dw64, p.sdw, cw, "the reduce without its last slab")
    _rejected(_emulate_wgrad(p.x, p.gg, c.pad, drop_slab=n_slabs - 1)[1], p.db64, p.sdb, cb, "the reduce without its last slab (db)")
    _rejected(_cl(p.g.double()).sum((0, 1, 2, 3)).float(), p.db64, p.sdb, cb, "db from the ungated g")


@pytest.mark.parametrize("regime", REGIMES)
def test_checker_rejects_one_missing_voxel_at_the_largest_n(regime):
    """One voxel of 3 510 missing from dW and db: the voxel whose largest |g| is the smallest.  (tests/test_gpu_conv.py's 2e-3
    max |ref| + 1e-4 still sees it at this N -- one voxel's |x g| ~ 1 against 2e-3 max |dW| ~ 0.1: that check loses a voxel
    only at sizes far beyond any test here.)"""
    c = LARGEST_N
    p = _problem(c, regime)
    to, ho, wo = _out(c)
    gl = _cl(p.gg).abs().amax(-1)
    gl[gl == 0] = float("inf")
    idx = int(gl.argmin())
    m = torch.zeros(c.b * to * ho * wo, dtype=torch.bool)
    m[idx] = True
    gm = p.gg * (~m.view(c.b, 1, to, ho, wo))
    assert int((gm != p.gg).sum()) > 0
    dw64, _, db64, _ = _wgrad_ref(p.x, gm, c.pad)
    _rejected(dw64.float(), p.dw64, p.sdw, C["dw"][regime], "dW without one voxel")
    _rejected(db64.float(), p.db64, p.sdb, C["db"][regime], "db without one voxel")


# ---- the packers' special values ---------------------------------------------------------------------------------------------
def _special_f32():
    """float32 values that tell round-to-nearest-even from truncation and from round-half-up, by their bits: exactly halfway with
    an even and an odd last kept bit, halfway +- one float32 ulp, +-0, the largest finite bf16 and float32, the smallest normal."""
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00000000, 0x7F7F0000, 0x7F7FFFFF, 0x00800000,
           0x00808000, 0x00818000, 0x3F800000, 0x40490FDB]
    bits = pos + [b | 0x80000000 for b in pos]
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


def _half_up16(t):
    """float32 -> bf16 by adding half a step to the magnitude and truncating."""
    return ((t.contiguous().view(torch.int32) + 0x8000) & -65536).view(torch.float32)


def test_the_special_values_tell_the_rounding_modes_apart():
    v = _special_f32()
    rne = v.to(torch.bfloat16).to(torch.float32)
    assert not torch.equal(rne.view(torch.int32), _trunc16(v).view(torch.int32))
    finite = torch.isfinite(rne)
    assert not torch.equal(rne[finite].view(torch.int32), _half_up16(v)[finite].view(torch.int32))
    assert float(rne[0]) == 1.0 and float(rne[1]) == 1.015625 and float(rne[2]) == 1.0 and float(rne[3]) == 1.0078125
    assert rne[6].view(torch.int32).item() == 0 and rne[len(v) // 2 + 6].view(torch.int32).item() == -(1 << 31)      # +0, -0


def _with_specials(x):
    """x with the special values scattered over it (every channel, first and last voxels included)."""
    v = _special_f32()
    flat = x.clone().reshape(x.shape[0], x.shape[1], -1)
    n = flat.shape[-1]
    for i in range(len(v)):
        flat[i % x.shape[0], (3 * i) % x.shape[1], (7 * i) % n] = v[i]
    flat[:, :, 0], flat[:, :, -1] = v[1], v[len(v) // 2 + 3]
    return flat.reshape(x.shape)


# ---- GPU helpers -----------------------------------------------------------------------------------------------------------
def _ndhwc16(x, device):
    """Float32 NCDHW holding bf16 values -> the NDHWC bf16 image with its channels padded to 16 or 32 with zeros (built with
    torch, so the convolution tests do not lean on the pack kernel)."""
    b, ch, t, h, w = x.shape
    img = torch.zeros(b, t, h, w, 16 if ch <= 16 else 32, dtype=torch.bfloat16)
    img[..., :ch] = x.permute(0, 2, 3, 4, 1).to(torch.bfloat16)
    return img.to(device)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _check_y(family, y, c_out, ref, s, cy, what):
    """A bf16 NDHWC result of 32 stored channels: the first c_out within the bound, the others exactly zero."""
    y = y.cpu()
    assert y.dtype == torch.bfloat16 and y.shape[-1] == 32
    assert int(torch.count_nonzero(y[..., c_out:])) == 0, f"{family} {what}: a padded output channel is not zero"
    return _check(family, y[..., :c_out].float(), ref, s, cy, what, bf16_out=True)


def _fwd_both_layouts(K, family, xp, gate, wp, bias, c, ref64, s, cy, what, device):
    for relu in (True, False):
        ref = ref64.clamp_min(0) if relu else ref64
        y = K.conv3d_fwd_bf16(xp, gate, wp, bias, c.ci, c.co, c.pad, relu=relu, y_ncdhw=False)
        _check_y(family, y, c.co, ref, s, cy, f"{what} relu {relu}")
        yn = K.conv3d_fwd_bf16(xp, gate, wp, bias, c.ci, c.co, c.pad, relu=relu, y_ncdhw=True)
        assert yn.dtype == torch.bfloat16
        _check(family + " NCDHW", _cl(yn.cpu().float()), ref, s, cy, f"{what} relu {relu}", bf16_out=True)


# ---- GPU 1: the input-stationary kernel ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cr", _with_regimes(V3_CASES), ids=_cid)
def test_v3_forward(cr, device):
    """conv3d_fwd_bf16_v3_kernel<false, Y_NCDHW>: every step kind of the march, its time chunks, ragged rows and columns."""
    K = _ops()
    c, regime = cr
    p = _problem(c, regime)
    wp = K.conv3d_pack_weight_bf16(p.w.to(device))
    _fwd_both_layouts(K, "v3", _ndhwc16(p.x, device), None, wp, p.bias.to(device), c, p.y64, p.sy, C["y"][regime], _cid(cr), device)


# ---- GPU 2: the v1 marching kernel ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cr", _with_regimes(V1_CASES), ids=_cid)
def test_v1_forward(cr, device):
    """conv3d_fwd_bf16_kernel<16 / 32, false, Y_NCDHW, false>: 16 padded input channels, fewer than 32 output channels, and
    32 -> 32 with a single output slice."""
    K = _ops()
    c, regime = cr
    p = _problem(c, regime)
    wp = K.conv3d_pack_weight_bf16(p.w.to(device))
    _fwd_both_layouts(K, "v1", _ndhwc16(p.x, device), None, wp, p.bias.to(device), c, p.y64, p.sy, C["y"][regime], _cid(cr), device)


def _gate_image(shape, seed):
    """A bf16 NCDHW gate with positives, negatives, +0 and -0."""
    gen = torch.Generator().manual_seed(seed)
    gate = torch.randn(shape, generator=gen)
    kind = torch.randint(0, 4, shape, generator=gen)
    gate[kind == 0] = 0.0
    gate[kind == 1] = -0.0
    return gate.to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("cr", _with_regimes(V1_GATED_CASES), ids=_cid)
def test_v1_forward_with_a_gate(cr, device):
    """conv3d_fwd_bf16_kernel<16 / 32, true, ...>: x is taken only where the gate image is > 0 (+0, -0 and negatives close it)."""
    K = _ops()
    c, regime = cr
    p = _problem(c, regime)
    gate = _gate_image(p.x.shape, c.ci)
    xg = p.x * (gate.float() > 0)
    y64, sy = _fwd_ref(xg, p.w, p.bias, c.pad)
    assert 0.2 < float((gate.float() > 0).float().mean()) < 0.5
    wp = K.conv3d_pack_weight_bf16(p.w.to(device))
    _fwd_both_layouts(K, "v1 gated", _ndhwc16(p.x, device), _ndhwc16(gate.float(), device), wp, p.bias.to(device), c, y64, sy,
                      C["y"][regime], _cid(cr), device)


# ---- GPU 3: dgrad ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cr", _with_regimes(DGRAD_CASES), ids=_cid)
def test_dgrad(cr, device):
    """The forward entry point on transpose_flip weights with padding 2 - p: the gate as a bf16 image of the reference's own
    y64 > 0 pattern (v1, HAS_GATE), and g gated beforehand with no gate (v3)."""
    K = _ops()
    c, regime = cr
    p = _problem(c, regime)
    wpt = K.conv3d_pack_weight_bf16(p.w.to(device), transpose_flip=True)
    pad_b = tuple(2 - q for q in c.pad)
    gate = _ndhwc16(p.gate.float(), device)
    assert 0.05 < float(p.gate.float().mean()) < 0.95
    dx = K.conv3d_fwd_bf16(_ndhwc16(p.g, device), gate, wpt, None, c.co, c.ci, pad_b, relu=False)
    _check_y("dgrad v1 gated", dx, c.ci, p.dx64, p.sdx, C["y"][regime], _cid(cr))
    dx = K.conv3d_fwd_bf16(_ndhwc16(p.gg, device), None, wpt, None, c.co, c.ci, pad_b, relu=False)
    _check_y("dgrad v3", dx, c.ci, p.dx64, p.sdx, C["y"][regime], _cid(cr))


# ---- GPU 4: weight gradient and db -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cr", _with_regimes(list(zip(WGRAD_CASES, WGRAD_SLABS))), ids=lambda cr: _cid((cr[0][0], cr[1])))
def test_weight_gradient(cr, device):
    """conv3d_wgrad_bf16_v2_kernel<16 / 16 PACK12 / 32> + conv3d_wgrad_reduce_kernel, g gated outside and a gate handed over."""
    K = _ops()
    (c, (slabs, _)), regime = cr
    p = _problem(c, regime)
    to, ho, wo = _out(c)
    d, need = K.conv_dims(c.b, c.ci, c.co, c.t, c.h, c.w, c.pad), ctypes.c_size_t(0)
    K.check(K.get_lib().pv_conv3d_bwd_weight_bf16_workspace_bytes(ctypes.byref(d), ctypes.byref(need)), "wgrad workspace")
    assert need.value - c.b * to * ho * wo * 32 * 2 == slabs * 28 * 32 * 32 * 4, "the case left the path its slab count names"
    xp = _ndhwc16(p.x, device)
    what = _cid((c, regime))
    dw, db = K.conv3d_bwd_weight_bf16(xp, _ndhwc16(p.gg, device), None, c.ci, c.co, c.pad)
    _check("wgrad", dw, p.dw64, p.sdw, C["dw"][regime], f"dW {what} gated outside")
    _check("db", db, p.db64, p.sdb, C["db"][regime], f"db {what} gated outside")
    dw2, db2 = K.conv3d_bwd_weight_bf16(xp, _ndhwc16(p.g, device), _ndhwc16(p.gate.float(), device), c.ci, c.co, c.pad)
    _check("wgrad", dw2, p.dw64, p.sdw, C["dw"][regime], f"dW {what} gate handed over")
    _check("db", db2, p.db64, p.sdb, C["db"][regime], f"db {what} gate handed over")


# ---- GPU 5: the first layer from the f32 NCDHW input ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cr", _with_regimes(FIRST_CASES), ids=_cid)
def test_first_layer_from_f32(cr, device):
    """conv3d_first_f32in_kernel (w % 4 == 0) and conv3d_fwd_bf16_kernel<16, ..., X_F32> (otherwise) on the UNROUNDED x: y against
    float64 of the rounded x, the NDHWC image it leaves bit for bit x.to(bfloat16) with zero padded channels."""
    K = _ops()
    c, regime = cr
    p = _problem(c, regime)
    x_raw = _raw_inputs(c, regime)[0]
    assert not torch.equal(x_raw, p.x)
    wp = K.conv3d_pack_weight_bf16(p.w.to(device))
    for relu in (True, False):
        y, xp = K.conv3d_fwd_bf16_f32in(x_raw.to(device), wp, p.bias.to(device), c.co, c.pad, relu=relu)
        _check_y("first" if c.w % 4 == 0 else "first (v1 form)", y, c.co, p.y64.clamp_min(0) if relu else p.y64, p.sy, C["y"][regime],
                 f"{_cid(cr)} relu {relu}")
        assert torch.equal(_bits16(xp.cpu()), _bits16(_ndhwc16(p.x, "cpu"))), "the NDHWC image is not x rounded to nearest even"


# ---- GPU 6: the packers ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 11, 2, 3, 6), (2, 11, 3, 3, 5), (1, 32, 2, 2, 5), (3, 17, 1, 7, 3), (2, 1, 1, 5, 5)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pack_rounds_to_nearest_even(shape, device):
    """pack_ncdhw_to_ndhwc_v4_kernel (t h w % 4 == 0) and pack_ncdhw_to_ndhwc_kernel, CPAD 16 and 32, bit for bit x.to(bfloat16)."""
    K = _ops()
    x = _with_specials(torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))))
    got = K.pack_ncdhw_f32_to_ndhwc_bf16(x.to(device)).cpu()
    ref = torch.zeros(got.shape, dtype=torch.bfloat16)
    ref[..., :shape[1]] = x.to(torch.bfloat16).permute(0, 2, 3, 4, 1)
    assert torch.equal(_bits16(got), _bits16(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 32, 2, 3, 6), (2, 32, 3, 3, 5), (1, 5, 2, 2, 5), (3, 5, 1, 7, 3)], ids=lambda s: "x".join(map(str, s)))
def test_repack_gate_bit_for_bit(shape, device):
    """repack_gate_ncdhw_to_ndhwc_bf16 and its _v4 form: dy where the gate is > 0 (-0, +0 and negatives close it), +0 elsewhere and
    in the padded channels; dy's own bits (-0 included) pass unchanged."""
    K = _ops()
    gen = torch.Generator().manual_seed(sum(shape))
    dy = _with_specials(torch.randn(shape, generator=gen)).to(torch.bfloat16)
    dy[:, 0] = -0.0
    gate = _gate_image(shape, sum(shape) + 1)
    got = K.repack_gate_ncdhw_to_ndhwc_bf16(dy.to(device), gate.to(device)).cpu()
    ref = torch.zeros(got.shape, dtype=torch.bfloat16)
    ref[..., :shape[1]] = torch.where(gate > 0, dy, torch.zeros_like(dy)).permute(0, 2, 3, 4, 1)
    assert torch.equal(_bits16(got), _bits16(ref))
    assert int((_bits16(got) == -32768).sum()) > 0, "a -0 of dy is expected to pass an open gate"


# ---- GPU 7: exact homogeneity ---------------------------------------------------------------------------------------------------
def _assert_scalable(p):
    """Nothing reaches the subnormal range or overflows when x (and the bias) move by 2^+-20: on the reference's operands."""
    def smallest(t):
        return float(t[t != 0].abs().min())
    assert smallest(p.x) * smallest(p.w) * 2.0 ** -20 * 2.0 ** -24 > 2.0 ** -126
    assert smallest(p.x) * smallest(p.g) * 2.0 ** -20 * 2.0 ** -24 > 2.0 ** -126
    assert smallest(p.bias) * 2.0 ** -20 * 2.0 ** -24 > 2.0 ** -126
    for ref, s in ((p.y64, p.sy), (p.dw64, p.sdw)):
        assert float(s.max()) * 2.0 ** 20 < 2.0 ** 100 and smallest(ref) * 2.0 ** -20 > 2.0 ** -100


@pytest.mark.gpu
@pytest.mark.parametrize("family,c", [("v1", V1_CASES[2]), ("v3", V3_CASES[3]), ("first", FIRST_CASES[1]), ("first (v1 form)", FIRST_CASES[0])],
                         ids=["v1", "v3", "first-fallback", "first-loader"])
def test_forward_is_exactly_homogeneous(family, c, device):
    """x and the bias times 2^k give y times 2^k bit for bit (bf16 has float32's exponent range; every rounding moves with the
    exponent)."""
    K = _ops()
    p = _problem(c, "zero_mean")
    _assert_scalable(p)
    wp = K.conv3d_pack_weight_bf16(p.w.to(device))

    def run(k):
        x, bias = (p.x * 2.0 ** k).to(device), (p.bias * 2.0 ** k).to(device)
        if family.startswith("first"):
            return K.conv3d_fwd_bf16_f32in(x, wp, bias, c.co, c.pad, relu=True)[0].float()
        return K.conv3d_fwd_bf16(_ndhwc16(p.x * 2.0 ** k, device), None, wp, bias, c.ci, c.co, c.pad, relu=True).float()

    y0 = run(0)
    assert float(y0.abs().max()) > 0
    for k in (20, -20):
        assert torch.equal(run(k), y0 * 2.0 ** k), f"{family}: y(2^{k} x) is not 2^{k} y(x)"


@pytest.mark.gpu
@pytest.mark.parametrize("c", [WGRAD_CASES[1], WGRAD_CASES[6], WGRAD_CASES[7]], ids=_id)
def test_weight_gradient_is_exactly_homogeneous(c, device):
    """x times 2^k gives dW times 2^k bit for bit and leaves db's bits alone (PACK12, 17 and 32 channels)."""
    K = _ops()
    p = _problem(c, "zero_mean")
    _assert_scalable(p)
    gp = _ndhwc16(p.gg, device)
    dw0, db0 = K.conv3d_bwd_weight_bf16(_ndhwc16(p.x, device), gp, None, c.ci, c.co, c.pad)
    assert float(dw0.abs().max()) > 0
    for k in (20, -20):
        dw, db = K.conv3d_bwd_weight_bf16(_ndhwc16(p.x * 2.0 ** k, device), gp, None, c.ci, c.co, c.pad)
        assert torch.equal(dw, dw0 * 2.0 ** k) and torch.equal(db, db0), f"dW(2^{k} x) is not 2^{k} dW(x)"


if __name__ == "__main__":
    _measure()
