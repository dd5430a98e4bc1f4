"""The strided GEMM family of csrc/gemm_f32.hip -- gemm_bf16x3_kernel (three-term, one-term, A stored as bf16), gemm_rows_x3_kernel
(f32 and bf16 output), gemm_f32_kernel (PV_GEMM_EXACT_F32), split-K with sum_slabs_f32, colsum -- per element against a float64
product, at the shapes where each of their paths begins and ends -- and CPU tests that show the checker rejects a GEMM that is
subtly wrong.

Reference.  `_ref`: c64 = a @ b in float64 on the CPU, bias and residual (and the tensor accumulated into) added in float64, ReLU
applied in float64; S = sum_k |a_ik b_kj| + |bias_j| + |res_ij| + |acc_ij| in float64; under ReLU relu(c64) with the same S.  For
bf16_operands=True and for an A stored as bf16, c64 and S are those of the operands rounded once to bf16 (nearest even), and the
result must NOT be within the bound of the unrounded operands' product.  colsum: c64 = sum_r x_rc (+ acc_c), S = sum_r |x_rc| (+ |acc_c|).

Bound, per element, never a norm (`_check`, through conv2d_f32_helpers._within):
    |c - c64| <= c_regime 2^-24 S   (+ 2^-8 |c64| for a bf16 result)
The bf16 term is bfloat16's unit roundoff: 8 significant bits, so round-to-nearest-even moves a value by up to half a step =
2^-8 of the bottom of its binade.  (2^-9, first written down for this file, is that half step relative to the TOP of a binade:
on the CPU the correctly rounded float32 results of (256, 96, 192) reach 1.99 x 2^-9 |c64|.)  The bf16-output kernel is held
to more than this anyway: bitwise the float32 kernel's result rounded.

Regimes (seeded, on the CPU): `zero_mean` randn operands, at every shape; `positive` |randn| operands (as ReLU activations are:
nothing cancels, accumulation error is at its largest) at K <= 128 only -- a legitimate f32 accumulator updated once per 16-deep
step reaches 39 x 2^-24 S at K = 19 456 and 62 at K = 70 000 with positive operands, and a constant that admits that hides the rest.

Constants.  From the REFERENCE's own error, never from the kernels: worst err / (2^-24 S) of two CPU evaluations of every
(shape, regime) of this file, times 4 (the margin for another summation order inside the matrix instruction):
  float32 torch `a @ b` (for the one-term rows: of the rounded operands), and
  `_emulate`, the kernels' arithmetic as the comments of gemm_f32.hip state it: operands split by truncation into three bf16
  terms, the partial products mm, lh, hl, mh, hm, hh, one f32 accumulator updated once per 16-deep K step and product; one-term:
  operands rounded, one product; split-K: that per chunk of ceil(ceil(K / splits) / 16) 16, the slabs added as sum_slabs_f32
  documents it (eight groups take slabs g, g + 8, ... in index order, the groups are then added in order).
`python tests/test_gpu_gemm_numerics.py` prints (x3 / x1: three-term / one-term; rows-form shapes are slices of (2079, K, 128)):
    shape (m, k, n)       zero_mean x3    zero_mean x1    positive x3     positive x1        (float32 torch / emulation)
    1x1x1                 0.13 / 0.13     0    / 0        0.32 / 1.56     0    / 0
    128x32x64             3.22 / 2.59     1.29 / 0.92     6.01 / 3.62     2.79 / 1.49
    127x31x63             3.22 / 2.74     1.11 / 0.94     6.03 / 3.48     2.71 / 1.50
    129x33x65             3.17 / 2.98     1.16 / 0.76     5.90 / 5.90     3.03 / 2.19
    130x80x65             3.64 / 2.16     1.44 / 0.99     9.22 / 6.15     5.22 / 2.30
    129x1000x66           1.31 / 2.22     0.59 / 0.90        -               -
    5x37x7                1.80 / 0.73     0.48 / 0.34     2.94 / 3.47     1.74 / 1.63
    256x96x192            3.91 / 2.38     2.13 / 1.11     10.32 / 6.44    5.00 / 2.55
    2079x38x70            3.82 / 3.49     1.93 / 1.34     6.79 / 5.94     4.42 / 2.26
    2079xKx128, K = 64    4.70 / 2.90     1.82 / 1.26     10.96 / 5.73    5.37 / 2.22
      48, 50, 38, 49, 37  <= 4.99 / 3.56  <= 2.40 / 1.40  <= 10.17 / 7.53 <= 4.64 / 2.76
      6, 8, 9, 16, 17, 33 <= 4.41 / 4.51  <= 2.15 / 1.37  <= 7.16 / 6.51  <= 4.70 / 2.48
      K = 1               1.00 / 6.37     0    / 0        1.00 / 6.87     0    / 0
    8229x64x1024          5.91 / 3.55     3.34 / 1.41     11.35 / 6.96    6.79 / 2.60
    8229x38x1024          5.68 / 5.90     2.77 / 1.90     9.33 / 6.75     5.10 / 2.40
    split-K 48x257x37 (2 splits) 2.55 / 0.95, 48x512x37 (2) 1.38 / 0.99, 48x513x37 (3) 2.12 / 1.51, 48x19456x37 (76) 0.24 / 0.16,
            130x4097x65 (17) 0.53 / 0.37 (x3; x1 lower throughout)
    worst zero_mean: float32 torch 5.91, emulation 6.37 -> C["zero_mean"] = 25.5
    worst positive:  float32 torch 11.35, emulation 7.53 -> C["positive"] = 45.4
(K = 1 is the three-term form's own error laid bare: one product, whose dropped terms ml + lm + ll reach 2^-21 of it -- h has
8 significant bits, so m < 2^-7 and l < 2^-15 of the operand's binade -- where gemm_f32.hip's comment says 2^-23.)
colsum, the same two ways plus the documented order (`_emulate_colsum`: per chunk four lanes with two alternating partial sums
each, lanes added in order, chunks through sum_slabs' grouped order); float32 torch / float32 row after row / emulation:
    1x1        0 / 0 / 0 both regimes          31x5  zero_mean 0.51 / 0.52 / 0.21   positive 0.38 / 1.36 / 1.32
    32x64      zero_mean 0.95 / 0.89 / 0.79    positive 2.35 / 4.00 / 1.50
    33x65      zero_mean 0.94 / 1.22 / 0.60    positive 2.36 / 3.19 / 2.60
    16385x70   zero_mean 0.07 / 1.18 / 0.06    positive 2.19 / 73.42 / 2.37
    70001x38   zero_mean 0.03 / 0.86 / 0.03    positive 2.57 / 134.0 / 2.12
    -> C_COLSUM["zero_mean"] = 4.9, C_COLSUM["positive"] = 536 (the row-after-row float32 sum of 70 001 positive numbers: with
    that constant a missing row of (70001, 38) is 2.1 x the bound only; the zero_mean constant sees it at every shape)

What the checker is sensitive to (CPU tests below).  A partial product dropped (mm or lh: 2^-16 of every product) is 73 ... 318
x 2^-24 S at K <= 70 but only 9 at K = 19 456, where the float64 sum S has grown past the kernel's error: the small-K cases
carry this sensitivity, and REJECT_CASES are K <= 128 shapes.  There the checker also rejects: the last k element dropped, the
bias added twice or not at all, the residual read one row off, two columns of the last ragged column tile swapped (which the
max-over-max check of test_gpu_perceiver_ops.py lets through when those columns are small), the one-term form with truncated
operands, the f32-accurate product where the rounded operands' product is due, a split-K sum without its last slab, a colsum
without its last row.

GPU cases.  Tiles from the source: three-term / one-term tiled 128 x 64, K panels of 32; exact 128 x 64, panels of 16; rows
form 32-row x 64-column blocks.
  1 tiled   TILED_SHAPES: (1,1,1) nothing whole; (128,32,64) one whole tile and panel, quads only; (127,31,63) per element only;
            (129,33,65) whole and ragged tiles and a one-element panel in one launch; (130,80,65) K = 5 x 16; (129,1000,66);
            (5,37,7); tall shapes that the rows rule refuses: (2047,38,70), and (2079,38,70) with A one element off its base.
            x A / B row-major or transposed view (the four A_KC / B_KC instantiations) x three-term, one-term, A stored as bf16.
            Quad-path disqualifiers on (129,33,65) and (256,96,192), A and B, either storage: base off by 1, 2, 3 (and 4: eligible
            for f32, 8 bytes for bf16) elements, leading dimension + 1 and + 2, inner stride 2, stride 0.
  2 epilogues   bias / ReLU / residual / all three / residual with ldr = n + 3 on (129,33,65) and (2079,38,70) (rows form);
            `out` as column slice, row slice and both of a sentinel-filled tensor.
  3 batches  (3,), (2,4), stride-0 A and B; per-head views [b, n, h d] -> [b, h, n, d], q k^T and p v through an `out` head view, d = 8
            and 6 -- at which no workgroup is eligible for quads at all (K = d < 32 in q k^T, n = d < 64 in p v) -- and d = 68 and 66,
            the smallest head sizes where aligned and misaligned heads do mix quad and per-element workgroups in one launch.
  4 exact    PV_GEMM_EXACT_F32 (read per call) on the shapes of 1 and the epilogues of 2: same bound, and within the sum of both bounds
            of the default result.  (PV_GEMM_NO_ROWS_FORM is read once per process and cannot be flipped in a test.)
  5 rows     K = 64, 48 (VEC 4, KSTEPS 4, 3), 50, 38 (VEC 2), 49, 37 (VEC 1), 1, 6, 8, 9, 16, 17, 33 (edges of the lanes' 8-element
            halves), A = wide[:, :K] of K + 2 / K + 1 columns; m = 2048, 2049, 2079 (2047: tiled); n = 64, 70, 72, 5; B = w.t() (quads
            when K % 4 == 0) and contiguous (pairs); (8229, K, 1024): the persistent loop's second trip and mid-trip break.
  6 bf16 out   the K of 5, m = 2048, 2079, n = 64, 128 (LDS tile), 72 (tile, then lane by lane), 70 (lane by lane); bitwise
            gemm(...).to(bfloat16); pv_gemm_rows_bf16out_f32 with ldc = n + 8 and n + 1 into a sentinel-filled buffer.
  7 split-K  (48,257,37) 2 splits of 144: the second starts at k = 16 mod 32; (48,512,37); (48,513,37) 3 x 176; (48,19456,37)
            76 x 256; (130,4097,65) 17 splits, the last of one element; A also as a .t() view and stored as bf16; equal bits
            twice; accumulate_into; an empty third split (k = 32, k_splits = 3) through pv_gemm_ex_f32.
  8 colsum   COLSUM_SHAPES, both regimes, accumulate_into.

Measured on the MI355X with these constants, worst error / bound over all cases: tiled x3 0.25 ((2047, 1, 72): the K = 1 product
of the table), tiled x1 0.08, bf16 A 0.06, exact 0.20, rows x3 0.25 ((8229, 38, 1024) zero_mean), rows x1 0.10, split-K 0.12,
colsum 0.17 ((33, 65) zero_mean), bf16 output 1.00 ((2079, 16, 128): 0.996, the rounding term alone -- a value half a step from
both neighbours at the bottom of its binade; with 2^-9 it would read 1.99): every kernel stays within 1.1 x the worst of the CPU
evaluations above.  No case found a fault in the kernels.  The 241 GPU cases of this file take 7 s together, the slowest
((8229, K, 1024)) 0.3 s each.
"""
import ctypes

import pytest
import torch

from conv2d_f32_helpers import _ops, _within

U32 = 2.0 ** -24
U16 = 2.0 ** -8          # unit roundoff of bfloat16 (8 significant bits): see the module docstring
SENTINEL = 1.2345678e30          # finite: its bits are compared, never its value

# 4 x the reference-only ratios of the module docstring
C = {"zero_mean": 25.5, "positive": 45.4}
C_COLSUM = {"zero_mean": 4.9, "positive": 536.0}

REGIMES = ("zero_mean", "positive")
POSITIVE_MAX_K = 128

TILED_SHAPES = [(1, 1, 1), (128, 32, 64), (127, 31, 63), (129, 33, 65), (130, 80, 65), (129, 1000, 66), (5, 37, 7)]
TALL_TILED_SHAPES = [(2047, 38, 70), (2079, 38, 70)]      # tall, but refused by the rows rule (m < 2048; A base one element off)
QUAD_SHAPES = [(129, 33, 65), (256, 96, 192)]
ROWS_K = [64, 48, 50, 38, 49, 37, 1, 6, 8, 9, 16, 17, 33]
ROWS_M = [2048, 2049, 2079, 2047]
ROWS_N = [64, 70, 72, 5]
ROWS_M_MAX, ROWS_N_MAX = 2079, 72
BF16OUT_M = [2048, 2079]
BF16OUT_N = [64, 128, 72, 70]
LOOP_SHAPES = [(8229, 64, 1024), (8229, 38, 1024)]
EPILOGUE_SHAPES = [(129, 33, 65), (2079, 38, 70)]
SPLITK_SHAPES = [(48, 257, 37), (48, 512, 37), (48, 513, 37), (48, 19456, 37), (130, 4097, 65)]
COLSUM_SHAPES = [(1, 1), (31, 5), (32, 64), (33, 65), (16385, 70), (70001, 38)]
EPILOGUES = ["bias", "relu", "res", "bias+res+relu", "res_slice"]
# partial products of the three-term form in the kernels' order (A term, B term)
ORDER = ("mm", "lh", "hl", "mh", "hm", "hh")


def _regimes(k):
    return [r for r in REGIMES if r == "zero_mean" or k <= POSITIVE_MAX_K]


def _with_regimes(shapes):
    return [(s, r) for s in shapes for r in _regimes(s[1])]


# every (shape, regime) of this file whose products differ: the rows-form shapes are slices of (2079, K, 72) / (2079, K, 128)
TABLE_SHAPES = (TILED_SHAPES + [QUAD_SHAPES[1]] + TALL_TILED_SHAPES[1:] + [(ROWS_M_MAX, k, BF16OUT_N[1]) for k in ROWS_K] + LOOP_SHAPES)
TABLE_CASES = _with_regimes(TABLE_SHAPES)
REJECT_CASES = _with_regimes([(128, 32, 64), (127, 31, 63), (129, 33, 65), (130, 80, 65), (5, 37, 7), (2079, 38, 70)])


def _case_id(case):
    (m, k, n), regime = case
    return f"{m}x{k}x{n}-{regime}"


def _shape_id(shape):
    return "x".join(str(s) for s in shape)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _operands(m, k, n, regime):
    """a [m, k], b [k, n] (the transposed view of a weight [n, k], as nn.Linear passes it), bias [n], res [m, n]: float32, CPU."""
    g = torch.Generator().manual_seed(1000003 * m + 10007 * k + 101 * n + (regime == "positive"))
    a, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    bias, res = torch.randn(n, generator=g), torch.randn(m, n, generator=g)
    if regime == "positive":
        a, w, bias, res = a.abs(), w.abs(), bias.abs(), res.abs()
    return a, w.t(), bias, res


def _colsum_input(rows, cols, regime):
    g = torch.Generator().manual_seed(7919 * rows + cols)
    x, acc = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g)
    return (x.abs(), acc.abs()) if regime == "positive" else (x, acc)


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)      # nearest even


def _trunc16(t):
    """float32 -> the bf16 value below it in magnitude (the low 16 bits cleared)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ---- float64 reference and the checker -------------------------------------------------------------------------------------
def _ref(a, b, bias=None, res=None, relu=False, acc=None, rounded=False):
    """(c64, S): the float64 product with its epilogue, and its sum of absolute terms.  rounded: of the operands rounded once to
    bf16 (an A already stored as bf16 is taken as it is)."""
    a64 = (_bf16(a) if rounded and a.dtype == torch.float32 else a).double()
    b64 = (_bf16(b) if rounded else b).double()
    c, s = a64 @ b64, a64.abs() @ b64.abs()
    for t in (bias, res, acc):
        if t is not None:
            c, s = c + t.double(), s + t.double().abs()
    return (c.clamp_min(0) if relu else c), s


def _colsum_ref(x, acc=None):
    c, s = x.double().sum(0), x.double().abs().sum(0)
    if acc is not None:
        c, s = c + acc.double(), s + acc.double().abs()
    return c, s


def _ratio(got, c64, s, c, bf16_out=False):
    """Worst error / bound over the elements (a non-finite result counts as infinite)."""
    got = got.detach().double().cpu()
    bound = c * U32 * s + (U16 * c64.abs() if bf16_out else 0.0) + 1e-30
    ratio = (got - c64).abs() / bound
    return float(torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).max())


def _check(form, got, c64, s, c, what, bf16_out=False):
    """|got - c64| <= c 2^-24 S (+ 2^-8 |c64| for a bf16 result), per element; prints the worst error / bound."""
    worst = _ratio(got, c64, s, c, bf16_out)
    print(f"[{form}] {what}: error / bound {worst:.3f}")
    absref = s + (U16 / (c * U32)) * c64.abs() if bf16_out else s          # tol * absref == the bound above
    _within(got.detach().float(), c64, absref, tol=c * U32, what=f"{form} {what}")
    return worst


def _norm_check(got, c64, tol=2e-6):
    """The max-over-max check of tests/test_gpu_perceiver_ops.py."""
    return float((got.double() - c64).abs().max() / c64.abs().max()) < tol


# ---- CPU emulation of the kernels' documented arithmetic -------------------------------------------------------------------
def _split3(x):
    """x = h + m + l, three bf16 terms by truncation (both subtractions exact)."""
    h = _trunc16(x)
    r = x - h
    m = _trunc16(r)
    return {"h": h.double(), "m": m.double(), "l": _trunc16(r - m).double()}


def _emulate(a, b, terms=3, drop=None, kbeg=0, kend=None, truncate=False):
    """gemm_bf16x3_kernel / gemm_rows_x3_kernel as their comments state them: one f32 accumulator per element, updated once per
    16-deep K step and partial product (exact bf16 products, summed here in float64 and rounded once into the accumulator).
    terms 3: operands split by truncation, products mm, lh, hl, mh, hm, hh (`drop` leaves one out); terms 1: operands rounded to
    nearest even (`truncate`: truncated instead), one product.  An A stored as bf16 is exact already."""
    a, b = a.float(), b.float()
    kend = a.shape[1] if kend is None else kend
    if terms == 3:
        sa, sb = _split3(a), _split3(b)
        prods = [(sa[p[0]], sb[p[1]]) for p in ORDER if p != drop]
    else:
        rnd = _trunc16 if truncate else _bf16
        prods = [(rnd(a).double(), rnd(b).double())]
    acc = torch.zeros(a.shape[0], b.shape[1])
    for k0 in range(kbeg, kend, 16):
        k1 = min(k0 + 16, kend)
        for x, y in prods:
            acc = (acc.double() + x[:, k0:k1] @ y[k0:k1]).float()
    return acc


def _epilogue(acc, bias=None, res=None, relu=False):
    """The kernels' epilogue in float32: + bias, + residual, ReLU."""
    if bias is not None:
        acc = acc + bias
    if res is not None:
        acc = acc + res
    return acc.clamp_min(0) if relu else acc


def _sum_slabs(slabs, acc=None):
    """sum_slabs_f32's order: eight groups add slabs g, g + 8, ... in index order, the group sums are added in group order."""
    groups = []
    for g in range(8):
        s = torch.zeros_like(slabs[0])
        for slab in slabs[g::8]:
            s = s + slab
        groups.append(s)
    t = groups[0]
    for s in groups[1:]:
        t = t + s
    return t if acc is None else acc + t


def _splits(m, k, n):
    """hip_ops.gemm_splitk's split count (SPLITK_TARGET_WORKGROUPS = 1024, SPLITK_MIN_CHUNK = 256) and pv_gemm_ex_f32's chunk."""
    tiles = ((m + 127) // 128) * ((n + 63) // 64)
    splits = max(1, min((1024 + tiles - 1) // tiles, (k + 255) // 256, 4096))
    return splits, _chunk(k, splits)


def _chunk(k, splits):
    return ((k + splits - 1) // splits + 15) // 16 * 16


def _emulate_splitk(a, b, splits, terms=3, n_slabs=None, acc=None):
    k = a.shape[1]
    chunk = _chunk(k, splits)
    slabs = [_emulate(a, b, terms, kbeg=min(s * chunk, k), kend=min((s + 1) * chunk, k)) for s in range(splits)]
    return _sum_slabs(slabs[:n_slabs], acc)


def _colsum_chunks(rows):
    chunks = min((rows + 31) // 32, 512)
    per = (rows + chunks - 1) // chunks
    return (rows + per - 1) // per, per


def _emulate_colsum(x, acc=None):
    """colsum_partial_f32 + sum_slabs_f32: per chunk of `per` rows four lanes take rows r, r + 4, ... into two alternating
    partial sums; a lane's sum is s0 + s1, the four lanes are added in order, the chunks through sum_slabs' grouped order.
    (Rows of zeros pad the last chunk and a lane's last pair: adding 0.f changes nothing.)"""
    rows, cols = x.shape
    chunks, per = _colsum_chunks(rows)
    p8 = (per + 7) // 8 * 8
    xp = torch.zeros(chunks, p8, cols)
    for c in range(chunks):
        r0, r1 = c * per, min((c + 1) * per, rows)
        xp[c, :r1 - r0] = x[r0:r1]
    xp = xp.view(chunks, p8 // 8, 2, 4, cols)            # row of a chunk = 8 i + 4 t + lane
    s = torch.zeros(chunks, 2, 4, cols)
    for i in range(p8 // 8):
        s = s + xp[:, i]
    lanes = s[:, 0] + s[:, 1]
    part = ((lanes[:, 0] + lanes[:, 1]) + lanes[:, 2]) + lanes[:, 3]
    return _sum_slabs(list(part), acc)


def _colsum_row_order(x):
    """A plain float32 column sum, one row after the other."""
    s = x[0].clone().numpy()
    for row in x[1:].numpy():
        s += row
    return torch.from_numpy(s)


# ---- CPU: the checker accepts the reference-only evaluations ----------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE_CASES, ids=_case_id)
def test_checker_accepts_float32_torch_and_the_emulation(case):
    (m, k, n), regime = case
    a, b, bias, res = _operands(m, k, n, regime)
    c64, s = _ref(a, b)
    _check("cpu", a @ b, c64, s, C[regime], f"float32 torch {_case_id(case)}")
    _check("cpu", _emulate(a, b), c64, s, C[regime], f"emulation x3 {_case_id(case)}")
    c16, s16 = _ref(a, b, rounded=True)
    _check("cpu", _bf16(a) @ _bf16(b), c16, s16, C[regime], f"float32 torch, rounded operands {_case_id(case)}")
    _check("cpu", _emulate(a, b, terms=1), c16, s16, C[regime], f"emulation x1 {_case_id(case)}")
    if m <= 256:      # epilogue and bf16 store
        e64, es = _ref(a, b, bias, res, relu=True)
        got = _epilogue(_emulate(a, b), bias, res, relu=True)
        _check("cpu", got, e64, es, C[regime], f"emulation x3 with epilogue {_case_id(case)}")
        _check("cpu", _bf16(got), e64, es, C[regime], f"emulation x3, bf16 store {_case_id(case)}", bf16_out=True)


@pytest.mark.parametrize("shape", SPLITK_SHAPES, ids=_shape_id)
def test_checker_accepts_the_splitk_emulation_and_rejects_a_missing_last_slab(shape):
    m, k, n = shape
    a, b, _, acc = _operands(m, k, n, "zero_mean")
    splits, _ = _splits(m, k, n)
    c64, s = _ref(a, b)
    _check("cpu", a @ b, c64, s, C["zero_mean"], f"float32 torch {_shape_id(shape)}")
    for terms in (3, 1):
        r64, rs = _ref(a, b, rounded=terms == 1)
        _check("cpu", _emulate_splitk(a, b, splits, terms), r64, rs, C["zero_mean"], f"split-K emulation x{terms} {_shape_id(shape)}")
    a64, as_ = _ref(a, b, acc=acc)
    _check("cpu", _emulate_splitk(a, b, splits, acc=acc), a64, as_, C["zero_mean"], f"split-K emulation, accumulating {_shape_id(shape)}")
    if k <= 4097:      # (at K = 19 456 one slab of 76 is missing: no different in kind, and slower)
        with pytest.raises(AssertionError, match="x the bound"):
            _check("cpu", _emulate_splitk(a, b, splits, n_slabs=splits - 1), c64, s, C["zero_mean"], "last slab missing")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=_shape_id)
def test_colsum_checker_accepts_float32_sums_and_rejects_a_missing_last_row(shape, regime):
    x, acc = _colsum_input(*shape, regime)
    c64, s = _colsum_ref(x)
    c = C_COLSUM[regime]
    _check("cpu", x.sum(0), c64, s, c, f"float32 torch colsum {_shape_id(shape)} {regime}")
    _check("cpu", _colsum_row_order(x), c64, s, c, f"row-order colsum {_shape_id(shape)} {regime}")
    _check("cpu", _emulate_colsum(x), c64, s, c, f"colsum emulation {_shape_id(shape)} {regime}")
    a64, as_ = _colsum_ref(x, acc)
    _check("cpu", _emulate_colsum(x, acc), a64, as_, c, f"colsum emulation, accumulating {_shape_id(shape)} {regime}")
    with pytest.raises(AssertionError, match="x the bound"):
        _check("cpu", _emulate_colsum(x[:-1]) if shape[0] > 1 else torch.zeros(shape[1]), c64, s, c, "last row missing")


# ---- CPU: the checker rejects what it must ----------------------------------------------------------------------------------
def _rejected(got, c64, s, regime, what, bf16_out=False):
    with pytest.raises(AssertionError, match="x the bound"):
        _check("cpu", got, c64, s, C[regime], what, bf16_out)


@pytest.mark.parametrize("case", REJECT_CASES, ids=_case_id)
def test_checker_rejects_subtly_wrong_products(case):
    (m, k, n), regime = case
    a, b, bias, res = _operands(m, k, n, regime)
    c64, s = _ref(a, b)
    for drop in ("mm", "lh"):      # 2^-16 of each product
        _rejected(_emulate(a, b, drop=drop), c64, s, regime, f"partial product {drop} dropped")
    _rejected(_emulate(a[:, :-1], b[:-1]), c64, s, regime, "last k element dropped")
    e64, es = _ref(a, b, bias, res)
    acc = _emulate(a, b)
    _check("cpu", _epilogue(acc, bias, res), e64, es, C[regime], "correct epilogue")
    _rejected(_epilogue(acc, 2 * bias, res), e64, es, regime, "bias added twice")
    _rejected(_epilogue(acc, None, res), e64, es, regime, "bias not added")
    _rejected(_epilogue(acc, bias, res.roll(1, 0)), e64, es, regime, "residual read one row off")
    swapped = acc.clone()
    j = n - 2 if (n - 1) % 64 else None      # two columns in the last ragged column tile (n % 64 == 1: it holds one column)
    if j is not None:
        swapped[:, [j, j + 1]] = acc[:, [j + 1, j]]
        _rejected(swapped, c64, s, regime, "two columns of the last ragged tile swapped")
    c16, s16 = _ref(a, b, rounded=True)
    _check("cpu", _emulate(a, b, terms=1), c16, s16, C[regime], "one term, rounded")
    _rejected(_emulate(a, b, terms=1, truncate=True), c16, s16, regime, "one term, operands truncated instead of rounded")
    _rejected(_emulate(a, b), c16, s16, regime, "the f32-accurate product where the product of the rounded operands is due")


def test_checker_rejects_swapped_columns_that_a_norm_check_lets_through():
    """Columns 64 ... 69 of (2079, 38, 70), the ragged second column block, scaled by 2^-24: two of them swapped is an error of
    the order of those elements -- 6e-8 of the matrix's largest, inside the 2e-6 of a max-over-max check."""
    m, k, n = 2079, 38, 70
    a, b, _, _ = _operands(m, k, n, "zero_mean")
    b = b.clone()
    b[:, 64:] *= 2.0 ** -24
    c64, s = _ref(a, b)
    good = _emulate(a, b)
    _check("cpu", good, c64, s, C["zero_mean"], "small ragged columns")
    bad = good.clone()
    bad[:, [68, 69]] = good[:, [69, 68]]
    assert _norm_check(bad, c64), "the norm check is expected to let the swap through"
    _rejected(bad, c64, s, "zero_mean", "columns 68 and 69 swapped")


# ---- GPU helpers -----------------------------------------------------------------------------------------------------------
def _dev(x, device, transposed=False):
    """x on the device, stored row-major or stored as its transpose and handed over as the .t() view."""
    return x.t().contiguous().to(device).t() if transposed else x.contiguous().to(device)


def _strided(x, device, transposed=False, off=0, ld_pad=0, step=1):
    """x (or, transposed, x.t()) inside a NaN-filled buffer: base `off` elements in, leading dimension padded by ld_pad, inner
    stride `step`.  An element read outside the view would poison the product."""
    p = x.t() if transposed else x
    r, c = p.shape
    ld = c * step + ld_pad
    buf = torch.full((off + r * ld + 8,), float("nan"), dtype=x.dtype).to(device)
    v = torch.as_strided(buf, (r, c), (ld, step), off)
    v.copy_(p.to(device))
    return v.t() if transposed else v


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _form(terms, a16=False, m=0, k=0, rows_ok=True):
    if a16:
        return "bf16 A"
    kind = "rows" if rows_ok and m >= 2048 and k <= 64 else "tiled"
    return f"{kind} x{terms}"


FORMS = {"x3": (3, False), "x1": (1, False), "a16": (1, True)}


# ---- GPU 1: the tiled kernel, four layouts x three forms ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", _with_regimes(TILED_SHAPES + TALL_TILED_SHAPES), ids=_case_id)
def test_tiled_kernel_in_four_layouts(case, form, device):
    """gemm_bf16x3_kernel<A_KC, B_KC, TERMS, A_BF16>: A and B row-major or transposed views."""
    K = _ops()
    (m, k, n), regime = case
    terms, a16 = FORMS[form]
    a, b, _, _ = _operands(m, k, n, regime)
    c64, s = _ref(a, b, rounded=terms == 1)
    c32, s32 = _ref(a, b)
    for ta in (False, True):
        for tb in (False, True):
            src = a.to(torch.bfloat16) if a16 else a
            # (2079 rows, row-major f32 A: one element off its base, or the rows form would take it)
            ad = _strided(src, device, off=1) if (m >= 2048 and not ta and not a16) else _dev(src, device, ta)
            got = K.gemm(ad, _dev(b, device, tb), bf16_operands=terms == 1)
            _check(_form(terms, a16), got, c64, s, C[regime], f"{_case_id(case)} A^T {ta} B^T {tb}")
            if terms == 1 and m * n > 1:
                assert _ratio(got, c32, s32, C[regime]) > 1.0, "the one-term form gave the f32-accurate product"


DISQUALIFIERS = {"off1": dict(off=1), "off2": dict(off=2), "off3": dict(off=3), "off4": dict(off=4), "ld+1": dict(ld_pad=1),
                 "ld+2": dict(ld_pad=2), "step2": dict(step=2), "stride0": None}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DISQUALIFIERS))
@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=_shape_id)
def test_tiled_kernel_quad_path_disqualifiers(shape, operand, kind, device):
    """One operand, in either memory layout, as a view that must not (or, for bf16 at 4 elements = 8 bytes, f32 at 4 elements
    = 16 bytes: may) take the 16-byte quad loads; the other operand plain row-major."""
    K = _ops()
    m, k, n = shape
    a, b, _, _ = _operands(m, k, n, "zero_mean")
    for transposed in (False, True):
        for form, (terms, a16) in FORMS.items():
            if a16 and operand == "B":
                continue
            x = a if operand == "A" else b
            if a16:
                x = x.to(torch.bfloat16)
            if kind == "stride0":      # equal rows (row-major storage) / equal columns (transposed storage)
                if transposed:
                    x, xd = x[:, :1].expand(*x.shape), x[:, :1].contiguous().to(device).expand(*x.shape)
                else:
                    x, xd = x[:1].expand(*x.shape), x[:1].contiguous().to(device).expand(*x.shape)
            else:
                xd = _strided(x, device, transposed, **DISQUALIFIERS[kind])
            al, bl = (x, b) if operand == "A" else (a, x)
            ad, bd = (xd, _dev(b, device)) if operand == "A" else (_dev(a.to(torch.bfloat16) if a16 else a, device), xd)
            c64, s = _ref(al, bl, rounded=terms == 1)
            got = K.gemm(ad, bd, bf16_operands=terms == 1)
            _check(_form(terms, a16), got, c64, s, C["zero_mean"], f"{_shape_id(shape)} {operand} {kind} transposed {transposed}")


# ---- GPU 2: epilogues and output views -------------------------------------------------------------------------------------
def _epilogue_args(epi, bias, res, device):
    """-> (bias, res on the CPU, bias, res on the device, relu)."""
    use_bias, use_res, relu = "bias" in epi, "res" in epi, "relu" in epi
    bd = bias.to(device) if use_bias else None
    rd = None
    if epi == "res_slice":      # ldr = n + 3
        rd = _strided(torch.cat([res, res[:, :3]], dim=1), device)[:, :res.shape[1]]
    elif use_res:
        rd = res.to(device)
    return (bias if use_bias else None), (res if use_res else None), bd, rd, relu


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", EPILOGUE_SHAPES, ids=_shape_id)
def test_epilogues(shape, epi, terms, device):
    """bias, ReLU and residual (also with ldr > n) in the tiled and the rows kernel."""
    K = _ops()
    m, k, n = shape
    for regime in REGIMES:
        a, b, bias, res = _operands(m, k, n, regime)
        bc, rc, bd, rd, relu = _epilogue_args(epi, bias, res, device)
        c64, s = _ref(a, b, bc, rc, relu, rounded=terms == 1)
        if relu and regime == "zero_mean":      # (`positive` clamps nothing: there ReLU must change nothing)
            assert 0.05 < float((c64 == 0).double().mean()) < 0.95, "ReLU is expected to clamp some elements and keep some"
        got = K.gemm(a.to(device), _dev(b, device, True), bias=bd, relu=relu, residual=rd, bf16_operands=terms == 1)
        _check(_form(terms, m=m, k=k), got, c64, s, C[regime], f"{_shape_id(shape)} {epi} {regime}")


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("shape", EPILOGUE_SHAPES, ids=_shape_id)
def test_output_views_leave_their_surroundings_alone(shape, terms, device):
    """`out` as a column slice (ldc > n), a row slice and both of a sentinel-filled tensor: the product inside, the sentinel's
    bits everywhere else."""
    K = _ops()
    m, k, n = shape
    a, b, bias, _ = _operands(m, k, n, "zero_mean")
    c64, s = _ref(a, b, bias, rounded=terms == 1)
    for r0, c0, rows, cols in [(0, 3, m, n + 5), (2, 0, m + 4, n), (2, 3, m + 4, n + 5)]:
        big = torch.full((rows, cols), SENTINEL, device=device)
        ret = K.gemm(a.to(device), _dev(b, device, True), bias=bias.to(device), out=big[r0:r0 + m, c0:c0 + n], bf16_operands=terms == 1)
        assert ret.data_ptr() == big[r0:r0 + m, c0:c0 + n].data_ptr()
        _check(_form(terms, m=m, k=k), big[r0:r0 + m, c0:c0 + n], c64, s, C["zero_mean"], f"{_shape_id(shape)} out at ({r0}, {c0}) of {rows} x {cols}")
        outside = torch.ones(rows, cols, dtype=torch.bool)
        outside[r0:r0 + m, c0:c0 + n] = False
        assert bool((_bits(big.cpu())[outside] == _bits(torch.tensor([SENTINEL]))).all()), "written outside the m x n view"


# ---- GPU 3: batches --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("batch", [(3,), (2, 4)], ids=["3", "2x4"])
def test_batched_products(batch, terms, device):
    """One and two leading dims, B also as a transposed view, a stride-0 broadcast A and a stride-0 broadcast B."""
    K = _ops()
    m, k, n = 129, 33, 65
    g = torch.Generator().manual_seed(len(batch))
    a, b = torch.randn(batch + (m, k), generator=g), torch.randn(batch + (k, n), generator=g)
    one = terms == 1
    c64, s = _ref(a, b, rounded=one)
    ad, bd = a.to(device), b.to(device)
    bt = b.transpose(-1, -2).contiguous().to(device).transpose(-1, -2)
    form = _form(terms)
    _check(form, K.gemm(ad, bd, bf16_operands=one), c64, s, C["zero_mean"], f"batch {batch}")
    _check(form, K.gemm(ad, bt, bf16_operands=one), c64, s, C["zero_mean"], f"batch {batch}, B^T view")
    a0, b0 = a[(0,) * len(batch)], b[(0,) * len(batch)]
    c64, s = _ref(a0, b, rounded=one)
    _check(form, K.gemm(a0.to(device).expand(batch + (m, k)), bd, bf16_operands=one), c64, s, C["zero_mean"], f"batch {batch}, A broadcast")
    c64, s = _ref(a, b0, rounded=one)
    _check(form, K.gemm(ad, b0.to(device).expand(batch + (k, n)), bf16_operands=one), c64, s, C["zero_mean"], f"batch {batch}, B broadcast")


def _heads(t, h):
    b, n, c = t.shape
    return t.view(b, n, h, c // h).permute(0, 2, 1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("d", [8, 6, 68, 66])
def test_per_head_views(d, terms, device):
    """q k^T and p v over the per-head permuted views [b, n, h d] -> [b, h, n, d] of perceiver_functional, p v written through an
    `out` head view.  Head bases are 16-byte aligned for d = 8 and 68 and misaligned in the odd heads for d = 6 and 66.
    (At d = 8 and 6 NO workgroup can take the quad path: K = d < 32 is a ragged panel in q k^T, n = d < 64 a ragged tile in p v.
    d = 68 and 66 are the smallest head sizes at which one launch does mix quad and per-element workgroups: one whole 32-deep
    panel in q k^T, one whole 64-column tile of V in p v, h d a multiple of 4.)"""
    K = _ops()
    b, h, nq, nk = 2, 2, 130, 70
    g = torch.Generator().manual_seed(d)
    q, kv = torch.randn(b, nq, h * d, generator=g), torch.randn(b, nk, 2 * h * d, generator=g)
    p = torch.randn(b, h, nq, nk, generator=g).softmax(dim=-1)
    one = terms == 1
    qd, kvd = q.to(device), kv.to(device)
    kh, vh = _heads(kv[..., :h * d], h), _heads(kv[..., h * d:], h)
    c64, s = _ref(_heads(q, h), kh.transpose(-1, -2), rounded=one)
    got = K.gemm(_heads(qd, h), _heads(kvd[..., :h * d], h).transpose(-1, -2), bf16_operands=one)
    _check(_form(terms), got, c64, s, C["zero_mean"], f"q k^T, head dim {d}")
    c64, s = _ref(p, vh, rounded=one)
    o = torch.full((b, nq, h * d), SENTINEL, device=device)
    K.gemm(p.to(device), _heads(kvd[..., h * d:], h), out=_heads(o, h), bf16_operands=one)
    _check(_form(terms), _heads(o, h), c64, s, C["zero_mean"], f"p v into a head view, head dim {d}")


# ---- GPU 4: the exact-f32 kernel -------------------------------------------------------------------------------------------
# PV_GEMM_EXACT_F32 is read per call, so monkeypatch can set it.  PV_GEMM_NO_ROWS_FORM is read ONCE per process and cannot be
# flipped in a test: the tiled kernels are reached for tall shapes through views the rows rule refuses (m = 2047, or an A whose
# base is one element off 16 bytes) -- TALL_TILED_SHAPES.
@pytest.mark.gpu
@pytest.mark.parametrize("case", _with_regimes(TILED_SHAPES + TALL_TILED_SHAPES), ids=_case_id)
def test_exact_f32_kernel_in_four_layouts(case, device, monkeypatch):
    """gemm_f32_kernel (v_mfma_f32_32x32x2_f32) within the same bound, and within the sum of both bounds of the default form."""
    K = _ops()
    (m, k, n), regime = case
    a, b, _, _ = _operands(m, k, n, regime)
    c64, s = _ref(a, b)
    views = [(ta, tb, _strided(a, device, off=1) if (m >= 2048 and not ta) else _dev(a, device, ta), _dev(b, device, tb))
             for ta in (False, True) for tb in (False, True)]
    default = [K.gemm(ad, bd).cpu() for _, _, ad, bd in views]
    monkeypatch.setenv("PV_GEMM_EXACT_F32", "1")
    exact = [K.gemm(ad, bd).cpu() for _, _, ad, bd in views]
    monkeypatch.delenv("PV_GEMM_EXACT_F32")
    for (ta, tb, _, _), x3, ex in zip(views, default, exact):
        _check("exact", ex, c64, s, C[regime], f"{_case_id(case)} A^T {ta} B^T {tb}")
        _check("tiled x3", x3, c64, s, C[regime], f"{_case_id(case)} A^T {ta} B^T {tb} (default)")
        bound = 2 * C[regime] * U32 * s + 1e-30
        assert float(((ex.double() - x3.double()).abs() / bound).max()) <= 1.0, "exact and three-term results further apart than both bounds"


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPILOGUES)
def test_exact_f32_kernel_epilogues(epi, device, monkeypatch):
    K = _ops()
    m, k, n = 129, 33, 65
    a, b, bias, res = _operands(m, k, n, "zero_mean")
    bc, rc, bd, rd, relu = _epilogue_args(epi, bias, res, device)
    c64, s = _ref(a, b, bc, rc, relu)
    monkeypatch.setenv("PV_GEMM_EXACT_F32", "1")
    got = K.gemm(a.to(device), _dev(b, device, True), bias=bd, relu=relu, residual=rd)
    big = torch.full((m, n + 5), SENTINEL, device=device)
    K.gemm(a.to(device), _dev(b, device, True), bias=bd, relu=relu, residual=rd, out=big[:, 3:3 + n])
    monkeypatch.delenv("PV_GEMM_EXACT_F32")
    _check("exact", got, c64, s, C["zero_mean"], f"{epi}")
    assert torch.equal(big[:, 3:3 + n], got) and bool((_bits(big[:, :3].cpu()) == _bits(torch.tensor([SENTINEL]))).all())
    assert bool((_bits(big[:, 3 + n:].cpu()) == _bits(torch.tensor([SENTINEL]))).all())


# ---- GPU 5: the rows form --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("k", ROWS_K)
def test_rows_form(k, terms, device):
    """gemm_rows_x3_kernel<KSTEPS, VEC, false, TERMS>: every m in ROWS_M (2047: the tiled kernel) x n in ROWS_N x B as w.t() and
    as its contiguous copy, both regimes; then A as wide[:, :K] of a K + 2 and a K + 1 columns wide matrix (VEC 2 / VEC 1 whatever
    K).  All are slices of one (2079, K, 72) product."""
    K = _ops()
    one = terms == 1
    for regime in REGIMES:
        a, b, _, _ = _operands(ROWS_M_MAX, k, ROWS_N_MAX, regime)
        c64, s = _ref(a, b, rounded=one)
        c32, s32 = _ref(a, b)
        ad, wd = a.to(device), b.t().contiguous().to(device)
        assert ad.data_ptr() % 16 == 0
        for m in ROWS_M:
            for n in ROWS_N:
                for contiguous in (False, True):
                    b_op = wd[:n].t().contiguous() if contiguous else wd[:n].t()
                    got = K.gemm(ad[:m], b_op, bf16_operands=one)
                    _check(_form(terms, m=m, k=k), got, c64[:m, :n], s[:m, :n], C[regime],
                           f"{m}x{k}x{n} {regime} B contiguous {contiguous}")
        if one:
            assert _ratio(got, c32[:m, :n], s32[:m, :n], C[regime]) > 1.0, "the one-term form gave the f32-accurate product"
        for pad in (2, 1):
            wide = _strided(a, device, ld_pad=pad)
            assert wide.data_ptr() % 16 == 0 and wide.stride(0) == k + pad
            for n in (72, 64):
                got = K.gemm(wide, wd[:n].t(), bf16_operands=one)
                _check(_form(terms, m=ROWS_M_MAX, k=k), got, c64[:, :n], s[:, :n], C[regime], f"A = wide[:, :{k}] of {k + pad} columns, n {n} {regime}")


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("case", _with_regimes(LOOP_SHAPES), ids=_case_id)
def test_rows_form_persistent_loop(case, terms, device):
    """(8229, K, 1024): 16 column blocks, per_col = 32, a stride of 128 row blocks over 258: waves 0 and 1 of each workgroup
    take three blocks (a second trip that leaves at the mid-trip break), the others two; the last block holds 5 rows."""
    K = _ops()
    (m, k, n), regime = case
    a, b, bias, _ = _operands(m, k, n, regime)
    c64, s = _ref(a, b, bias, rounded=terms == 1)
    got = K.gemm(a.to(device), _dev(b, device, True), bias=bias.to(device), bf16_operands=terms == 1)
    _check(_form(terms, m=m, k=k), got, c64, s, C[regime], _case_id(case))


# ---- GPU 6: the bf16-output rows form ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("k", ROWS_K)
def test_rows_form_bf16_output(k, terms, device):
    """gemm_rows_x3_kernel<KSTEPS, VEC, true, TERMS> through gemm_rows_bf16out: n = 64, 128 through the LDS tile, 72: block 0
    through the tile and block 1 lane by lane, 70: lane by lane (ldc & 7); bitwise the f32 result rounded."""
    K = _ops()
    one = terms == 1
    for regime in REGIMES:
        a, b, bias, _ = _operands(ROWS_M_MAX, k, BF16OUT_N[1], regime)
        c64, s = _ref(a, b, bias, rounded=one)
        ad, wd, bd = a.to(device), b.t().contiguous().to(device), bias.to(device)
        for m in BF16OUT_M:
            for n in BF16OUT_N:
                for contiguous in (False, True):
                    b_op = wd[:n].t().contiguous() if contiguous else wd[:n].t()
                    assert K.gemm_rows_bf16out_supported(ad[:m], b_op)
                    got = K.gemm_rows_bf16out(ad[:m], b_op, bias=bd[:n], bf16_operands=one)
                    assert got.dtype == torch.bfloat16
                    _check("bf16 output", got, c64[:m, :n], s[:m, :n], C[regime], f"{m}x{k}x{n} x{terms} {regime} B contiguous {contiguous}",
                           bf16_out=True)
                    assert torch.equal(got, K.gemm(ad[:m], b_op, bias=bd[:n], bf16_operands=one).to(torch.bfloat16))


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("k,n", [(64, 64), (38, 72), (37, 128)])
def test_rows_form_bf16_output_with_a_padded_leading_dimension(k, n, terms, device):
    """pv_gemm_rows_bf16out_f32 called as hip_ops.gemm_rows_bf16out calls it, but with ldc = n + 8 (the LDS-tile store with a
    stride) and ldc = n + 1 (lane by lane) into a sentinel-filled buffer."""
    K = _ops()
    m = 2079
    a, b, bias, _ = _operands(m, k, n, "zero_mean")
    c64, s = _ref(a, b, bias, rounded=terms == 1)
    ad, bd, biasd = a.to(device), _dev(b, device, True), bias.to(device)
    sent = torch.tensor([SENTINEL]).to(torch.bfloat16)
    for ldc in (n + 8, n + 1):
        buf = sent.to(device).repeat(m * ldc).view(m, ldc)
        d = K._lib.GemmDesc(m, n, k, ad.stride(0), ad.stride(1), bd.stride(0), bd.stride(1), ldc, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)
        K.check(K.get_lib().pv_gemm_rows_bf16out_f32(K.ptr(ad), K.ptr(bd), K.ptr(biasd), K.ptr(buf), ctypes.byref(d),
                                                     K.GEMM_BF16_OPERANDS if terms == 1 else 0, K.current_stream_ptr()),
                "pv_gemm_rows_bf16out_f32")
        _check("bf16 output", buf[:, :n], c64, s, C["zero_mean"], f"{m}x{k}x{n} x{terms} ldc {ldc}", bf16_out=True)
        assert bool((_bits(buf[:, n:].cpu()) == _bits(sent)).all()), "written outside the m x n view"


# ---- GPU 7: split-K --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", SPLITK_SHAPES + [(48, 100, 37)], ids=_shape_id)
def test_splitk(shape, form, device):
    """gemm_splitk: A row-major and as the .t() view a weight gradient passes, twice (equal bits), and accumulating.
    ((48, 100, 37) is one split: plain gemm, but still slab + sum_slabs when it accumulates.)"""
    K = _ops()
    m, k, n = shape
    assert (K.SPLITK_TARGET_WORKGROUPS, K.SPLITK_MIN_CHUNK) == (1024, 256)      # _splits restates them
    terms, a16 = FORMS[form]
    a, b, _, acc0 = _operands(m, k, n, "zero_mean")
    src = a.to(torch.bfloat16) if a16 else a
    c64, s = _ref(a, b, rounded=terms == 1)
    a64, as_ = _ref(a, b, acc=acc0, rounded=terms == 1)
    for ta in (False, True):
        ad, bd = _dev(src, device, ta), b.contiguous().to(device)
        got = K.gemm_splitk(ad, bd, bf16_operands=terms == 1)
        _check("split-K", got, c64, s, C["zero_mean"], f"{_shape_id(shape)} {form} A^T {ta}")
        assert torch.equal(got, K.gemm_splitk(ad, bd, bf16_operands=terms == 1)), "two calls differ"
        acc = acc0.to(device)
        ret = K.gemm_splitk(ad, bd, accumulate_into=acc, bf16_operands=terms == 1)
        assert ret is acc
        _check("split-K", acc, a64, as_, C["zero_mean"], f"{_shape_id(shape)} {form} A^T {ta} accumulate_into")


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("m,n", [(48, 37), (129, 65)])
def test_splitk_with_an_empty_split(m, n, terms, device):
    """pv_gemm_ex_f32 with k = 32, k_splits = 3: k_chunk = 16, the third split has kbeg = kend = 32 -- it loads nothing (both
    kernels guard their first load and their loop with kbeg < kend) and must store zeros."""
    K = _ops()
    k, splits = 32, 3
    assert _chunk(k, splits) == 16
    a, b, _, _ = _operands(m, k, n, "zero_mean")
    c64, s = _ref(a, b, rounded=terms == 1)
    ad, bd = a.to(device), b.contiguous().to(device)
    slabs = torch.full((splits, m, n), SENTINEL, device=device)
    d = K._lib.GemmDesc(m, n, k, ad.stride(0), ad.stride(1), bd.stride(0), bd.stride(1), n, 1, 1, 0, 0, 0, 0, 0, 0, splits, m * n)
    K.check(K.get_lib().pv_gemm_ex_f32(K.ptr(ad), K.ptr(bd), None, None, 0, K.ptr(slabs), ctypes.byref(d), 0,
                                       K.GEMM_BF16_OPERANDS if terms == 1 else 0, K.current_stream_ptr()), "pv_gemm_ex_f32")
    slabs = slabs.cpu()
    assert bool((_bits(slabs[2]) == 0).all()), "the empty split's slab is not +0"
    _check("split-K", (slabs[0] + slabs[1]) + slabs[2], c64, s, C["zero_mean"], f"{m}x{k}x{n} x{terms}, three slabs")


# ---- GPU 8: colsum ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=_shape_id)
def test_colsum(shape, regime, device):
    """colsum_partial_f32 + sum_slabs_f32: one chunk ... 512 chunks of 33 rows (16385) and of 137 (70001), and accumulating."""
    K = _ops()
    x, acc0 = _colsum_input(*shape, regime)
    c64, s = _colsum_ref(x)
    xd = x.to(device)
    _check("colsum", K.colsum(xd), c64, s, C_COLSUM[regime], f"{_shape_id(shape)} {regime}")
    a64, as_ = _colsum_ref(x, acc0)
    acc = acc0.to(device)
    assert K.colsum(xd, accumulate_into=acc) is acc
    _check("colsum", acc, a64, as_, C_COLSUM[regime], f"{_shape_id(shape)} {regime} accumulate_into")


# ---- the table in the module docstring -------------------------------------------------------------------------------------
def _measure():
    """Worst error / (2^-24 S) of the reference-only evaluations over every (shape, regime) of this file."""
    worst = {r: [0.0, 0.0] for r in REGIMES}

    def row(name, regime, torch32, emulation):
        worst[regime][0], worst[regime][1] = max(worst[regime][0], torch32), max(worst[regime][1], emulation)
        print(f"    {name:<34} float32 torch {torch32:6.2f}   emulation {emulation:6.2f}")

    for (m, k, n), regime in TABLE_CASES:
        a, b, bias, res = _operands(m, k, n, regime)
        c64, s = _ref(a, b)
        c16, s16 = _ref(a, b, rounded=True)
        row(f"{m}x{k}x{n} {regime} x3", regime, _ratio(a @ b, c64, s, 1.0), _ratio(_emulate(a, b), c64, s, 1.0))
        row(f"{m}x{k}x{n} {regime} x1", regime, _ratio(_bf16(a) @ _bf16(b), c16, s16, 1.0), _ratio(_emulate(a, b, terms=1), c16, s16, 1.0))
    for m, k, n in SPLITK_SHAPES:
        a, b, _, _ = _operands(m, k, n, "zero_mean")
        splits, _ = _splits(m, k, n)
        c64, s = _ref(a, b)
        c16, s16 = _ref(a, b, rounded=True)
        row(f"{m}x{k}x{n} split-K ({splits}) x3", "zero_mean", _ratio(a @ b, c64, s, 1.0), _ratio(_emulate_splitk(a, b, splits), c64, s, 1.0))
        row(f"{m}x{k}x{n} split-K ({splits}) x1", "zero_mean", _ratio(_bf16(a) @ _bf16(b), c16, s16, 1.0),
            _ratio(_emulate_splitk(a, b, splits, terms=1), c16, s16, 1.0))
    for regime in REGIMES:
        print(f"worst {regime}: float32 torch {worst[regime][0]:.2f}, emulation {worst[regime][1]:.2f} -> c = {4 * max(worst[regime]):.1f}")
    cs = {r: 0.0 for r in REGIMES}
    for shape in COLSUM_SHAPES:
        for regime in REGIMES:
            x, _ = _colsum_input(*shape, regime)
            c64, s = _colsum_ref(x)
            r = (_ratio(x.sum(0), c64, s, 1.0), _ratio(_colsum_row_order(x), c64, s, 1.0), _ratio(_emulate_colsum(x), c64, s, 1.0))
            cs[regime] = max(cs[regime], *r)
            print(f"    colsum {_shape_id(shape)} {regime:<10} float32 torch {r[0]:6.2f}   row order {r[1]:6.2f}   emulation {r[2]:6.2f}")
    for regime in REGIMES:
        print(f"worst colsum {regime}: {cs[regime]:.2f} -> c = {4 * cs[regime]:.1f}")


if __name__ == "__main__":
    _measure()
