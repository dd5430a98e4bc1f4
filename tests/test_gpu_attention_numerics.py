"""The fused attention kernels (pv_attention_{fwd,bwd}_f32, pv_attention_{fwd,bwd}_bf16, ..._bf16kv, pv_attention_bwd_bf16kv16),
the unfused route of perceiver_functional.attention_core and softmax_{fwd,bwd}_f32, per element against a float64 restatement,
in the numeric regimes where an online softmax, a split merge or a log-sum-exp goes wrong -- and CPU tests that show the checker
itself rejects such mistakes.

Reference.  `_reference`: softmax(scale q k^T) v per head from the [b, n, h*64] / [b, n, 2*h*64] layout in float64 on the CPU:
out, lse, and dq / dkv by autograd.  For the bf16-operand kernels q, k, v and dO are rounded to bf16 (nearest even) first; the
probabilities are never rounded in the reference (where P is rounded is an implementation's choice: it belongs in the bound).

Bounds, per element, never a norm.  With u = 2^-24, A_i = max_j scale sum_d |q_id k_jd| (a score's rounding error is a RELATIVE
error of its probability) and every quantity taken from the float64 reference:
    out   c_out u (1 + A_i) sum_j p_ij |v_jd|
    lse   c_lse u (1 + A_i + |lse_i|)
    dv    c_dv  u sum_i (1 + A_i) p_ij |dO_id|
    dq    c_dq  u (1 + A_i) scale sum_j w_ij |k_jd|         w_ij = p_ij (sum_d |dO_id v_jd| + sum_d |dO_id| sum_j p_ij |v_jd|)
    dk    c_dk  u scale sum_i (1 + A_i) w_ij |q_id|
(w bounds |dS_ij| / scale = p_ij |dP_ij - delta_i| with dP and delta replaced by THEIR sums of absolute products: both are
cancelling sums of 64 products whose rounding error is relative to those, and near a one-hot row dP_ij - delta_i cancels almost
entirely.)  The bf16-operand kernels get, on top, one bf16 rounding (2^-9) of every probability / dS as it becomes a matrix
operand: c16 2^-9 times the same sums without the (1 + A_i) factor; their lse keeps the f32 bound (the softmax statistics
are f32).  Every bound carries a floor of 2^-126 (smallest normal float32: a probability that underflows is flushed to zero) times
the number of terms times the largest absolute operands, which matters only for keys that carry no mass at all.

Constants.  They come from the REFERENCE's own error, not from the kernels: the same formula evaluated with plain torch on the
CPU in float32 (for the bf16 term: in float64 with P rounded to bf16 after normalisation and dS rounded to bf16), worst
error / bound-with-c=1 over every (shape, regime) of CASES below; the kernels get 4x that (another summation order, v_exp_f32
instead of libm, P rounded before instead of after normalisation).  `python tests/test_gpu_attention_numerics.py` prints
the table these were read from:
                 out    lse    dq     dk     dv
    float32     19.7   2.58   9.68   1.77   5.51     (out, dq: `equal` at 1025 and 16 384 keys, where the rounding errors of identical
    bf16 P/dS   1.90    -     0.60   1.04   1.99      addends do not cancel -- every other regime stays below 4.6 and 0.84;
    c           79.0   10.4   38.8   7.10   22.1      lse, dk, dv: `peaked` at (128, 8, 16, 600))
    c16         7.60    -     2.42   4.15   7.97     (2^-9 is half a bf16 rounding step at the top of a binade, a quarter at its
                                                      bottom: a single rounding reaches 2.0 of it)
softmax_scaled_: |p - p64| <= c u (1 + max_j |scale x_j|) p64 + 2^-126; float32 torch reaches 1.71, c = 6.83.  Its backward:
|dx - dx64| <= c u (1 + max_j |scale x_j|) scale p64_i (|dp_i| + sum_j |dp_j| p64_j) (+ floor); float32 torch 1.56, c = 6.23.
Measured on the MI355X with these constants (worst error / bound over all cases): f32 kernels out 0.22, lse 0.65, dq 0.06,
dk 0.26, dv 0.31; bf16-operand kernels out 0.25, lse 0.23, dq 0.25, dk 0.24, dv 0.25; attention_core 0.24; softmax_scaled_ 0.24:
every kernel stays within 2.6x the float32 torch evaluation's own error.  The GPU cases of this file take 22 s together.

Regimes (seeded, built on the CPU; `_assert_regime` asserts each one's condition on the float64 reference before the kernel
is looked at; conditions that need room -- a maximum below 0.1 -- are asserted from 513 keys on):
    flat        randn, q * 0.75, scale 0.125               max p of every row < 0.1
                (plain randn reaches 0.12 at (3, 2, 97, 513) and 0.19 among the 16 384 rows of (128, 8, 16, 600))
    peaked      q * 8                                      median over rows of max p > 0.5
    shifted     + 80 on every key component                rows with max s > 100 and with max s < -100; p == p of the same keys less 80
                (the 40 first thought of gives one such row in 128 on average: the condition failed at the 128-query shapes)
    late_peak   last key = 40 e_0, q_0 = 4                 arg max is the last key in > 90 % of the rows, p there > 0.5
    early_peak  the same for key 0                         as above for key 0
    one_split   k_0 = 160 inside one split's key range,    the other keys' mass is 0 in float32 (scores trail by > 104 = 149 ln 2),
                0 outside, q_0 = 8                         the range sums to 1
    tiny        q * 1e-4                                   all p within 1e-3 relative of 1 / n_k, |lse - log n_k| < 1e-3
                (q * 1e-3 leaves deviations of 4.5e-3: the construction was tightened, not the condition)
    equal       all keys and values identical, q and k     p == 1 / n_k exactly, |dq| < 1e-12
                bf16-representable (scores exact in float64 in any summation order)

Shapes (batch, heads, n_q, n_k), with the split geometry from the sources (T = ceil(n_k / 32) key tiles):
  forward bf16 (attn_fwd_splits): s = min(ceil(768 / (b h ceil(n_q / 128))), T / 16), tiles per split = ceil(T / s);
  backward f32 (attn_bwd_splits): s = min(ceil(1024 / (b h)), T / 8); backward bf16: s = min(768 / (b h), T / 8); both: tiles per
  split = ceil(T / s) rounded up to 4; the f32 forward never splits.
    (2, 2, 40, 70) (1, 1, 1, 1) (1, 1, 128, 1) (1, 1, 1, 33)      no split anywhere, ragged tiles
    (., ., ., 513)    T = 17: backward 2 splits of 12 + 5 tiles, key 512 alone in the last tile; forward unsplit
    (., ., ., 1025)   T = 33: forward 2 splits of 17 + 16 tiles, backward 3 splits of 12 + 12 + 9; key 1024 alone in the last tile
    (2, 1, 128, 16384)   T = 512: forward 32 splits of 16 tiles, backward 64 splits of 8
    (1, 1, 100, 2100)    T = 66: forward 4 splits of 17, 17, 17, 15 tiles, backward 6 splits of 12 (last: 6), 20 keys in the last tile
    (128, 8, 16, 600)    1024 groups: forward 1 split, backward f32 ceil(1024 / 1024) = 1, bf16 768 / 1024 = 0 -> 1: 19 tiles unsplit
    (1, 2, 130, 2100) (1, 1, 257, 33)   forward only (more than 128 queries): 2 / 3 query blocks; 4 splits / none
"""
import math

import pytest
import torch

HD = 64
SCALE = 0.125
U32 = 2.0 ** -24
U16 = 2.0 ** -9
TINY = 2.0 ** -126
SHIFT = 80.0
FLAT = 0.75

# 4 x the reference-only ratios of the module docstring
C_F32 = {"out": 79.0, "lse": 10.4, "dq": 38.8, "dk": 7.10, "dv": 22.1}
C_B16 = {"out": 7.60, "dq": 2.42, "dk": 4.15, "dv": 7.97}
C_SOFTMAX, C_SOFTMAX_BWD = 6.83, 6.23

REGIMES = ("flat", "peaked", "shifted", "late_peak", "early_peak", "one_split", "tiny", "equal")
EVERY_REGIME_SHAPES = [(1, 1, 128, 513), (3, 2, 97, 513), (1, 1, 128, 1025), (3, 2, 97, 1025), (2, 1, 128, 16384)]
FLAT_PEAKED_SHAPES = [(2, 2, 40, 70), (1, 1, 1, 1), (1, 1, 128, 1), (1, 1, 1, 33), (1, 1, 100, 2100), (128, 8, 16, 600),
                      (1, 2, 130, 2100), (1, 1, 257, 33)]
CASES = ([(s, r) for s in EVERY_REGIME_SHAPES for r in REGIMES] + [(s, r) for s in FLAT_PEAKED_SHAPES for r in ("flat", "peaked")])
# the key range of ONE split that holds all the mass in `one_split`: the backward's last split at 513 keys (with the lone key
# of the ragged tile), the forward's second split at 1025, the forward's second split (= two backward splits) at 16384
SPLIT_RANGE = {513: (384, 513), 1025: (544, 1025), 16384: (512, 1024)}


def _case_id(case):
    (b, h, nq, nk), regime = case
    return f"{b}x{h}x{nq}x{nk}-{regime}"


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _inputs(shape, regime):
    """q [b, nq, h*64], kv [b, nk, 2*h*64] (k | v), dout like q: float32 on the CPU.  The draws depend on the shape alone, so
    every regime is a stated change of `flat`'s tensors."""
    b, h, nq, nk = shape
    g = torch.Generator().manual_seed(1000003 * b + 10007 * h + 101 * nq + nk)
    q = torch.randn(b, nq, h * HD, generator=g)
    kv = torch.randn(b, nk, 2 * h * HD, generator=g)
    dout = torch.randn(b, nq, h * HD, generator=g)
    k = kv[..., :h * HD].view(b, nk, h, HD)      # views: written through below
    q0 = q.view(b, nq, h, HD)[..., 0]
    if regime == "peaked":
        q *= 8
        return q, kv, dout
    q *= FLAT           # every other regime is a change of `flat`
    if regime == "flat":
        pass
    elif regime == "shifted":
        k += SHIFT
    elif regime in ("late_peak", "early_peak"):
        j = nk - 1 if regime == "late_peak" else 0
        q0.fill_(4.0)
        k[:, j] = 0.0
        k[:, j, :, 0] = 40.0                      # its score is 0.125 * 4 * 40 = 20, every other key's about N(0, 0.9)
    elif regime == "one_split":
        lo, hi = SPLIT_RANGE.get(nk, (nk - (nk + 2) // 3, nk))
        q0.fill_(8.0)
        k[..., 0] = 0.0
        k[:, lo:hi, :, 0] = 160.0                 # 0.125 * 8 * 160 = 160 ahead of the rest, whose scores are about N(0, 1)
    elif regime == "tiny":
        q *= 1e-4 / FLAT
    elif regime == "equal":
        # bf16-representable q and k: every product and every partial sum of a score is exact in float64 in ANY summation
        # order, so the reference's scores of identical keys are identical bits whatever its matrix product does
        q, kv = _bf16(q), _bf16(kv)
        kv[:] = kv[:, :1].clone()
    else:
        raise ValueError(regime)
    return q, kv, dout


def _unshifted(shape):
    """`shifted`'s inputs with the constant taken off its float32 keys again in float64 (k + 80 is rounded to float32, so these are
    flat's keys moved by up to 2^-18): the inputs whose probabilities `shifted` must reproduce."""
    q, kv, dout = _inputs(shape, "shifted")
    kv = kv.double()
    kv[..., :shape[1] * HD] -= SHIFT
    return q, kv, dout


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)      # nearest even


# ---- float64 reference -----------------------------------------------------------------------------------------------------
def _heads(t, h):
    b, n, c = t.shape
    return t.view(b, n, h, c // h).permute(0, 2, 1, 3)


def _flat(t):
    b, h, n, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, n, h * hd)


class _Ref:
    pass


def _reference(q, kv, dout, h, scale, round_bf16=False, backward=True):
    """float64 restatement and the sums of absolute products its bounds are made of (all in the kernels' layouts)."""
    if round_bf16:
        q, kv, dout = _bf16(q), _bf16(kv), _bf16(dout)
    b, nq, inner = q.shape
    nk = kv.shape[1]
    q64 = q.detach().double().requires_grad_(backward)
    kv64 = kv.detach().double().requires_grad_(backward)
    do64 = dout.double()
    qh, kh, vh = _heads(q64, h), _heads(kv64[..., :inner], h), _heads(kv64[..., inner:], h)
    s = (qh @ kh.transpose(-1, -2)) * scale
    p = s.softmax(dim=-1)
    out = _flat(p @ vh)
    r = _Ref()
    r.shape, r.scale = (b, h, nq, nk), scale
    r.out, r.lse, r.p, r.smax = out.detach(), torch.logsumexp(s, dim=-1).detach(), p.detach(), s.detach().amax(dim=-1)
    if backward:
        out.backward(do64)
        r.dq, r.dkv = q64.grad, kv64.grad
    with torch.no_grad():
        qa, ka, va, da = qh.abs(), kh.abs(), vh.abs(), _heads(do64, h).abs()
        r.A = scale * (qa @ ka.transpose(-1, -2)).amax(dim=-1)                  # [b, h, nq]
        r.one_A = _flat((1.0 + r.A)[..., None].expand(b, h, nq, inner // h))            # (1 + A_i) in q's layout
        r.out_abs = _flat(r.p @ va)
        r.out_floor = TINY * nk * float(va.max())
        if backward:
            w = r.p * (da @ va.transpose(-1, -2) + (da * (r.p @ va)).sum(-1, keepdim=True))      # >= |dS| / scale
            wA = w * (1.0 + r.A)[..., None]
            r.dq_abs = _flat(scale * (w @ ka))
            r.dkv_abs = torch.cat([_flat(scale * (w.transpose(-1, -2) @ qa)), _flat(r.p.transpose(-1, -2) @ da)], dim=-1)
            r.dkv_abs_A = torch.cat([_flat(scale * (wA.transpose(-1, -2) @ qa)),
                                     _flat((r.p * (1.0 + r.A)[..., None]).transpose(-1, -2) @ da)], dim=-1)
            wmax = float((da @ va.transpose(-1, -2)).max() + (da * (r.p @ va)).sum(-1).max())
            r.dq_floor = TINY * scale * nk * wmax * float(ka.max())
            r.dk_floor = TINY * scale * nq * wmax * float(qa.max())
            r.dv_floor = TINY * nq * float(da.max())
    return r


def _assert_regime(regime, r, flat=None):
    """The regime's stated condition, on the float64 reference."""
    b, h, nq, nk = r.shape
    pmax, arg = r.p.max(dim=-1)
    if regime == "flat":
        if nk >= 513:
            assert float(pmax.max()) < 0.1, f"flat: max p {float(pmax.max())}"
    elif regime == "peaked":
        assert float(pmax.median()) > 0.5, f"peaked: median of max p {float(pmax.median())}"
    elif regime == "shifted":
        assert int((r.smax > 100).sum()) > 0 and int((r.smax < -100).sum()) > 0, "shifted: no row with max s beyond +-100"
        if flat is not None:
            assert float((r.p - flat.p).abs().max()) < 1e-12 and float(((r.p - flat.p).abs() / flat.p).max()) < 1e-9
            assert float(flat.p.max()) < 0.1 and float(flat.smax.abs().max()) < 10      # and those are flat
    elif regime in ("late_peak", "early_peak"):
        j = nk - 1 if regime == "late_peak" else 0
        assert float((arg == j).double().mean()) > 0.9 and float(r.p[..., j].median()) > 0.5, f"{regime}: key {j} does not win"
    elif regime == "one_split":
        lo, hi = SPLIT_RANGE.get(nk, (nk - (nk + 2) // 3, nk))
        inside = r.p[..., lo:hi].sum(-1)
        outside = torch.cat([r.p[..., :lo], r.p[..., hi:]], dim=-1)
        assert float((inside - 1.0).abs().max()) < 1e-12, "one_split: the range does not hold the row's mass"
        assert float(outside.max()) < math.exp(-104.0) and float(outside.float().max()) == 0.0, "one_split: mass outside"
    elif regime == "tiny":
        assert float((r.p * nk - 1.0).abs().max()) < 1e-3 and float((r.lse - math.log(nk)).abs().max()) < 1e-3
    elif regime == "equal":
        assert bool((r.p == 1.0 / nk).all()), "equal: p is not 1 / n_k"
        if hasattr(r, "dq"):
            assert float(r.dq.abs().max()) < 1e-12, f"equal: dq {float(r.dq.abs().max())}"


# ---- the checker -----------------------------------------------------------------------------------------------------------
def _worst(got, ref64, bound):
    got = got.detach().double().cpu()
    ratio = (got - ref64).abs() / bound
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def _bounds(r, c32, c16=None):
    """name -> per-element bound; c16 None: f32 kernels."""
    inner = r.out.shape[-1]
    bd = {"out": c32["out"] * U32 * r.one_A * r.out_abs + r.out_floor,
          "lse": c32["lse"] * U32 * (1.0 + r.A + r.lse.abs())}
    if hasattr(r, "dq"):
        floor = torch.cat([torch.full((inner,), r.dk_floor), torch.full((inner,), r.dv_floor)]).double()
        ckv = torch.cat([torch.full((inner,), c32["dk"]), torch.full((inner,), c32["dv"])]).double()
        bd["dq"] = c32["dq"] * U32 * r.one_A * r.dq_abs + r.dq_floor
        bd["dkv"] = ckv * U32 * r.dkv_abs_A + floor
    if c16 is not None:
        bd["out"] = bd["out"] + c16["out"] * U16 * r.out_abs
        if hasattr(r, "dq"):
            ckv16 = torch.cat([torch.full((inner,), c16["dk"]), torch.full((inner,), c16["dv"])]).double()
            bd["dq"] = bd["dq"] + c16["dq"] * U16 * r.dq_abs
            bd["dkv"] = bd["dkv"] + ckv16 * U16 * r.dkv_abs
    return bd


def _attention_ratios(r, out, lse, dq=None, dkv=None, bf16=False):
    """Worst error / bound per tensor (a non-finite result counts as infinite)."""
    bd = _bounds(r, C_F32, C_B16 if bf16 else None)
    ratios = {"out": _worst(out, r.out, bd["out"]), "lse": _worst(lse, r.lse, bd["lse"])}
    if dq is not None:
        inner = r.out.shape[-1]
        ratios["dq"] = _worst(dq, r.dq, bd["dq"])
        ratios["dk"] = _worst(dkv[..., :inner], r.dkv[..., :inner], bd["dkv"][..., :inner])
        ratios["dv"] = _worst(dkv[..., inner:], r.dkv[..., inner:], bd["dkv"][..., inner:])
    return ratios


def _check_attention(r, out, lse, dq=None, dkv=None, bf16=False, what=""):
    ratios = _attention_ratios(r, out, lse, dq, dkv, bf16)
    print(f"{what}: error / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: error beyond the per-element bound, worst error / bound: {bad}"


# ---- plain-torch restatements: the correct one the constants are measured with, and four wrong ones -----------------------
def _torch_attention(q, kv, h, scale, dtype=torch.float32, dout=None):
    """softmax(scale q k^T) v with torch ops in `dtype`; with dout: (out, lse, dq, dkv) through autograd."""
    inner = q.shape[-1]
    q_, kv_ = q.detach().to(dtype, copy=True).requires_grad_(dout is not None), kv.detach().to(dtype, copy=True).requires_grad_(dout is not None)
    s = (_heads(q_, h) @ _heads(kv_[..., :inner], h).transpose(-1, -2)) * scale
    out = _flat(s.softmax(dim=-1) @ _heads(kv_[..., inner:], h))
    lse = torch.logsumexp(s, dim=-1)
    if dout is None:
        return out.detach(), lse.detach()
    out.backward(dout.to(dtype))
    return out.detach(), lse.detach(), q_.grad, kv_.grad


def _scores(q, kv, h, scale):
    inner = q.shape[-1]
    return (_heads(q, h) @ _heads(kv[..., :inner], h).transpose(-1, -2)) * scale, _heads(kv[..., inner:], h)


def _wrong_no_max(q, kv, h, scale):
    """float32 softmax without any maximum subtraction."""
    s, v = _scores(q, kv, h, scale)
    e = s.exp()
    l = e.sum(-1, keepdim=True)
    return _flat((e / l) @ v), l.squeeze(-1).log()


def _wrong_no_rescale(q, kv, h, scale, tile=32):
    """online softmax in key tiles of 32 whose accumulator is NOT rescaled when the running maximum rises (the sum is)."""
    s, v = _scores(q, kv, h, scale)
    m = torch.full(s.shape[:-1], -float("inf"))
    l = torch.zeros(s.shape[:-1])
    acc = torch.zeros(s.shape[:-1] + (v.shape[-1],))
    for j0 in range(0, s.shape[-1], tile):
        st = s[..., j0:j0 + tile]
        m_new = torch.maximum(m, st.amax(-1))
        e = (st - m_new[..., None]).exp()
        l = l * (m - m_new).exp() + e.sum(-1)
        acc = acc + e @ v[..., j0:j0 + tile, :]          # correct: acc * exp(m - m_new)[..., None] + ...
        m = m_new
    return _flat(acc / l[..., None]), m + l.log()


def _wrong_merge(q, kv, h, scale, bounds):
    """key splits merged from their unnormalised accumulators and sums WITHOUT their maxima."""
    s, v = _scores(q, kv, h, scale)
    acc, l, m_all = 0.0, 0.0, None
    for lo, hi in bounds:
        st = s[..., lo:hi]
        m = st.amax(-1, keepdim=True)
        e = (st - m).exp()
        acc, l = acc + e @ v[..., lo:hi, :], l + e.sum(-1, keepdim=True)      # correct: each weighted by exp(m - max m)
        m_all = m if m_all is None else torch.maximum(m_all, m)
    return _flat(acc / l), (m_all + l.log()).squeeze(-1)


def _wrong_drop_last(q, kv, h, scale, dout):
    """the last key never takes part: its dk / dv rows stay zero."""
    out, lse, dq, dkv = _torch_attention(q, kv[:, :-1].contiguous(), h, scale, dout=dout)
    return out, lse, dq, torch.cat([dkv, torch.zeros_like(dkv[:, :1])], dim=1)


def _bf16_p_attention(r, q, kv, dout, h, scale):
    """float64 on the rounded operands with P rounded to bf16 AFTER normalisation and dS rounded to bf16 (the other place an
    implementation may round them): what the c16 constants are measured with."""
    inner = q.shape[-1]
    q, kv, dout = _bf16(q).double(), _bf16(kv).double(), _bf16(dout).double()
    qh, kh, vh, dh = _heads(q, h), _heads(kv[..., :inner], h), _heads(kv[..., inner:], h), _heads(dout, h)
    p = ((qh @ kh.transpose(-1, -2)) * scale).softmax(dim=-1)
    pr = _bf16(p)
    oh = pr @ vh
    ds = _bf16(scale * p * (dh @ vh.transpose(-1, -2) - (dh * oh).sum(-1, keepdim=True)))
    return _flat(oh), r.lse, _flat(ds @ kh), torch.cat([_flat(ds.transpose(-1, -2) @ qh), _flat(pr.transpose(-1, -2) @ dh)], dim=-1)


# ---- CPU: the checker itself -----------------------------------------------------------------------------------------------
CPU_SHAPE = (1, 1, 128, 513)


@pytest.mark.parametrize("regime", REGIMES)
def test_checker_accepts_float32_torch_in_every_regime(regime):
    q, kv, dout = _inputs(CPU_SHAPE, regime)
    r = _reference(q, kv, dout, 1, SCALE)
    flat = _reference(*_unshifted(CPU_SHAPE), 1, SCALE, backward=False) if regime == "shifted" else None
    _assert_regime(regime, r, flat)
    _check_attention(r, *_torch_attention(q, kv, 1, SCALE, dout=dout), what=f"float32 torch, {regime}")
    # and the bf16-operand bound holds the other rounding place of P / dS
    r16 = _reference(q, kv, dout, 1, SCALE, round_bf16=True)
    _check_attention(r16, *_bf16_p_attention(r16, q, kv, dout, 1, SCALE), bf16=True, what=f"bf16 P after normalisation, {regime}")


def test_checker_rejects_a_softmax_without_maximum_subtraction_only_off_the_flat_regime():
    q, kv, dout = _inputs(CPU_SHAPE, "flat")
    _check_attention(_reference(q, kv, dout, 1, SCALE, backward=False), *_wrong_no_max(q, kv, 1, SCALE), what="no maximum, flat")
    q, kv, dout = _inputs(CPU_SHAPE, "shifted")
    with pytest.raises(AssertionError, match="beyond the per-element bound"):
        _check_attention(_reference(q, kv, dout, 1, SCALE, backward=False), *_wrong_no_max(q, kv, 1, SCALE), what="no maximum, shifted")


def test_checker_rejects_an_accumulator_that_is_not_rescaled():
    q, kv, dout = _inputs(CPU_SHAPE, "late_peak")
    r = _reference(q, kv, dout, 1, SCALE, backward=False)
    _assert_regime("late_peak", r)
    with pytest.raises(AssertionError, match="beyond the per-element bound"):
        _check_attention(r, *_wrong_no_rescale(q, kv, 1, SCALE), what="no rescale, late peak")


def test_checker_rejects_a_split_merge_without_the_maxima():
    q, kv, dout = _inputs(CPU_SHAPE, "one_split")
    r = _reference(q, kv, dout, 1, SCALE, backward=False)
    _assert_regime("one_split", r)
    with pytest.raises(AssertionError, match="beyond the per-element bound"):
        _check_attention(r, *_wrong_merge(q, kv, 1, SCALE, [(0, 384), (384, 513)]), what="merge without maxima, one split")


def test_checker_rejects_a_dropped_last_key_that_a_norm_check_lets_through():
    q, kv, dout = _inputs(CPU_SHAPE, "late_peak")
    r = _reference(q, kv, dout, 1, SCALE)
    with pytest.raises(AssertionError, match="beyond the per-element bound"):
        _check_attention(r, *_wrong_drop_last(q, kv, 1, SCALE, dout), what="last key dropped, late peak")
    # flat, 16 384 keys: one key's wholly wrong dk / dv rows move the relative norm by 1 / sqrt(16384) = 7.8e-3, inside the
    # 1.5e-2 a norm check of the bf16 backward allows; per element they are caught
    shape = (1, 1, 128, 16384)
    q, kv, dout = _inputs(shape, "flat")
    r = _reference(q, kv, dout, 1, SCALE)
    out, lse, dq, dkv = _wrong_drop_last(q, kv, 1, SCALE, dout)
    assert float((dkv.double() - r.dkv).norm() / r.dkv.norm()) < 1.5e-2
    ratios = _attention_ratios(r, out, lse, dq, dkv)
    assert ratios["dk"] > 1.0 and ratios["dv"] > 1.0 and ratios["out"] > 1.0, ratios
    assert _attention_ratios(r, out, lse, dq, dkv, bf16=True)["dv"] > 1.0


# ---- GPU: the fused kernels ------------------------------------------------------------------------------------------------
def _mods():
    from predict_pv_yield_amd import hip_ops as K
    from predict_pv_yield_amd import perceiver_functional as PF
    return K, PF


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_attention_f32_kernels_per_element(case, device):
    """pv_attention_fwd_f32 / pv_attention_bwd_f32 against float64."""
    K, _ = _mods()
    shape, regime = case
    b, h, nq, nk = shape
    q, kv, dout = _inputs(shape, regime)
    backward = nq <= 128
    r = _reference(q, kv, dout, h, SCALE, backward=backward)
    flat = _reference(*_unshifted(shape), h, SCALE, backward=False) if regime == "shifted" else None
    _assert_regime(regime, r, flat)
    qd, kvd, dd = q.to(device), kv.to(device), dout.to(device)
    out, lse = K.attention_fwd(qd, kvd, h, SCALE)
    if not backward:
        _check_attention(r, out, lse, what=f"f32 forward {_case_id(case)}")
        return
    dq, dkv = K.attention_bwd(qd, kvd, out, dd, lse, h, SCALE)
    _check_attention(r, out, lse, dq, dkv, what=f"f32 {_case_id(case)}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_attention_bf16_kernels_per_element(case, device):
    """pv_attention_{fwd,bwd}_bf16 against float64 on the bf16-rounded operands, and the bit identities of the other entry points:
    K / V stored as bf16 (the roundings the f32-K/V kernels make on the way in), dkv stored as bf16 (the f32 dkv rounded),
    accumulate_dkv_into (one float32 addition per element)."""
    K, _ = _mods()
    shape, regime = case
    b, h, nq, nk = shape
    q, kv, dout = _inputs(shape, regime)
    backward = nq <= 128
    r = _reference(q, kv, dout, h, SCALE, round_bf16=True, backward=backward)
    if regime != "shifted":      # (the rounded keys of `shifted` are no longer flat's keys plus a constant: asserted in the f32 test)
        _assert_regime(regime, r)
    qd, kvd, dd = q.to(device), kv.to(device), dout.to(device)
    kv16 = kvd.to(torch.bfloat16)
    out, lse = K.attention_fwd(qd, kvd, h, SCALE, bf16_operands=True)
    out16, lse16 = K.attention_fwd(qd, kv16, h, SCALE, bf16_operands=True)
    assert torch.equal(out, out16) and torch.equal(lse, lse16), "bf16-stored K / V: forward differs"
    if not backward:
        _check_attention(r, out, lse, bf16=True, what=f"bf16 forward {_case_id(case)}")
        return
    dq, dkv = K.attention_bwd(qd, kvd, out, dd, lse, h, SCALE, bf16_operands=True)
    dq16, dkv16 = K.attention_bwd(qd, kv16, out, dd, lse, h, SCALE, bf16_operands=True)
    assert dkv16.dtype == torch.float32 and torch.equal(dq, dq16) and torch.equal(dkv, dkv16), "bf16-stored K / V: backward differs"
    dqb, dkvb = K.attention_bwd(qd, kv16, out, dd, lse, h, SCALE, bf16_operands=True, dkv_bf16=True)
    assert dkvb.dtype == torch.bfloat16 and torch.equal(dq, dqb) and torch.equal(dkvb, dkv.to(torch.bfloat16)), "bf16-stored dkv"
    start = torch.randn(kv.shape, generator=torch.Generator().manual_seed(nk)).to(device)
    acc = start.clone()
    dqa, ret = K.attention_bwd(qd, kv16, out, dd, lse, h, SCALE, bf16_operands=True, accumulate_dkv_into=acc)
    assert ret is acc and torch.equal(dq, dqa) and torch.equal(acc, start + dkv), "accumulate_dkv_into"
    _check_attention(r, out, lse, dq, dkv, bf16=True, what=f"bf16 {_case_id(case)}")


# ---- GPU: attention_core through autograd (fused and unfused routes) -----------------------------------------------------
def _core_inputs(shape, hd, regime):
    """As _inputs for a head dimension hd: q [b, nq, h*hd], kv [b, nk, 2*h*hd]; scale hd^-0.5."""
    b, h, nq, nk = shape
    g = torch.Generator().manual_seed(7 * nq + nk + hd)
    q = torch.randn(b, nq, h * hd, generator=g)
    kv = torch.randn(b, nk, 2 * h * hd, generator=g)
    dout = torch.randn(b, nq, h * hd, generator=g)
    if regime == "peaked":
        q *= 8
    else:
        q *= FLAT
    if regime == "shifted":
        kv[..., :h * hd] += SHIFT * (HD / hd) ** 0.5      # the same spread of row shifts at any head dimension
    return q, kv, dout


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["flat", "peaked", "shifted"])
@pytest.mark.parametrize("shape,hd,bf16", [((2, 2, 128, 600), 64, False), ((2, 2, 128, 600), 64, True), ((2, 2, 130, 600), 64, False),
                                           ((2, 4, 100, 600), 32, False)],
                         ids=["fused-f32", "fused-bf16", "unfused-130-queries", "unfused-head-dim-32"])
def test_attention_core_through_autograd(shape, hd, bf16, regime, device):
    """perceiver_functional.attention_core end to end: the fused kernels (<= 128 queries of head dimension 64) and the unfused
    route (gemm, softmax_fwd_f32 in place, gemm; softmax_bwd_f32 in the backward) against the same float64 reference and bounds."""
    _, PF = _mods()
    b, h, nq, nk = shape
    scale = hd ** -0.5
    q, kv, dout = _core_inputs(shape, hd, regime)
    r = _reference(q, kv, dout, h, scale, round_bf16=bf16)
    if regime == "flat":
        assert float(r.p.max()) < 0.1
    elif regime == "peaked":
        assert float(r.p.amax(-1).median()) > 0.5
    else:
        assert int((r.smax > 100).sum()) > 0 and int((r.smax < -100).sum()) > 0
    qd, kvd = q.to(device).requires_grad_(True), kv.to(device).requires_grad_(True)
    out = PF.attention_core(qd, kvd, h, scale, bf16_operands=bf16)
    out.backward(dout.to(device))
    # (attention_core does not return its log-sum-exp: the reference's own stands in, so only out / dq / dkv are judged)
    _check_attention(r, out, r.lse, qd.grad, kvd.grad, bf16=bf16, what=f"attention_core {shape} hd {hd} bf16 {bf16} {regime}")


# ---- GPU: softmax_scaled_ --------------------------------------------------------------------------------------------------
def _softmax_rows(n, regime):
    rows = 6
    g = torch.Generator().manual_seed(n)
    x = torch.randn(rows, n, generator=g) * 8          # scale 0.125: logits of sigma 1
    dy = torch.randn(rows, n, generator=g)
    if regime == "peaked":
        x *= 12                                        # (sigma 8 leaves the median of max p at 0.49 in rows of 5000)
    elif regime == "shifted":
        x += torch.tensor([200.0, -200.0] * (rows // 2))[:, None] / SCALE
    elif regime == "one_hot":
        hot = torch.tensor([n - 1, 0, n // 2, n - 1, 0, n // 3])
        x[torch.arange(rows), hot] = x.amax(-1) + 60.0 / SCALE        # leads by 60: the rest is about e^-60, a normal float32
    return x, dy


def _softmax_reference(x, dy):
    x64 = x.double()
    p = (x64 * SCALE).softmax(dim=-1)
    dx = SCALE * p * (dy.double() - (dy.double() * p).sum(-1, keepdim=True))
    amp = U32 * (1.0 + (x64 * SCALE).abs().amax(-1, keepdim=True))
    b_p = amp * p
    b_dx = amp * SCALE * p * (dy.double().abs() + (dy.double().abs() * p).sum(-1, keepdim=True))
    return p, dx, b_p, b_dx


def _assert_softmax_regime(regime, x, p):
    if regime == "peaked":
        assert float(p.amax(-1).median()) > 0.5
    elif regime == "shifted":
        s = x.double() * SCALE
        assert float(s.amax(-1).max()) > 100 and float(s.amax(-1).min()) < -100
    elif regime == "one_hot":
        assert float(p.amax(-1).min()) > 1 - 1e-12 and float(p.float().min()) > TINY


def _check_softmax(x, dy, p_got, dx_got, what):
    p, dx, b_p, b_dx = _softmax_reference(x, dy)
    rp = _worst(p_got, p, C_SOFTMAX * b_p + TINY)
    rdx = _worst(dx_got, dx, C_SOFTMAX_BWD * b_dx + TINY * (1 + float(dy.abs().max())))
    print(f"{what}: error / bound p {rp:.3f} dx {rdx:.3f}")
    assert rp <= 1.0 and rdx <= 1.0, f"{what}: error beyond the per-element bound, worst error / bound: p {rp} dx {rdx}"


@pytest.mark.parametrize("regime", ["peaked", "shifted", "one_hot"])
@pytest.mark.parametrize("n", [37, 4096, 5000])
def test_softmax_checker_accepts_float32_torch(n, regime):
    x, dy = _softmax_rows(n, regime)
    _assert_softmax_regime(regime, x, _softmax_reference(x, dy)[0])
    x32 = x.clone().requires_grad_(True)
    p = (x32 * SCALE).softmax(dim=-1)
    p.backward(dy)
    _check_softmax(x, dy, p, x32.grad, f"float32 torch softmax {n} {regime}")


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["peaked", "shifted", "one_hot"])
@pytest.mark.parametrize("n", [37, 4096, 5000])
def test_softmax_scaled_per_element(n, regime, device):
    """softmax_fwd_f32 / softmax_bwd_f32 (rows kept in registers up to 4096, re-read beyond) through softmax_scaled_."""
    _, PF = _mods()
    x, dy = _softmax_rows(n, regime)
    _assert_softmax_regime(regime, x, _softmax_reference(x, dy)[0])
    xd = x.to(device).requires_grad_(True)
    p = PF.softmax_scaled_(xd * 1.0, SCALE)          # in place on the temporary
    p.backward(dy.to(device))
    _check_softmax(x, dy, p, xd.grad, f"softmax_scaled_ {n} {regime}")


# ---- the table in the module docstring -------------------------------------------------------------------------------------
def _measure():
    """Worst error / bound-with-c=1 of the reference-only evaluations over CASES (and the softmax rows)."""
    one32, one16 = dict.fromkeys(C_F32, 1.0), dict.fromkeys(C_B16, 1.0)
    worst32, worst16, where = dict.fromkeys(C_F32, 0.0), dict.fromkeys(C_B16, 0.0), {}
    for case in CASES:
        (b, h, nq, nk), regime = case
        q, kv, dout = _inputs((b, h, nq, nk), regime)
        back = nq <= 128
        r = _reference(q, kv, dout, h, SCALE, backward=back)
        bd = _bounds(r, one32)
        got = _torch_attention(q, kv, h, SCALE, dout=dout if back else None)
        row = {"out": _worst(got[0], r.out, bd["out"]), "lse": _worst(got[1], r.lse, bd["lse"])}
        if back:
            inner = h * HD
            row.update(dq=_worst(got[2], r.dq, bd["dq"]), dk=_worst(got[3][..., :inner], r.dkv[..., :inner], bd["dkv"][..., :inner]),
                       dv=_worst(got[3][..., inner:], r.dkv[..., inner:], bd["dkv"][..., inner:]))
            r16 = _reference(q, kv, dout, h, SCALE, round_bf16=True)
            g16 = _bf16_p_attention(r16, q, kv, dout, h, SCALE)
            # the bf16 term alone, c = 1 (no f32 term: these evaluations are float64)
            row16 = {"out": _worst(g16[0], r16.out, U16 * r16.out_abs + r16.out_floor),
                     "dq": _worst(g16[2], r16.dq, U16 * r16.dq_abs + r16.dq_floor),
                     "dk": _worst(g16[3][..., :inner], r16.dkv[..., :inner], U16 * r16.dkv_abs[..., :inner] + r16.dk_floor),
                     "dv": _worst(g16[3][..., inner:], r16.dkv[..., inner:], U16 * r16.dkv_abs[..., inner:] + r16.dv_floor)}
            for k_, v_ in row16.items():
                worst16[k_] = max(worst16[k_], v_)
        else:
            row16 = {}
        for k_, v_ in row.items():
            if v_ > worst32[k_]:
                worst32[k_], where[k_] = v_, _case_id(case)
        print(_case_id(case), "f32", {k_: round(v_, 3) for k_, v_ in row.items()}, "bf16", {k_: round(v_, 3) for k_, v_ in row16.items()})
    print("worst float32:", worst32, where)
    print("worst bf16 P / dS:", worst16)
    sp = sd = 0.0
    for n in (37, 4096, 5000):
        for regime in ("peaked", "shifted", "one_hot"):
            x, dy = _softmax_rows(n, regime)
            p, dx, b_p, b_dx = _softmax_reference(x, dy)
            x32 = x.clone().requires_grad_(True)
            p32 = (x32 * SCALE).softmax(dim=-1)
            p32.backward(dy)
            sp = max(sp, _worst(p32, p, b_p + TINY))
            sd = max(sd, _worst(x32.grad, dx, b_dx + TINY * (1 + float(dy.abs().max()))))
    print("worst float32 softmax: p", sp, "dx", sd)


if __name__ == "__main__":
    _measure()
