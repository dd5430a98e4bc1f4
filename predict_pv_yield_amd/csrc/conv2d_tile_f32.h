// The two implicit GEMMs of an exact-f32 Conv2d 3x3 whose weights fit the VGPRs (at most 32 x 32 channels), over a tile of
// tr x tc output positions of one image staged in LDS (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation):
//   forward-like  D[m][pos]  = sum_{tap, c} A[m][(tap, c)] * X[c][pos + tap]     A = weights, held in VGPRs
//   wgrad-like    D[m][col]  = sum_{pos} G[m][pos] * X[c][pos + tap]             col = (c, tap), plus a ones column
// conv2d_f32.hip (experiments/002: full-width bands of rows, tc = w_out), conv2d_ae_f32.hip (notebooks/16_maxpool: tiles of
// at most 64 columns) and conv2d_s2_f32.hip (notebooks 14 / 15: the same two GEMMs at stride 2, STRIDE = 2, the tile staged
// split by column parity) instantiate them; each keeps its tile planner, its argument checks and its first layer's source
// kind.  conv3d_s2_f32.hip (notebook 08) instantiates the stride-2 weight gradient over depth slices of NCDHW tensors
// (SRC_DEPTH) and keeps forward-like kernels of its own, which run one K pass per depth tap.  conv2d_frames_f32.hip (notebook
// 07) instantiates both at stride 2 over its per-frame sources (SRC_FRAME_HORIZON, SRC_FRAME_SHARED, SRC_CH_GROUP).
// conv2d_inputs_f32.hip (notebook 05) instantiates both at stride 1 with conv2d_ae_f32.hip's planners (conv2d_ae_plan_f32.h)
// over its three-tensor first layer (SRC_INPUTS4) and the horizon channel (SRC_HORIZON, conv2d_horizon_f32.h).  A
// forward-like output element's sum depends only on the (tap, channel group) order, not on the tile it
// falls in; the weight gradient's bits depend on the row-major position order inside an item, the items per slab and the
// slab order (fixed slabs, each block writing its own, added in slab order: no atomics, identical bits run to run).
#pragma once
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int kLdsFloats = 16 * 1024;   // 64 KB per block (two blocks per CU)
constexpr int kMaxSlabs = 512;

// input channel ch (0 <= ch < c_in) of image n at (r, col), inside [0, h) x [0, w).  A file's own source kind is an
// explicit specialisation of this (or of stage_in) in that file.
template <int SRC>
__device__ __forceinline__ float load_in(const In& s, int n, int ch, int r, int col) {
  static_assert(SRC == SRC_PLAIN || SRC == SRC_POOLED, "this source kind needs its file's specialisation");
  return SRC == SRC_POOLED ? load_pooled(s, n, ch, r, col) : load_plain(s, n, ch, r, col);
}

// Stage channels [0, cinp) x rows [r0, r0 + rows) x columns [c0, c0 + cols) of image n as lds[ch][r][col]; outside the
// image (padding) and beyond the source's channels: 0.
template <int SRC>
__device__ void stage_in(float* lds, const In& s, int n, int cinp, int r0, int rows, int c0, int cols) {
  const int tot = cinp * rows * cols;
  for (int i = threadIdx.x; i < tot; i += kBlock) {
    const int col = i % cols, r = (i / cols) % rows, ch = i / (cols * rows);
    const int ir = r0 + r, ic = c0 + col;
    float v = 0.0f;
    if (ch < s.c_in && ir >= 0 && ir < s.h && ic >= 0 && ic < s.w) v = load_in<SRC>(s, n, ch, ir, ic);
    lds[i] = v;
  }
}

// The same for a stride-2 pass, split by column parity: row r of a channel holds its even columns first ((cols + 1) / 2 of
// them), then its odd ones, so that the columns 2 ow + kw of consecutive ow are consecutive words for each kw (kw = 0, 2:
// even part at ow, ow + 1; kw = 1: odd part at ow) -- a unit-stride ds_read_b32 where the plain layout read at stride 2
// would put two lanes on every bank.
__device__ __forceinline__ int split_col(int col, int n_even) { return (col & 1) * n_even + (col >> 1); }

template <int SRC>
__device__ void stage_in_split(float* lds, const In& s, int n, int cinp, int r0, int rows, int c0, int cols) {
  const int tot = cinp * rows * cols, n_even = (cols + 1) / 2;
  for (int i = threadIdx.x; i < tot; i += kBlock) {
    const int col = i % cols, r = (i / cols) % rows, ch = i / (cols * rows);
    const int ir = r0 + r, ic = c0 + col;
    float v = 0.0f;
    if (ch < s.c_in && ir >= 0 && ir < s.h && ic >= 0 && ic < s.w) v = load_in<SRC>(s, n, ch, ir, ic);
    lds[i - col + split_col(col, n_even)] = v;
  }
}

struct Fwd {
  In in;
  const float* w;          // element (m, c, tap) at w[m * w_sm + c * w_sc + (flip ? 8 - tap : tap)]
  const float* bias;       // [m_out] or null
  float* y;                // POOL: pooled [n][m_out][h_out / 3][w_out / 3]; else [n][m_out][h_out][w_out]
  uint8_t* codes;          // POOL: same shape as y
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int m_out, pad, h_out, w_out, tr, tc, n_rb, n_cb, w_sm, w_sc, flip, relu;
};

// weights resident in VGPRs: lane holds A[m = mt * 16 + lane % 16][c = s * 4 + lane / 16] of every tap
template <int MT, int KS>
__device__ __forceinline__ void load_weights(float (&wa)[MT][9][KS], const Fwd& a, int lane) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = mt * 16 + (lane & 15);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int c = s * 4 + (lane >> 4);
        wa[mt][tap][s] = (m < a.m_out && c < a.in.c_in) ? a.w[m * a.w_sm + c * a.w_sc + (a.flip ? 8 - tap : tap)] : 0.0f;
      }
    }
  }
}

// one output element of a forward-like pass: bias, ReLU, output gate
__device__ __forceinline__ void store_out(const Fwd& a, int n, int m, int r, int c, float acc) {
  const size_t off = (((size_t)n * a.m_out + m) * a.h_out + r) * a.w_out + c;
  float v = acc + (a.bias ? a.bias[m] : 0.0f);
  if (a.relu) v = v > 0.0f ? v : 0.0f;
  if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
  a.y[off] = v;
}

// Forward-like pass.  Block = (image, row band, column band): tr x tc output positions flattened row-major, wave w takes
// the 16-position tiles w, w + 4, ...  CINP = input channels rounded up to 4 (one MFMA k-step = 4 channels of one tap), MT
// = 16-row tiles of output channels.  Per tile: 9 * CINP / 4 k-steps, each one ds_read_b32 (B: 4 channels x 16 positions)
// feeding MT MFMAs against weights resident in VGPRs (A: 16 output channels x 4 channels).  The bias is added after the
// accumulation.  POOL: the tile is one row of whole windows (3 x 3 k positions); pre-activations go to LDS behind the
// staged tile, then every thread takes (channel, window) pairs through pool3_relu.  STRIDE = 2 (pad 0, no POOL): output (oh,
// ow) reads rows 2 oh + kh and columns 2 ow + kw of a (2 rows + 1) x (2 cols + 1) tile staged split by column parity.
template <int CINP, int MT, int SRC, bool POOL, int STRIDE = 1>
__global__ __launch_bounds__(kBlock) void conv2d_tile_fwd(Fwd a) {
  static_assert(STRIDE == 1 || (STRIDE == 2 && !POOL), "stride 1, or stride 2 without the pool");
  extern __shared__ float lds[];
  constexpr int KS = CINP / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bid = blockIdx.x;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int n = bid / a.n_rb;
  const int r0 = rb * a.tr, c0 = cb * a.tc;
  const int rows = min(a.tr, a.h_out - r0), cols = min(a.tc, a.w_out - c0);
  const int sw = STRIDE == 2 ? 2 * cols + 1 : cols + 2, sr = STRIDE == 2 ? 2 * rows + 1 : rows + 2;
  const int cs = sr * sw, npos = rows * cols;

  // SRC_FRAME_SHARED: image n = n_frames b + f takes the f-th slice of m_out rows of the weight (a block-uniform offset)
  if constexpr (SRC == SRC_FRAME_SHARED) a.w += (size_t)(n % a.in.n_frames) * a.m_out * a.w_sm;
  float wa[MT][9][KS];
  load_weights<MT, KS>(wa, a, lane);

  if constexpr (STRIDE == 2) stage_in_split<SRC>(lds, a.in, n, CINP, 2 * r0, sr, 2 * c0, sw);
  else stage_in<SRC>(lds, a.in, n, CINP, r0 - a.pad, sr, c0 - a.pad, sw);
  __syncthreads();
  float* pre = lds + CINP * cs;   // POOL: [MT * 16][npos]

  const int tiles = (npos + 15) / 16;
  for (int t = wave; t < tiles; t += 4) {
    const int p = t * 16 + (lane & 15);
    const bool valid = p < npos;
    const int pp = valid ? p : 0;
    const int oh = pp / cols, ow = pp - oh * cols;
    const float* src = lds + (lane >> 4) * cs + STRIDE * oh * sw + ow;
    acc4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      // stride 2: kw = 1 is the odd half (cols + 1 words in), kw = 2 the even half one word on
      const float* st = src + (tap / 3) * sw + (STRIDE == 2 ? (tap % 3 == 1 ? cols + 1 : tap % 3 / 2) : tap % 3);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float b = st[s * 4 * cs];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][tap][s], b, acc[mt], 0, 0, 0);
      }
    }
    if (!valid) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt * 16 + (lane >> 4) * 4 + i;
        if (POOL) {
          pre[m * npos + p] = acc[mt][i];
        } else if (m < a.m_out) {
          store_out(a, n, m, r0 + oh, c0 + ow, acc[mt][i]);
        }
      }
  }
  if (!POOL) return;

  __syncthreads();
  const int pw_tile = cols / 3, ph = a.h_out / 3, pw = a.w_out / 3;
  for (int e = threadIdx.x; e < MT * 16 * pw_tile; e += kBlock) {
    const int m = e / pw_tile, wc = e - m * pw_tile;
    if (m >= a.m_out) continue;
    const float bm = a.bias ? a.bias[m] : 0.0f;
    const float* win = pre + m * npos + wc * 3;
    const size_t off = (((size_t)n * a.m_out + m) * ph + rb) * pw + c0 / 3 + wc;
    a.y[off] = pool3_relu([&](int k) { return win[(k / 3) * cols + k % 3] + bm; }, a.codes[off]);
  }
}

// wgrad-like pass.  D[m][col] over the positions of every (image, tile) item of this block's slab; col = c * 9 + tap for
// col < in.c_in * 9, col == in.c_in * 9 is a column of ones (dbias), the rest zero.  Wave w owns the 16-column tiles w, w +
// 4, ... (NTW at most) against all MT row tiles; a k-step is 4 positions (A: g, 16 rows x 4 positions; B: 4 positions x 16
// columns).  The tile's g lives in LDS as [MT * 16][dps] (zero beyond g.c_in rows and beyond the tile), x as [cinp][tr + 2]
// [tc + 2] read from (r0 - pad, c0 - pad), plus xo[pos] = the position's offset in the x tile.
struct Wg {
  In in;                    // the operand that slides under the taps
  In g;                     // the operand at the output positions, c_in = the D rows (the layer's output channels)
  float* slabs;             // [n_slabs][g.c_in][in.c_in * 9 + 1]
  int pad, h_out, w_out, tr, tc, n_rb, n_cb, items, per, cinp;
};

// STRIDE = 2 (pad 0): position (oh, ow) slides over x at (2 oh + kh, 2 ow + kw); the x tile is (2 tr + 1) x (2 tc + 1), staged
// split by column parity (stage_in_split).
template <int MT, int NTW, int XSRC, int GSRC, int STRIDE = 1>
__global__ __launch_bounds__(kBlock) void conv2d_tile_wgrad(Wg q) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // GSRC == SRC_CH_GROUP: blockIdx.y names the group of g.c_in channels of g whose rows this block sums, and a slab holds
  // every group's rows one after the other ([n_slabs][groups * g.c_in][ncols]: one slab sum over all of them)
  if constexpr (GSRC == SRC_CH_GROUP) q.g.t_per_ex = blockIdx.y * q.g.c_in;
  const int k9 = q.in.c_in * 9, ncols = k9 + 1, nt = (ncols + 15) / 16;
  const int sw = STRIDE == 2 ? 2 * q.tc + 1 : q.tc + 2, sr = STRIDE == 2 ? 2 * q.tr + 1 : q.tr + 2, cs = sr * sw;
  const int dps = (q.tr * q.tc + 3) & ~3;
  float* xl = lds;
  float* dl = xl + q.cinp * cs;
  int* xo = (int*)(dl + MT * 16 * dps);

  // per owned column tile: the lane's column -> offset in the x tile, multiplier and addend (ones / zero columns)
  int coff[NTW];
  float bmul[NTW], badd[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave + 4 * j) * 16 + (lane & 15);
    const bool real = col < k9;
    const int ci = real ? col / 9 : 0, tap = real ? col % 9 : 0;
    coff[j] = ci * cs + (tap / 3) * sw + (STRIDE == 2 ? (tap % 3 == 1 ? q.tc + 1 : tap % 3 / 2) : tap % 3);
    bmul[j] = real ? 1.0f : 0.0f;
    badd[j] = col == k9 ? 1.0f : 0.0f;
  }
  acc4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};

  const int it0 = blockIdx.x * q.per, it1 = min(it0 + q.per, q.items);
  for (int it = it0; it < it1; ++it) {
    const int cb = it % q.n_cb, rb = (it / q.n_cb) % q.n_rb, n = it / (q.n_cb * q.n_rb);
    const int r0 = rb * q.tr, c0 = cb * q.tc;
    const int rows = min(q.tr, q.h_out - r0), cols = min(q.tc, q.w_out - c0), npos = rows * cols;
    __syncthreads();   // the previous item's reads are done
    if constexpr (STRIDE == 2) stage_in_split<XSRC>(xl, q.in, n, q.cinp, 2 * r0, sr, 2 * c0, sw);
    else stage_in<XSRC>(xl, q.in, n, q.cinp, r0 - q.pad, sr, c0 - q.pad, sw);
    for (int i = threadIdx.x; i < MT * 16 * dps; i += kBlock) {
      const int m = i / dps, p = i - m * dps;
      float v = 0.0f;
      if (m < q.g.c_in && p < npos) {
        const int oh = p / cols, ow = p - oh * cols;
        v = load_in<GSRC>(q.g, n, m, r0 + oh, c0 + ow);
      }
      dl[i] = v;
    }
    for (int p = threadIdx.x; p < dps; p += kBlock) {
      const int oh = p / cols, ow = p - oh * cols;
      xo[p] = p < npos ? STRIDE * oh * sw + ow : 0;
    }
    __syncthreads();
    if (wave < nt) {
      const int steps = (npos + 3) / 4;
      for (int s = 0; s < steps; ++s) {
        const int p = s * 4 + (lane >> 4);
        const int xoff = xo[p];
        float av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = dl[(mt * 16 + (lane & 15)) * dps + p];
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          if (wave + 4 * j < nt) {
            const float b = xl[coff[j] + xoff] * bmul[j] + badd[j];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt][j], 0, 0, 0);
          }
        }
      }
    }
  }
  // this slab's partial sums: D row m = mt * 16 + (lane / 16) * 4 + i, column = tile * 16 + lane % 16
  size_t slab = blockIdx.x;
  if constexpr (GSRC == SRC_CH_GROUP) slab = slab * gridDim.y + blockIdx.y;
  float* out = q.slabs + slab * q.g.c_in * ncols;
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave + 4 * j) * 16 + (lane & 15);
    if (wave + 4 * j < nt && col < ncols) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt * 16 + (lane >> 4) * 4 + i;
          if (m < q.g.c_in) out[m * ncols + col] = acc[mt][j][i];
        }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// forward-like Fwd of a plain conv [c_in] -> [c_out] over x (pad 0) ...
inline Fwd conv_fwd_args(const float* w, const float* bias, float* y, int c_in, int c_out, int h_in, int w_in, int relu) {
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = c_out, a.pad = 0, a.h_out = h_in - 2, a.w_out = w_in - 2;
  a.w_sm = c_in * 9, a.w_sc = 9, a.flip = 0, a.relu = relu ? 1 : 0;
  return a;
}

// ... and of the padded, mirrored form: out [m_out] over a (h_src + 2) x (w_src + 2) grid from a [c] x h_src x w_src source,
// weights stored [c][m_out][3][3] (ConvTranspose2d forward) or [c][m_out] = [c_out][c_in] of a Conv2d (its data gradient)
inline Fwd full_fwd_args(const float* w, const float* bias, float* y, int m_out, int h_src, int w_src, int relu) {
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = m_out, a.pad = 2, a.h_out = h_src + 2, a.w_out = w_src + 2;
  a.w_sm = 9, a.w_sc = m_out * 9, a.flip = 1, a.relu = relu ? 1 : 0;
  return a;
}

// the forward-like pass over n images with the tiles (tr, tc, n_rb, n_cb) its caller planned
template <int CINP, int MT, int SRC, bool POOL, int STRIDE = 1>
int launch_fwd(const char* who, const Fwd& a, int n, hipStream_t st) {
  size_t lds = STRIDE == 2 ? (size_t)CINP * (2 * a.tr + 1) * (2 * a.tc + 1) : (size_t)CINP * (a.tr + 2) * (a.tc + 2);
  if (POOL) lds += (size_t)MT * 16 * a.tr * a.tc;
  lds *= sizeof(float);
  PV_REQUIRE(lds <= kLdsFloats * sizeof(float), PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, lds);
  const long long blocks = (long long)n * a.n_rb * a.n_cb;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  conv2d_tile_fwd<CINP, MT, SRC, POOL, STRIDE><<<dim3((unsigned)blocks), dim3(kBlock), lds, st>>>(a);
  return check_launch(who);
}

// The weight gradient's plan: (h_out, w_out) = the positions the sum runs over, tiles, and items = n * n_rb * n_cb (image,
// tile) pairs cut into n_slabs <= kMaxSlabs slabs of per items.  A caller sets the tiles, then slab_split fills the rest.
struct WgPlan {
  int h_out, w_out, tr, tc, n_rb, n_cb, items, n_slabs, per, cinp, mt;
  size_t lds, ws;
};

inline size_t wg_lds_floats(int cinp, int mt, int tr, int tc, int stride = 1) {
  const size_t dps = ((size_t)tr * tc + 3) & ~(size_t)3;
  const size_t tile = stride == 2 ? (size_t)(2 * tr + 1) * (2 * tc + 1) : (size_t)(tr + 2) * (tc + 2);
  return (size_t)cinp * tile + (size_t)mt * 16 * dps + dps;
}

// rows = the D rows (the layer's output channels), c = the sliding operand's channels
inline void slab_split(WgPlan& p, int n, int c, int rows, int stride = 1) {
  p.items = n * p.n_rb * p.n_cb;
  const int want = std::min(p.items, kMaxSlabs);
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  p.lds = wg_lds_floats(p.cinp, p.mt, p.tr, p.tc, stride) * sizeof(float);
  p.ws = (size_t)p.n_slabs * rows * (c * 9 + 1) * sizeof(float);
}

// the wgrad-like pass and its slab sum; MT = p.mt, NTW = ceil(ceil((9 in.c_in + 1) / 16) / 4) column tiles per wave
template <int MT, int NTW, int XSRC, int GSRC, int STRIDE = 1>
int launch_wgrad(const char* who, const In& in, const In& g, int pad, const WgPlan& p, float* dw, float* db, bool transposed,
                 void* ws, size_t ws_bytes, hipStream_t st) {
  int rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  PV_REQUIRE(p.lds <= kLdsFloats * sizeof(float), PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, p.lds);
  Wg q;
  q.in = in, q.g = g, q.slabs = (float*)ws, q.pad = pad;
  q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per, q.cinp = p.cinp;
  conv2d_tile_wgrad<MT, NTW, XSRC, GSRC, STRIDE><<<dim3((unsigned)p.n_slabs), dim3(kBlock), p.lds, st>>>(q);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, db, g.c_in, in.c_in * 9, p.n_slabs, st, transposed);
  return check_launch(who);
}

}  // namespace
}  // namespace pv
