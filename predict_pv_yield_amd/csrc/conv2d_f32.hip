// Conv2d 3x3, stride 1, no padding, in exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per product,
// f32 accumulation) for the satellite-image encoder of experiments/002_cnn_processes_single_sat_image_then_rnn.py
// (sat_conv1..3 at :93-101, the 17-channel input built at :140-162 and :180-208).
//
// All three passes are implicit GEMMs over a band of output rows of one image staged in LDS:
//   forward / dgrad  D[m][pos]  = sum_{tap, c} A[m][(tap, c)] * X[c][pos + tap]     A = weights, held in VGPRs
//   wgrad            D[co][col] = sum_{pos} dy[co][pos] * X[ci][pos + tap]           col = (ci, tap), plus a ones column
// dgrad is the forward of dy zero-padded by 2 with mirrored, channel-swapped weights; its epilogue gates dx by the layer
// input (> 0) so it leaves as the lower layer's pre-activation gradient.  The first layer never materialises its input:
// its 12 satellite channels are read channels-last from sat_data and the 5 synthesised channels are computed while the
// band is staged.  wgrad splits the (image, band) items into fixed slabs, each block writing its partial sums to its own
// workspace slab, then adds the slabs in index order: no atomics, identical bits run to run.  The 32 -> 4 layer's weight
// gradient is the one pass these tiles do not fit; it takes the general Conv3d f32 kernel (general_wgrad_geom below).  The
// slab sum, the synthesised channels and the shared argument checks are in conv2d_f32_common.h.
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int kSatChannels = 12;
constexpr int kCoordChannels = 17;   // 12 satellite + centre marker, geo x, geo y, pixel x, pixel y

struct C2 {
  // input of the pass: x[n][c_in][h_in][w_in] (mode plain) or sat[n][h_in][w_in][12] + coords (mode coords)
  const float* x;
  const float* gate;       // plain input gated by (gate > 0) while staged (same layout as x); may be null
  const float* xc;         // [n / t][w_in] geo x (varies along the last axis)
  const float* yc;         // [n / t][h_in] geo y (varies along rows)
  const float* w;          // weights, element (m, c, tap) at w[m * w_sm + c * w_sc + (flip ? 8 - tap : tap)]
  const float* bias;       // [m_out] or null
  float* y;                // y[n][m_out][h_out][w_out]
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int n, c_in, m_out, h_in, w_in, pad, h_out, w_out, rb, n_bands, t_per_ex, w_sm, w_sc, flip, relu;
};

// Stage input rows [ir0, ir0 + rows) x columns [ic0, ic0 + cols) of image n, channels [0, cinp), as lds[c][r][col]
// (channel stride cs, row stride cols); outside the image (padding) and beyond c_in: 0.
template <bool COORDS>
__device__ void stage_band(float* lds, const C2& a, int cinp, int cs, int n, int ir0, int rows, int ic0, int cols) {
  if (COORDS) {
    // satellite channels: global reads in their native channels-last order (12 consecutive floats per pixel)
    const int tot = rows * cols * kSatChannels;
    for (int i = threadIdx.x; i < tot; i += kBlock) {
      const int ch = i % kSatChannels, pix = i / kSatChannels;
      const int col = pix % cols, r = pix / cols;
      const int ir = ir0 + r, ic = ic0 + col;
      float v = 0.0f;
      if (ir >= 0 && ir < a.h_in && ic >= 0 && ic < a.w_in)
        v = a.x[(((size_t)n * a.h_in + ir) * a.w_in + ic) * kSatChannels + ch];
      lds[ch * cs + r * cols + col] = v;
    }
    const int b = n / a.t_per_ex;
    const float* xc_b = a.xc + (size_t)b * a.w_in;
    const float* yc_b = a.yc + (size_t)b * a.h_in;
    const int tot2 = (cinp - kSatChannels) * rows * cols;
    for (int i = threadIdx.x; i < tot2; i += kBlock) {
      const int col = i % cols, r = (i / cols) % rows, ch = kSatChannels + i / (cols * rows);
      const int ir = ir0 + r, ic = ic0 + col;
      float v = 0.0f;
      // the channels of experiments/002...py:140-162, 180-208 (row r = the W axis, column c = the H axis); 0 beyond them
      if (ir >= 0 && ir < a.h_in && ic >= 0 && ic < a.w_in)
        v = synth_channel(ch - kSatChannels, ir, ic, a.h_in / 2, a.w_in / 2, xc_b, yc_b);
      lds[ch * cs + r * cols + col] = v;
    }
  } else {
    const int tot = cinp * rows * cols;
    for (int i = threadIdx.x; i < tot; i += kBlock) {
      const int col = i % cols, r = (i / cols) % rows, ch = i / (cols * rows);
      const int ir = ir0 + r, ic = ic0 + col;
      float v = 0.0f;
      if (ch < a.c_in && ir >= 0 && ir < a.h_in && ic >= 0 && ic < a.w_in) {
        const size_t off = (((size_t)n * a.c_in + ch) * a.h_in + ir) * a.w_in + ic;
        v = a.x[off];
        if (a.gate && !(a.gate[off] > 0.0f)) v = 0.0f;
      }
      lds[ch * cs + r * cols + col] = v;
    }
  }
}

// Forward / dgrad.  Block = one band of rb output rows of one image; wave w takes 16-position tiles w, w + 4, ... of the
// band's flattened rows.  CINP = input channels rounded up to 4 (one MFMA k-step = 4 channels of one tap), MT = 16-row
// tiles of output channels.  Per tile: 9 * CINP / 4 k-steps, each one ds_read_b32 (B: 4 channels x 16 positions) feeding
// MT MFMAs against weights resident in VGPRs (A: 16 output channels x 4 channels).
template <int CINP, int MT, bool COORDS>
__global__ __launch_bounds__(kBlock) void conv2d_mfma_f32(C2 a) {
  extern __shared__ float lds[];
  constexpr int KS = CINP / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x / a.n_bands, band = blockIdx.x % a.n_bands;
  const int r0 = band * a.rb, rows = min(a.rb, a.h_out - r0);
  const int sw = a.w_out + 2, srows = rows + 2, cs = (a.rb + 2) * sw;

  // weights: lane holds A[m = mt * 16 + lane % 16][c = s * 4 + lane / 16] of every tap
  float wa[MT][9][KS];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = mt * 16 + (lane & 15);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int c = s * 4 + (lane >> 4);
        wa[mt][tap][s] = (m < a.m_out && c < a.c_in) ? a.w[m * a.w_sm + c * a.w_sc + (a.flip ? 8 - tap : tap)] : 0.0f;
      }
    }
  }
  float bias[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mt * 16 + (lane >> 4) * 4 + i;
      bias[mt][i] = (a.bias && m < a.m_out) ? a.bias[m] : 0.0f;
    }

  stage_band<COORDS>(lds, a, CINP, cs, n, r0 - a.pad, srows, -a.pad, sw);
  __syncthreads();

  const int npos = rows * a.w_out, tiles = (npos + 15) / 16;
  for (int t = wave; t < tiles; t += 4) {
    const int p = t * 16 + (lane & 15);
    const bool valid = p < npos;
    const int pp = valid ? p : 0;
    const int oh = pp / a.w_out, ow = pp - oh * a.w_out;
    const float* src = lds + (lane >> 4) * cs + oh * sw + ow;
    acc4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const float* st = src + (tap / 3) * sw + (tap % 3);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float b = st[s * 4 * cs];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][tap][s], b, acc[mt], 0, 0, 0);
      }
    }
    if (valid) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt * 16 + (lane >> 4) * 4 + i;
          if (m < a.m_out) {
            const size_t off = (((size_t)n * a.m_out + m) * a.h_out + r0 + oh) * a.w_out + ow;
            float v = acc[mt][i] + bias[mt][i];
            if (a.relu) v = v > 0.0f ? v : 0.0f;
            if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
            a.y[off] = v;
          }
        }
    }
  }
}

// wgrad.  D[co][col] over the positions of every (image, band) item of this block's slab; col = ci * 9 + tap for
// col < c_in * 9, col == c_in * 9 is a column of ones (dbias), the rest zero.  Wave w owns the 16-column tiles w, w + 4,
// ... (NTW of them at most) against all MT output-channel tiles; a k-step is 4 positions (A: dy, 16 channels x 4
// positions; B: 4 positions x 16 columns).  The band's dy lives in LDS as [MT * 16][dps] (zero beyond c_out and beyond
// the band), x as [cinp][rb + 2][w_in], plus xo[pos] = the position's offset in the x band.
struct W2 {
  C2 a;                    // x / gate / coords as for the forward; m_out = c_out of the layer
  const float* dy;         // [n][c_out][h_out][w_out]
  const float* dy_gate;    // dy zeroed where dy_gate <= 0; may be null
  float* slabs;            // [n_slabs][c_out][c_in * 9 + 1]
  int items, per, cinp;
};

template <int MT, int NTW, bool COORDS>
__global__ __launch_bounds__(kBlock) void conv2d_wgrad_mfma_f32(W2 q) {
  extern __shared__ float lds[];
  const C2& a = q.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k9 = a.c_in * 9, ncols = k9 + 1, nt = (ncols + 15) / 16;
  const int xs = (a.rb + 2) * a.w_in;                     // x-band channel stride
  const int dps = (a.rb * a.w_out + 3) & ~3;               // dy-band channel stride (positions, multiple of 4)
  float* xl = lds;
  float* dl = xl + q.cinp * xs;
  int* xo = (int*)(dl + MT * 16 * dps);

  // per owned column tile: the lane's column -> offset in the x band, multiplier and addend (ones / zero columns)
  int coff[NTW];
  float bmul[NTW], badd[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave + 4 * j) * 16 + (lane & 15);
    const bool real = col < k9;
    const int ci = real ? col / 9 : 0, tap = real ? col % 9 : 0;
    coff[j] = ci * xs + (tap / 3) * a.w_in + tap % 3;
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
    const int n = it / a.n_bands, band = it % a.n_bands;
    const int r0 = band * a.rb, rows = min(a.rb, a.h_out - r0), npos = rows * a.w_out;
    __syncthreads();   // the previous item's reads are done
    stage_band<COORDS>(xl, a, q.cinp, xs, n, r0, rows + 2, 0, a.w_in);
    for (int i = threadIdx.x; i < MT * 16 * dps; i += kBlock) {
      const int co = i / dps, p = i - co * dps;
      float v = 0.0f;
      if (co < a.m_out && p < npos) {
        const size_t off = (((size_t)n * a.m_out + co) * a.h_out + r0) * a.w_out + p;
        v = q.dy[off];
        if (q.dy_gate && !(q.dy_gate[off] > 0.0f)) v = 0.0f;
      }
      dl[i] = v;
    }
    for (int p = threadIdx.x; p < dps; p += kBlock) {
      const int oh = p / a.w_out, ow = p - oh * a.w_out;
      xo[p] = p < npos ? oh * a.w_in + ow : 0;
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
  // this slab's partial sums: D row co = mt * 16 + (lane / 16) * 4 + i, column = tile * 16 + lane % 16
  float* out = q.slabs + (size_t)blockIdx.x * a.m_out * ncols;
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave + 4 * j) * 16 + (lane & 15);
    if (wave + 4 * j < nt && col < ncols) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int co = mt * 16 + (lane >> 4) * 4 + i;
          if (co < a.m_out) out[co * ncols + col] = acc[mt][j][i];
        }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

constexpr int kMaxSlabs = 512;
constexpr size_t kMaxLds = 64 * 1024;

// output rows per band: about 192 positions, bands of equal height, the staged input rows within kMaxLds
int band_rows(int h_out, int w_out, int cinp) {
  int rb = std::max(1, std::min(h_out, (192 + w_out - 1) / w_out));
  while (rb > 1 && (size_t)cinp * (rb + 2) * (w_out + 2) * sizeof(float) > kMaxLds) --rb;
  const int nb = (h_out + rb - 1) / rb;
  return (h_out + nb - 1) / nb;
}

size_t fwd_lds_bytes(int cinp, int rb, int w_out) { return (size_t)cinp * (rb + 2) * (w_out + 2) * sizeof(float); }

size_t wgrad_lds_bytes(int cinp, int mt, int rb, int w_in, int w_out) {
  const size_t dps = ((size_t)rb * w_out + 3) & ~(size_t)3;
  return ((size_t)cinp * (rb + 2) * w_in + (size_t)mt * 16 * dps) * sizeof(float) + dps * sizeof(int);
}

struct WgradPlan {
  int rb, n_bands, items, n_slabs, per, cinp, mt;
  size_t lds;
};

WgradPlan wgrad_plan(int n, int c_in, int c_out, int h_in, int w_in) {
  WgradPlan p;
  const int h_out = h_in - 2, w_out = w_in - 2;
  p.cinp = (c_in + 3) & ~3;
  p.mt = 2;   // c_out = 32 (4 output channels take the general kernel: general_wgrad_geom)
  p.rb = band_rows(h_out, w_out, p.cinp);
  while (p.rb > 1 && wgrad_lds_bytes(p.cinp, p.mt, p.rb, w_in, w_out) > kMaxLds) --p.rb;
  p.n_bands = (h_out + p.rb - 1) / p.rb;
  p.items = n * p.n_bands;
  // workspace: n_slabs <= 512 partials of c_out x (9 c_in + 1) floats, at most 512 x 32 x 289 x 4 B = 18.9 MB
  const int want = std::min(p.items, kMaxSlabs);
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  p.lds = wgrad_lds_bytes(p.cinp, p.mt, p.rb, w_in, w_out);
  return p;
}

int check_dims(const char* who, int n, int c_in, int c_out, int h_in, int w_in, bool coords) {
  int rc = check_conv_dims(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(w_in <= 96, PV_ESIZE, "%s: width %d beyond 96 (one band row per LDS image)", who, w_in);
  if (coords)
    PV_REQUIRE(c_out == 32, PV_ESIZE, "%s: unsupported channel count c_out=%d (the coords layer has 32)", who, c_out);
  else
    PV_REQUIRE(c_in == 32 && (c_out == 32 || c_out == 4), PV_ESIZE,
               "%s: unsupported channel counts c_in=%d c_out=%d (32 -> 32 or 32 -> 4)", who, c_in, c_out);
  return PV_OK;
}

size_t wgrad_ws_bytes(const WgradPlan& p, int c_in, int c_out) {
  return (size_t)p.n_slabs * c_out * (c_in * 9 + 1) * sizeof(float);
}

int launch_wgrad(const char* who, const C2& a, const float* dy, const float* dy_gate, float* dw, float* db,
                 const WgradPlan& p, void* ws, bool coords, hipStream_t st) {
  W2 q;
  q.a = a;
  q.a.rb = p.rb, q.a.n_bands = p.n_bands;
  q.dy = dy, q.dy_gate = dy_gate, q.slabs = (float*)ws, q.items = p.items, q.per = p.per, q.cinp = p.cinp;
  const dim3 grid((unsigned)p.n_slabs), block(kBlock);
  // column tiles: ceil((c_in * 9 + 1) / 16) = 10 (17 channels) or 19 (32 channels), over 4 waves
  if (coords) conv2d_wgrad_mfma_f32<2, 3, true><<<grid, block, p.lds, st>>>(q);
  else conv2d_wgrad_mfma_f32<2, 5, false><<<grid, block, p.lds, st>>>(q);
  int rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, db, a.m_out, a.c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

// The weight gradient of a 32 -> 4 layer (sat_conv3) is 0.95 GFLOP over the same 32-channel input bands as the 32 -> 32
// layer's: this kernel's 16-row output-channel tile would idle 12 of its rows and re-stage a 32-channel band per 4 output
// channels, so those calls take pv_conv3d_general_bwd_weight_f32 as a 1x3x3 conv with T = 1 (the same NCHW memory, dw
// [4][32][1][3][3] = [4][32][3][3]; deterministic: slab partials summed in slab order).
pv_conv3d_geom general_wgrad_geom(int n, int c_in, int c_out, int h_in, int w_in) {
  pv_conv3d_geom g = {};
  g.batch = n, g.c_in = c_in, g.c_out = c_out, g.t_in = 1, g.h_in = h_in, g.w_in = w_in;
  g.k_t = 1, g.k_h = 3, g.k_w = 3, g.stride_t = 1, g.stride_h = 1, g.stride_w = 1;
  return g;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_coords_fwd_f32(const float* sat, const float* x_coords, const float* y_coords, const float* w,
                             const float* bias, float* y, int32_t n, int32_t t_per_example, int32_t h_in, int32_t w_in,
                             int32_t c_out, void* stream) {
  const char* who = "pv_conv2d_coords_fwd_f32";
  PV_REQUIRE(sat && x_coords && y_coords && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, kCoordChannels, c_out, h_in, w_in, true);
  if (rc) return rc;
  PV_REQUIRE(t_per_example > 0 && n % t_per_example == 0, PV_EINVAL, "%s: n=%d is not a multiple of t_per_example=%d",
             who, n, t_per_example);
  C2 a = {};
  a.x = sat, a.xc = x_coords, a.yc = y_coords, a.w = w, a.bias = bias, a.y = y;
  a.n = n, a.c_in = kCoordChannels, a.m_out = c_out, a.h_in = h_in, a.w_in = w_in, a.pad = 0;
  a.h_out = h_in - 2, a.w_out = w_in - 2, a.t_per_ex = t_per_example;
  a.w_sm = kCoordChannels * 9, a.w_sc = 9, a.flip = 0, a.relu = 1;
  a.rb = band_rows(a.h_out, a.w_out, 20);
  a.n_bands = (a.h_out + a.rb - 1) / a.rb;
  const size_t lds = fwd_lds_bytes(20, a.rb, a.w_out);
  conv2d_mfma_f32<20, 2, true><<<dim3((unsigned)(n * a.n_bands)), dim3(kBlock), lds, as_stream(stream)>>>(a);
  return check_launch(who);
}

int pv_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                      int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  C2 a = {};
  a.x = x, a.w = w, a.bias = bias, a.y = y;
  a.n = n, a.c_in = c_in, a.m_out = c_out, a.h_in = h_in, a.w_in = w_in, a.pad = 0;
  a.h_out = h_in - 2, a.w_out = w_in - 2, a.t_per_ex = 1;
  a.w_sm = c_in * 9, a.w_sc = 9, a.flip = 0, a.relu = relu ? 1 : 0;
  a.rb = band_rows(a.h_out, a.w_out, 32);
  a.n_bands = (a.h_out + a.rb - 1) / a.rb;
  const size_t lds = fwd_lds_bytes(32, a.rb, a.w_out);
  const dim3 grid((unsigned)(n * a.n_bands)), block(kBlock);
  // 4 output channels: one 16-row tile (12 rows idle) -- the layer is 6 % of the forward's products
  if (c_out > 16) conv2d_mfma_f32<32, 2, false><<<grid, block, lds, as_stream(stream)>>>(a);
  else conv2d_mfma_f32<32, 1, false><<<grid, block, lds, as_stream(stream)>>>(a);
  return check_launch(who);
}

int pv_conv2d_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                           int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  // the forward of dy [n][c_out][h_in - 2][w_in - 2] padded by 2, weights mirrored with the channel roles swapped
  C2 a = {};
  a.x = dy, a.gate = dy_gate, a.w = w, a.y = dx, a.out_gate = x_gate;
  a.n = n, a.c_in = c_out, a.m_out = c_in, a.h_in = h_in - 2, a.w_in = w_in - 2, a.pad = 2;
  a.h_out = h_in, a.w_out = w_in, a.t_per_ex = 1;
  a.w_sm = 9, a.w_sc = c_in * 9, a.flip = 1, a.relu = 0;
  a.rb = band_rows(a.h_out, a.w_out, 32);
  a.n_bands = (a.h_out + a.rb - 1) / a.rb;
  const dim3 grid((unsigned)(n * a.n_bands)), block(kBlock);
  if (c_out > 16) conv2d_mfma_f32<32, 2, false><<<grid, block, fwd_lds_bytes(32, a.rb, a.w_out), as_stream(stream)>>>(a);
  else conv2d_mfma_f32<4, 2, false><<<grid, block, fwd_lds_bytes(4, a.rb, a.w_out), as_stream(stream)>>>(a);
  return check_launch(who);
}

int pv_conv2d_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                         size_t* bytes) {
  const char* who = "pv_conv2d_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, c_in == kCoordChannels);
  if (rc) return rc;
  if (c_out <= 16) {
    const pv_conv3d_geom g = general_wgrad_geom(n, c_in, c_out, h_in, w_in);
    return pv_conv3d_general_bwd_weight_workspace_bytes(&g, bytes);
  }
  const WgradPlan p = wgrad_plan(n, c_in, c_out, h_in, w_in);
  *bytes = wgrad_ws_bytes(p, c_in, c_out);
  return PV_OK;
}

int pv_conv2d_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                             int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                             void* stream) {
  const char* who = "pv_conv2d_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  if (c_out <= 16) {
    const pv_conv3d_geom g = general_wgrad_geom(n, c_in, c_out, h_in, w_in);
    size_t need = 0;
    rc = pv_conv3d_general_bwd_weight_workspace_bytes(&g, &need);
    if (rc) return rc;
    rc = check_workspace(who, ws, ws_bytes, need);
    if (rc) return rc;
    return pv_conv3d_general_bwd_weight_f32(x, dy, dy_gate, dw, dbias, &g, ws, ws_bytes, stream);
  }
  const WgradPlan p = wgrad_plan(n, c_in, c_out, h_in, w_in);
  rc = check_workspace(who, ws, ws_bytes, wgrad_ws_bytes(p, c_in, c_out));
  if (rc) return rc;
  C2 a = {};
  a.x = x, a.n = n, a.c_in = c_in, a.m_out = c_out, a.h_in = h_in, a.w_in = w_in, a.h_out = h_in - 2, a.w_out = w_in - 2;
  a.t_per_ex = 1;
  return launch_wgrad(who, a, dy, dy_gate, dw, dbias, p, ws, false, as_stream(stream));
}

int pv_conv2d_coords_bwd_weight_f32(const float* sat, const float* x_coords, const float* y_coords, const float* dy,
                                    float* dw, float* dbias, int32_t n, int32_t t_per_example, int32_t h_in,
                                    int32_t w_in, int32_t c_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_coords_bwd_weight_f32";
  PV_REQUIRE(sat && x_coords && y_coords && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, kCoordChannels, c_out, h_in, w_in, true);
  if (rc) return rc;
  PV_REQUIRE(t_per_example > 0 && n % t_per_example == 0, PV_EINVAL, "%s: n=%d is not a multiple of t_per_example=%d",
             who, n, t_per_example);
  const WgradPlan p = wgrad_plan(n, kCoordChannels, c_out, h_in, w_in);
  rc = check_workspace(who, ws, ws_bytes, wgrad_ws_bytes(p, kCoordChannels, c_out));
  if (rc) return rc;
  C2 a = {};
  a.x = sat, a.xc = x_coords, a.yc = y_coords;
  a.n = n, a.c_in = kCoordChannels, a.m_out = c_out, a.h_in = h_in, a.w_in = w_in, a.h_out = h_in - 2,
  a.w_out = w_in - 2, a.t_per_ex = t_per_example;
  return launch_wgrad(who, a, dy, nullptr, dw, dbias, p, ws, true, as_stream(stream));
}

}  // extern "C"
