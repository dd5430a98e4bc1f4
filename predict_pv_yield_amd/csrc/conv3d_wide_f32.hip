// Conv3d (2, 3, 3) on wide channel counts in exact f32 (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation)
// for the frame predictor of notebooks/12_just_3d_conv.ipynb (the nn.Sequential of LitAutoEncoder, raw lines 1397-1407 of the
// .ipynb file: Conv3d 2 -> 64 -> 128 -> 128 -> 128 -> 1, kernel (2, 3, 3), spatial padding 1; forward at 1409-1420).  A
// (2, 3, 3) stride-1 Conv3d is the sum of two padded 3x3 Conv2d's over adjacent depth slices, so the three passes are those of
// conv2d_wide_f32.hip with the depth tap kd as one more K axis and (image, output slice) where that file has the image:
//   pv_conv3d_wide_*          stride 1, spatial padding 1, depth padding 0 or 1, (c_in, c_out) = (64, 128) or (128, 128):
//     forward / dgrad  D[m][pos]  = sum_{kd, tap, c} A[m][(kd, tap, c)] * X[c][d + kd - pd][pos + tap]   64 x 256 per block
//     wgrad            D[co][col] = sum_{d, pos} dy[co][d][pos] * X[ci][d + kd - pd][pos + tap]          grid axis z = kd
//                             A depth slice outside the input is padding: it is skipped whole (no staging, no MFMAs).  dgrad
//                             is the forward of dy with depth padding 1 - pd, taps mirrored in all three axes and the channel
//                             roles swapped (so it also runs 128 -> 64).  wgrad keeps fixed slabs and adds them in slab order.
//   pv_conv3d_wide_horizon_*  the first layer, 2 -> 64, depth padding 0, ReLU: input channel 1 is the forecast horizon of the
//                             example, constant inside the image (0 in the spatial padding), synthesised while staging.  Its
//                             four (channel, kd) pairs are four pseudo-channels of one 3x3 conv (weight [64][2][2][3][3] read
//                             as [64][4][3][3]), so K = 36 is one chunk.
//   pv_conv2d_head_s2p1_*     3x3, stride 2, padding 1, one output channel, any c_in: the last layer on depth 2 is exactly this
//                             on the free views x [n][2 c][h][w] and w [1][2 c][3][3].  Vector code, as pv_conv2d_head_s2_*.
// The LDS layouts are those of conv2d_wide_f32.hip (weight rows 80 floats apart, input channel stride 16 mod 32, dy rows 98
// floats apart).  The slab sum and the workspace check are shared (conv2d_f32_common.h); the depth-sliced input has its own
// descriptor here.
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int kMT = 4, kMB = kMT * 16, kMBP = kMB + 16, kNTW = 4, kCC = 8, kPos = 4 * kNTW * 16;
constexpr int kMaxTc = 62, kMaxTr = 64;      // the staged band is at most 64 columns (one lane each) x 66 rows
constexpr int kWgCC = 14, kWgNTW = 2, kWgPos = 96, kWgDps = kWgPos + 2, kWgMaxTc = 48, kWgMaxTr = 32;
constexpr int kMaxWgBlocks = 512;
constexpr int kMaxW = 128;                   // widest input plane

// What a pass reads.  SRC3_PLAIN: x [n][c_in][d_in][h][w], zeroed where gate <= 0 (gate may be null).  SRC3_HORIZON: x =
// history [n][d_in][h][w]; pseudo-channel q = 2 * channel + kd of output slice d is history slice d + q for q < 2 and
// horizon[n] for q = 2, 3 (c_in = 4).
enum Src3 { SRC3_PLAIN, SRC3_HORIZON };

struct In3 {
  const float* x;
  const float* gate;
  const float* horizon;    // SRC3_HORIZON: [n]
  int c_in, d_in, h, w;
};

// channel ch (< c_in) of image n, slice ds, at (r, c) inside the image; ds inside [0, d_in) (SRC3_HORIZON: ds + 1 too)
template <int SRC>
__device__ __forceinline__ float load_in3(const In3& s, int n, int ch, int ds, int r, int c) {
  if (SRC == SRC3_HORIZON) {
    if (ch >= 2) return s.horizon[n];
    return s.x[(((size_t)n * s.d_in + ds + ch) * s.h + r) * s.w + c];
  }
  const size_t off = ((((size_t)n * s.c_in + ch) * s.d_in + ds) * s.h + r) * s.w + c;
  const float v = s.x[off];
  return (s.gate && !(s.gate[off] > 0.0f)) ? 0.0f : v;
}

// Stage channels [c0, c0 + cc) x rows [r0, r0 + rows) x columns [col0, col0 + cols) of slice ds of image n as lds[c * cs + r *
// sw + col]; outside the image (padding, a slice outside [0, d_in) included) and beyond c_in: 0.  One row per wave and pass,
// one column per lane: cols <= 64.
template <int SRC>
__device__ __forceinline__ void stage_rows3(float* lds, const In3& s, int n, int ds, int c0, int cc, int r0, int rows,
                                            int col0, int cols, int sw, int cs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ic = col0 + lane;
  const bool ok = ic >= 0 && ic < s.w && (SRC == SRC3_HORIZON || (ds >= 0 && ds < s.d_in));
  if (lane >= cols) return;
  int ch = 0, r = wave;
  while (r >= rows) r -= rows, ++ch;
  while (ch < cc) {
    const int gc = c0 + ch, ir = r0 + r;
    float v = 0.0f;
    if (ok && gc < s.c_in && ir >= 0 && ir < s.h) v = load_in3<SRC>(s, n, gc, ds, ir, ic);
    lds[ch * cs + r * sw + lane] = v;
    r += 4;
    while (r >= rows) r -= rows, ++ch;
  }
}

struct Fwd3 {
  In3 in;
  const float* w;          // element (m, c, kd, tap) at w[m * w_sm + c * w_sc + (flip ? 1 - kd : kd) * 9 + (flip ? 8 - tap : tap)]
  const float* bias;       // [m_out] or null
  float* y;                // [n][m_out][d_out][h_out][w_out]
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int m_out, pd, d_out, h_out, w_out, tr, tc, n_rb, n_cb, n_mg, w_sm, w_sc, flip, relu;
};

// channel stride of the staged band: >= rows * sw and 16 mod 32
__host__ __device__ inline int band_stride(int rows, int sw) {
  const int cs = rows * sw;
  return cs + ((16 - cs % 32) + 32) % 32;
}

// Forward / dgrad.  Block = (image, output slice, row band, column band, group of 64 output channels); the band is tr x tc
// output positions (<= 256) flattened row-major, wave w takes the 16-position tiles 4 w .. 4 w + 3.  Per depth tap whose
// source slice exists and per chunk of 8 input channels the weights [tap][c][m] and the input band [c][tr + 2][tc + 2] are
// staged, then 18 k-steps each read 4 A and 4 B values and issue 16 MFMAs.  SRC3_HORIZON: one depth tap (both are folded into
// the pseudo-channels), one chunk.
template <int SRC>
__global__ __launch_bounds__(kBlock) void wide3_fwd(Fwd3 a) {
  constexpr int MT = kMT, NTW = kNTW, CC = kCC, KS = CC / 4, MB = kMB, MBP = kMBP;
  constexpr int NKD = SRC == SRC3_HORIZON ? 1 : 2;
  extern __shared__ float lds[];
  float* wl = lds;                     // [9][CC][MBP]
  float* xl = lds + 9 * CC * MBP;      // [CC][csp]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bid = blockIdx.x;
  const int mg = bid % a.n_mg; bid /= a.n_mg;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb; bid /= a.n_rb;
  const int dz = bid % a.d_out;
  const int n = bid / a.d_out;
  const int m0 = mg * MB, r0 = rb * a.tr, c0 = cb * a.tc;
  const int rows = min(a.tr, a.h_out - r0), cols = min(a.tc, a.w_out - c0);
  const int sw = cols + 2, csp = band_stride(a.tr + 2, a.tc + 2), npos = rows * cols;

  int xoff[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int p = (wave * NTW + j) * 16 + (lane & 15);
    const int pp = p < npos ? p : 0;
    const int oh = pp / cols, ow = pp - oh * cols;
    xoff[j] = (lane >> 4) * csp + oh * sw + ow;
  }
  acc4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
  const bool busy = wave * NTW * 16 < npos;

  for (int kd = 0; kd < NKD; ++kd) {
    const int ds = SRC == SRC3_HORIZON ? dz : dz + kd - a.pd;
    if (SRC == SRC3_PLAIN && (ds < 0 || ds >= a.in.d_in)) continue;   // a padding slice: the same for the whole block
    const int wkd = (a.flip ? 1 - kd : kd) * 9;
    for (int k0 = 0; k0 < a.in.c_in; k0 += CC) {
      __syncthreads();   // the previous chunk's reads are done
      // weights: walk the global array along its contiguous axis, (c, tap) per m forward, (m, tap) per c mirrored
      for (int i = threadIdx.x; i < 9 * CC * MB; i += kBlock) {
        int ml, c, tap;
        if (a.flip) c = i / (MB * 9), ml = (i % (MB * 9)) / 9, tap = i % 9;
        else ml = i / (CC * 9), c = (i % (CC * 9)) / 9, tap = i % 9;
        const int m = m0 + ml, gc = k0 + c;
        const float v =
            (m < a.m_out && gc < a.in.c_in) ? a.w[(size_t)m * a.w_sm + (size_t)gc * a.w_sc + wkd + tap] : 0.0f;
        wl[((a.flip ? 8 - tap : tap) * CC + c) * MBP + ml] = v;
      }
      stage_rows3<SRC>(xl, a.in, n, ds, k0, CC, r0 - 1, rows + 2, c0 - 1, sw, sw, csp);
      __syncthreads();
      if (busy) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int toff = (tap / 3) * sw + (tap % 3);
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            float av[MT], bv[NTW];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = wl[(tap * CC + s * 4 + (lane >> 4)) * MBP + mt * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < NTW; ++j) bv[j] = xl[xoff[j] + s * 4 * csp + toff];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
              for (int j = 0; j < NTW; ++j)
                acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[j], acc[mt][j], 0, 0, 0);
          }
        }
      }
    }
  }

  if (!busy) return;
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int p = (wave * NTW + j) * 16 + (lane & 15);
    if (p >= npos) continue;
    const int oh = p / cols, ow = p - oh * cols;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + mt * 16 + (lane >> 4) * 4 + i;
        if (m < a.m_out) {
          const size_t off = ((((size_t)n * a.m_out + m) * a.d_out + dz) * a.h_out + r0 + oh) * a.w_out + c0 + ow;
          float v = acc[mt][j][i] + (a.bias ? a.bias[m] : 0.0f);
          if (a.relu) v = v > 0.0f ? v : 0.0f;
          if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
          a.y[off] = v;
        }
      }
  }
}

// wgrad.  Block = (slab, chunk of 14 input channels, depth tap); D[co][col] over every position of the slab's tiles, col =
// ci * 9 + tap (local to the chunk) for col < 126, col 126 a column of ones (dbias, chunk 0 only), col 127 zero.  An item is
// (image, output slice, row band, column band); an item whose source slice d + kd - pd is padding is skipped.  dbias needs
// every item once, so an item's ones column belongs to depth tap 0, or to depth tap 1 where tap 0's source is padding
// (output slice 0 under depth padding 1; tap 1 then reads slice 0, which exists): no block visits an item for the bias alone
// (that would give those blocks 3 items for the others' 2 under depth padding 1, and a launch lasts as long as its slowest
// block).  Tap 0's sum goes to the slab's bias column, tap 1's to bias1[slab], which
// bias1_add adds to dbias after the slab sum.  Tiles and k-steps as in conv2d_wide_f32.hip's wide_wgrad.  A slab row is
// [c_in][nkd][9] + the bias column: the layout of a [c_out][c_in][nkd][3][3] weight.
struct Wg3 {
  In3 in;                   // layer input
  In3 dy;                   // pre-activation gradient (SRC3_PLAIN with its gate), c_in = c_out of the layer, d_in = d_out
  float* slabs;             // [n_slabs][c_out][c_in * nkd * 9 + 1]
  float* bias1;             // [n_slabs][c_out] (depth padding 1 only): the bias partial of the depth tap 1 blocks
  int pd, nkd, d_out, h_out, w_out, tr, tc, n_rb, n_cb, items, per;
};

// dbias[co] += bias1[0][co] + bias1[1][co] + ... in slab order
__global__ __launch_bounds__(kBlock) void bias1_add(const float* __restrict__ bias1, float* __restrict__ db, int c_out,
                                                    int n_slabs) {
  const int co = blockIdx.x * kBlock + threadIdx.x;
  if (co >= c_out) return;
  float s = 0.0f;
  for (int i = 0; i < n_slabs; ++i) s += bias1[(size_t)i * c_out + co];
  db[co] += s;
}

template <int SRC, int MT>
__global__ __launch_bounds__(kBlock) void wide3_wgrad(Wg3 q) {
  constexpr int NTW = kWgNTW, CC = kWgCC, DPS = kWgDps, M = MT * 16;
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slab = blockIdx.x, chunk = blockIdx.y, kd = blockIdx.z, ci0 = chunk * CC;
  const int sw = q.tc + 2, cs = (q.tr + 2) * sw;
  float* xl = lds;                     // [CC][cs]
  float* dl = xl + CC * cs;            // [M][DPS]
  int* xo = (int*)(dl + M * DPS);      // [DPS]

  int coff[NTW];
  float bmul[NTW], badd[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave * NTW + j) * 16 + (lane & 15);
    const bool real = col < CC * 9 && ci0 + col / 9 < q.in.c_in;
    const int ci = real ? col / 9 : 0, tap = real ? col % 9 : 0;
    coff[j] = ci * cs + (tap / 3) * sw + tap % 3;
    bmul[j] = real ? 1.0f : 0.0f;
    badd[j] = col == CC * 9 ? 1.0f : 0.0f;
  }
  acc4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};

  const int it0 = slab * q.per, it1 = min(it0 + q.per, q.items);
  for (int it = it0; it < it1; ++it) {
    int rest = it;
    const int cb = rest % q.n_cb; rest /= q.n_cb;
    const int rb = rest % q.n_rb; rest /= q.n_rb;
    const int dz = rest % q.d_out;
    const int n = rest / q.d_out;
    const int ds = SRC == SRC3_HORIZON ? dz : dz + kd - q.pd;
    if (SRC == SRC3_PLAIN && (ds < 0 || ds >= q.in.d_in)) continue;   // a padding slice: the same for the whole block
    const int bias_kd = (SRC == SRC3_PLAIN && dz < q.pd) ? 1 : 0;
    const float ones = (chunk == 0 && kd == bias_kd) ? 1.0f : 0.0f;
    const int r0 = rb * q.tr, c0 = cb * q.tc;
    const int rows = min(q.tr, q.h_out - r0), cols = min(q.tc, q.w_out - c0), npos = rows * cols;
    __syncthreads();   // the previous item's reads are done
    stage_rows3<SRC>(xl, q.in, n, ds, ci0, CC, r0 - 1, q.tr + 2, c0 - 1, sw, sw, cs);
    // dy rows [co][oh] of the tile, packed to cols per row; the (up to 3) positions that round the tile to a k-step: 0
    stage_rows3<SRC3_PLAIN>(dl, q.dy, n, dz, 0, M, r0, rows, c0, cols, cols, DPS);
    for (int i = threadIdx.x; i < M * 4; i += kBlock) {
      const int p = npos + (i & 3);
      if (p < DPS) dl[(i >> 2) * DPS + p] = 0.0f;
    }
    for (int p = threadIdx.x; p < DPS; p += kBlock) {
      const int oh = p / cols, ow = p - oh * cols;
      xo[p] = p < npos ? oh * sw + ow : 0;
    }
    __syncthreads();
    const int steps = (npos + 3) / 4;
    for (int s = 0; s < steps; ++s) {
      const int p = s * 4 + (lane >> 4);
      const int xoff = xo[p];
      float av[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) av[mt] = dl[(mt * 16 + (lane & 15)) * DPS + p];
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        const float b = xl[coff[j] + xoff] * bmul[j] + badd[j] * ones;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt][j], 0, 0, 0);
      }
    }
  }
  // this slab's partial sums of the chunk's columns: row co = mt * 16 + (lane / 16) * 4 + i
  const int ncols = q.in.c_in * q.nkd * 9 + 1;
  float* out = q.slabs + (size_t)slab * M * ncols;
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave * NTW + j) * 16 + (lane & 15);
    int gcol = -1;
    if (col < CC * 9 && ci0 + col / 9 < q.in.c_in) gcol = ((ci0 + col / 9) * q.nkd + kd) * 9 + col % 9;
    else if (col == CC * 9 && chunk == 0 && kd == 0) gcol = ncols - 1;
    else if (col == CC * 9 && chunk == 0 && q.bias1) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) q.bias1[(size_t)slab * M + mt * 16 + (lane >> 4) * 4 + i] = acc[mt][j][i];
    }
    if (gcol < 0) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[(size_t)(mt * 16 + (lane >> 4) * 4 + i) * ncols + gcol] = acc[mt][j][i];
  }
}

// ---- the stride-2 head: 3x3, stride 2, padding 1, one output channel -------------------------------------------------------
// x [n][c_in][h][w] -> y [n][1][ho][wo], ho = (h - 1) / 2 + 1; output (oh, ow) reads rows 2 oh - 1 + kh, columns 2 ow - 1 + kw.
// The three kernels are those of pv_conv2d_head_s2_* (conv2d_wide_f32.hip) at padding 1.
constexpr int kHeadPad = 1;

// forward: one output per thread; the 9 taps of a channel are one fma chain, the channels go round-robin into four partial
// sums added in a fixed order
__global__ __launch_bounds__(kBlock) void head_p1_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y, int total,
                                                      int c_in, int h, int wi, int ho, int wo, int relu) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int ow = idx % wo, oh = (idx / wo) % ho, b = idx / (wo * ho);
  int off[9];
  bool ok[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int ir = 2 * oh - kHeadPad + t / 3, ic = 2 * ow - kHeadPad + t % 3;
    ok[t] = ir >= 0 && ir < h && ic >= 0 && ic < wi;
    off[t] = ok[t] ? ir * wi + ic : 0;
  }
  const size_t plane = (size_t)h * wi;
  const float* xb = x + (size_t)b * c_in * plane;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int ci = 0; ci < c_in; ++ci) {
    const float* xp = xb + ci * plane;
    const float* wp = w + ci * 9;
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) s = fmaf(wp[t], ok[t] ? xp[off[t]] : 0.0f, s);
    acc[ci & 3] += s;
  }
  float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + (bias ? bias[0] : 0.0f);
  if (relu) v = v > 0.0f ? v : 0.0f;
  y[idx] = v;
}

// data gradient: every dx element is written once, from the at most four taps of its parity class.  Block = (1024 elements
// of a plane, input channel, image): the channel's nine weights are uniform over the block, one division per element
constexpr int kHeadDxPerBlock = 4 * kBlock;
__global__ __launch_bounds__(kBlock) void head_p1_bwd_data(const float* __restrict__ dy, const float* __restrict__ w,
                                                           float* __restrict__ dx, const float* __restrict__ x_gate,
                                                           int c_in, int h, int wi, int ho, int wo) {
  const int ci = blockIdx.y, b = blockIdx.z, plane = h * wi;
  const float* dyb = dy + (size_t)b * ho * wo;
  const float* wp = w + ci * 9;
  const size_t base = ((size_t)b * c_in + ci) * plane;
  const int p1 = min(plane, (int)(blockIdx.x + 1) * kHeadDxPerBlock);
  for (int p = blockIdx.x * kHeadDxPerBlock + threadIdx.x; p < p1; p += kBlock) {
    const int r = p / wi, c = p - r * wi;
    float s = 0.0f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int tr = r + kHeadPad - kh;
      if (tr < 0 || (tr & 1) || (tr >> 1) >= ho) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tc = c + kHeadPad - kw;
        if (tc < 0 || (tc & 1) || (tc >> 1) >= wo) continue;
        s = fmaf(wp[kh * 3 + kw], dyb[(tr >> 1) * wo + (tc >> 1)], s);
      }
    }
    if (x_gate && !(x_gate[base + p] > 0.0f)) s = 0.0f;
    dx[base + p] = s;
  }
}

// weight / bias gradient.  Block = (input channel, slab of (image, band of 16 output rows) items); every thread sums its
// positions' nine products (and dy itself), then the block adds the threads' sums in a fixed tree.  slabs [n_slabs][c_in *
// 9 + 1], the last column the bias gradient (written by channel 0).
constexpr int kHeadBand = 16, kHeadMaxSlabs = 128;

__global__ __launch_bounds__(kBlock) void head_p1_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                        float* __restrict__ slabs, int c_in, int h, int wi, int ho, int wo,
                                                        int n_rb, int items, int per) {
  __shared__ float part[kBlock / 64][10];
  const int ci = blockIdx.x, slab = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float a[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) a[t] = 0.0f;
  const int it0 = slab * per, it1 = min(it0 + per, items);
  for (int it = it0; it < it1; ++it) {
    const int rb = it % n_rb, b = it / n_rb;
    const int oh0 = rb * kHeadBand, rows = min(kHeadBand, ho - oh0);
    const float* xp = x + ((size_t)b * c_in + ci) * h * wi;
    const float* dyb = dy + (size_t)b * ho * wo;
    for (int p = threadIdx.x; p < rows * wo; p += kBlock) {
      const int oh = oh0 + p / wo, ow = p % wo;
      const float g = dyb[oh * wo + ow];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ir = 2 * oh - kHeadPad + t / 3, ic = 2 * ow - kHeadPad + t % 3;
        const float v = (ir >= 0 && ir < h && ic >= 0 && ic < wi) ? xp[ir * wi + ic] : 0.0f;
        a[t] = fmaf(g, v, a[t]);
      }
      a[9] += g;
    }
  }
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    float v = a[t];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if (lane == 0) part[wave][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int t = threadIdx.x;
    const float v = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    const int ncols = c_in * 9 + 1;
    if (t < 9) slabs[(size_t)slab * ncols + ci * 9 + t] = v;
    else if (ci == 0) slabs[(size_t)slab * ncols + ncols - 1] = v;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

size_t fwd_lds_bytes(int tr, int tc) {
  return ((size_t)9 * kCC * kMBP + (size_t)kCC * band_stride(tr + 2, tc + 2)) * sizeof(float);
}

// forward tile: up to 62 columns x (256 / columns, at most 64) rows, bands of equal size
void fwd_tiles(Fwd3& a) {
  a.n_cb = (a.w_out + kMaxTc - 1) / kMaxTc;
  a.tc = (a.w_out + a.n_cb - 1) / a.n_cb;
  a.tr = std::max(1, std::min(std::min(a.h_out, kMaxTr), kPos / a.tc));
  a.n_rb = (a.h_out + a.tr - 1) / a.tr;
  a.tr = (a.h_out + a.n_rb - 1) / a.n_rb;
  a.n_mg = (a.m_out + kMB - 1) / kMB;
}

struct WgPlan {
  int d_out, h_out, w_out, tr, tc, n_rb, n_cb, items, n_chunks, nkd, n_slabs, per;
  size_t lds, ws, ws_slabs;
};

// c_in: the channels the kernel stages (4 pseudo-channels for the horizon layer, with nkd = 1)
WgPlan wg_plan(int n, int c_in, int nkd, int c_out, int d_out, int h_out, int w_out, int pad_d) {
  WgPlan p;
  p.d_out = d_out, p.h_out = h_out, p.w_out = w_out, p.nkd = nkd;
  p.n_cb = (w_out + kWgMaxTc - 1) / kWgMaxTc;
  p.tc = (w_out + p.n_cb - 1) / p.n_cb;
  p.tr = std::max(1, std::min(std::min(h_out, kWgMaxTr), kWgPos / p.tc));
  p.n_rb = (h_out + p.tr - 1) / p.tr;
  p.tr = (h_out + p.n_rb - 1) / p.n_rb;
  p.items = n * d_out * p.n_rb * p.n_cb;
  p.n_chunks = (c_in + kWgCC - 1) / kWgCC;
  // fixed slabs: at most kMaxWgBlocks blocks over (slab, chunk, kd); 128 -> 128: 25 slabs x 1.18 MB = 30 MB
  const int want = std::max(1, std::min(p.items, kMaxWgBlocks / (p.n_chunks * nkd)));
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  p.lds = ((size_t)kWgCC * (p.tr + 2) * (p.tc + 2) + (size_t)c_out * kWgDps) * sizeof(float) + kWgDps * sizeof(int);
  p.ws_slabs = (size_t)p.n_slabs * c_out * (c_in * nkd * 9 + 1) * sizeof(float);
  p.ws = p.ws_slabs + (pad_d ? (size_t)p.n_slabs * c_out * sizeof(float) : 0);      // + bias1
  return p;
}

// extents of a (2, 3, 3) stride-1 conv with spatial padding 1 and 32-bit indexing of every tensor
int check_wide3_dims(const char* who, int n, int c_in, int c_out, int d_in, int h_in, int w_in, int pad_d, int pad_hw) {
  PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && d_in > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(pad_d == 0 || pad_d == 1, PV_ESIZE, "%s: unsupported depth padding %d (0 or 1)", who, pad_d);
  PV_REQUIRE(pad_hw == 1, PV_ESIZE, "%s: unsupported spatial padding %d (1)", who, pad_hw);
  PV_REQUIRE(d_in + 2 * pad_d - 1 >= 1, PV_ESIZE, "%s: depth %d shorter than the 2-slice kernel", who, d_in);
  PV_REQUIRE(w_in <= kMaxW, PV_ESIZE, "%s: planes wider than %d columns are not supported (w_in=%d)", who, kMaxW, w_in);
  const long long depth = std::max(d_in, d_in + 2 * pad_d - 1);
  PV_REQUIRE((long long)n * std::max(c_in, c_out) * depth * h_in * w_in < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

int check_wide3(const char* who, int n, int c_in, int c_out, int d_in, int h_in, int w_in, int pad_d, int pad_hw) {
  int rc = check_wide3_dims(who, n, c_in, c_out, d_in, h_in, w_in, pad_d, pad_hw);
  if (rc) return rc;
  PV_REQUIRE((c_in == 64 || c_in == 128) && c_out == 128, PV_ESIZE,
             "%s: unsupported channel counts c_in=%d c_out=%d ((64 | 128) -> 128)", who, c_in, c_out);
  return PV_OK;
}

int check_horizon(const char* who, int n, int d_in, int h, int w, int c_out) {
  PV_REQUIRE(c_out == 64, PV_ESIZE, "%s: unsupported channel count c_out=%d (64)", who, c_out);
  return check_wide3_dims(who, n, 2, c_out, d_in, h, w, 0, 1);
}

inline In3 plain_in3(const float* x, const float* gate, int c, int d, int h, int w) {
  In3 s = {};
  s.x = x, s.gate = gate, s.c_in = c, s.d_in = d, s.h = h, s.w = w;
  return s;
}

inline In3 horizon_in3(const float* history, const float* horizon, int d, int h, int w) {
  In3 s = {};
  s.x = history, s.horizon = horizon, s.c_in = 4, s.d_in = d, s.h = h, s.w = w;
  return s;
}

template <int SRC>
int run_fwd(const char* who, Fwd3 a, int n, hipStream_t st) {
  fwd_tiles(a);
  const long long blocks = (long long)n * a.d_out * a.n_rb * a.n_cb * a.n_mg;
  PV_REQUIRE(blocks < (1LL << 31), PV_ESIZE, "%s: grid beyond 2^31 blocks", who);
  wide3_fwd<SRC><<<dim3((unsigned)blocks), dim3(kBlock), fwd_lds_bytes(a.tr, a.tc), st>>>(a);
  return check_launch(who);
}

template <int SRC>
int run_wgrad(const char* who, const In3& in, const In3& dy, int pd, const WgPlan& p, float* dw, float* db, void* ws,
              size_t ws_bytes, hipStream_t st) {
  int rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  Wg3 q;
  q.in = in, q.dy = dy, q.slabs = (float*)ws, q.pd = pd, q.nkd = p.nkd;
  q.bias1 = pd ? (float*)((char*)ws + p.ws_slabs) : nullptr;
  q.d_out = p.d_out, q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per;
  const dim3 grid((unsigned)p.n_slabs, (unsigned)p.n_chunks, (unsigned)p.nkd), block(kBlock);
  if (dy.c_in == 64) wide3_wgrad<SRC, 4><<<grid, block, p.lds, st>>>(q);
  else wide3_wgrad<SRC, 8><<<grid, block, p.lds, st>>>(q);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, db, dy.c_in, in.c_in * p.nkd * 9, p.n_slabs, st);
  rc = check_launch(who);
  if (rc || !q.bias1) return rc;
  bias1_add<<<dim3((unsigned)((dy.c_in + kBlock - 1) / kBlock)), dim3(kBlock), 0, st>>>(q.bias1, db, dy.c_in, p.n_slabs);
  return check_launch(who);
}

// the head: ho x wo outputs, every tensor within 32-bit indexing
int check_head(const char* who, int n, int c_in, int c_out, int h_in, int w_in) {
  PV_REQUIRE(n > 0 && c_in > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(c_out == 1, PV_ESIZE, "%s: unsupported channel count c_out=%d (1)", who, c_out);
  PV_REQUIRE((long long)n * c_in * h_in * w_in < (1LL << 31), PV_ESIZE, "%s: tensor beyond 2^31 elements (32-bit indexing)",
             who);
  return PV_OK;
}

inline int head_out(int side) { return (side - 1) / 2 + 1; }

struct HeadPlan {
  int ho, wo, n_rb, items, per, n_slabs;
  size_t ws;
};

HeadPlan head_plan(int n, int c_in, int h, int w) {
  HeadPlan p;
  p.ho = head_out(h), p.wo = head_out(w);
  p.n_rb = (p.ho + kHeadBand - 1) / kHeadBand;
  p.items = n * p.n_rb;
  const int want = std::min(p.items, kHeadMaxSlabs);
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  p.ws = (size_t)p.n_slabs * (c_in * 9 + 1) * sizeof(float);
  return p;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv3d_wide_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                           int32_t c_out, int32_t d_in, int32_t h_in, int32_t w_in, int32_t pad_d, int32_t pad_hw,
                           int32_t relu, void* stream) {
  const char* who = "pv_conv3d_wide_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide3(who, n, c_in, c_out, d_in, h_in, w_in, pad_d, pad_hw);
  if (rc) return rc;
  Fwd3 a = {};
  a.in = plain_in3(x, nullptr, c_in, d_in, h_in, w_in);
  a.w = w, a.bias = bias, a.y = y;
  a.m_out = c_out, a.pd = pad_d, a.d_out = d_in + 2 * pad_d - 1, a.h_out = h_in, a.w_out = w_in;
  a.w_sm = c_in * 18, a.w_sc = 18, a.flip = 0, a.relu = relu ? 1 : 0;
  return run_fwd<SRC3_PLAIN>(who, a, n, as_stream(stream));
}

int pv_conv3d_wide_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                int32_t n, int32_t c_in, int32_t c_out, int32_t d_in, int32_t h_in, int32_t w_in,
                                int32_t pad_d, int32_t pad_hw, void* stream) {
  const char* who = "pv_conv3d_wide_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide3(who, n, c_in, c_out, d_in, h_in, w_in, pad_d, pad_hw);
  if (rc) return rc;
  // the forward of dy [n][c_out][d_in + 2 pad_d - 1][h][w] with depth padding 1 - pad_d (spatial padding 2 - 1 = 1), weights
  // mirrored in all three axes with the channel roles swapped
  Fwd3 a = {};
  a.in = plain_in3(dy, dy_gate, c_out, d_in + 2 * pad_d - 1, h_in, w_in);
  a.w = w, a.y = dx, a.out_gate = x_gate;
  a.m_out = c_in, a.pd = 1 - pad_d, a.d_out = d_in, a.h_out = h_in, a.w_out = w_in;
  a.w_sm = 18, a.w_sc = c_in * 18, a.flip = 1, a.relu = 0;
  return run_fwd<SRC3_PLAIN>(who, a, n, as_stream(stream));
}

int pv_conv3d_wide_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t d_in, int32_t h_in,
                                              int32_t w_in, int32_t pad_d, int32_t pad_hw, size_t* bytes) {
  const char* who = "pv_conv3d_wide_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide3(who, n, c_in, c_out, d_in, h_in, w_in, pad_d, pad_hw);
  if (rc) return rc;
  *bytes = wg_plan(n, c_in, 2, c_out, d_in + 2 * pad_d - 1, h_in, w_in, pad_d).ws;
  return PV_OK;
}

int pv_conv3d_wide_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                  int32_t n, int32_t c_in, int32_t c_out, int32_t d_in, int32_t h_in, int32_t w_in,
                                  int32_t pad_d, int32_t pad_hw, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv3d_wide_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide3(who, n, c_in, c_out, d_in, h_in, w_in, pad_d, pad_hw);
  if (rc) return rc;
  const int d_out = d_in + 2 * pad_d - 1;
  const WgPlan p = wg_plan(n, c_in, 2, c_out, d_out, h_in, w_in, pad_d);
  return run_wgrad<SRC3_PLAIN>(who, plain_in3(x, nullptr, c_in, d_in, h_in, w_in),
                               plain_in3(dy, dy_gate, c_out, d_out, h_in, w_in), pad_d, p, dw, dbias, ws, ws_bytes,
                               as_stream(stream));
}

int pv_conv3d_wide_horizon_fwd_f32(const float* history, const float* horizon, const float* w, const float* bias, float* y,
                                   int32_t n, int32_t d_in, int32_t h, int32_t w_img, int32_t c_out, void* stream) {
  const char* who = "pv_conv3d_wide_horizon_fwd_f32";
  PV_REQUIRE(history && horizon && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, d_in, h, w_img, c_out);
  if (rc) return rc;
  Fwd3 a = {};
  a.in = horizon_in3(history, horizon, d_in, h, w_img);
  a.w = w, a.bias = bias, a.y = y;
  a.m_out = c_out, a.pd = 0, a.d_out = d_in - 1, a.h_out = h, a.w_out = w_img;
  a.w_sm = 36, a.w_sc = 9, a.flip = 0, a.relu = 1;
  return run_fwd<SRC3_HORIZON>(who, a, n, as_stream(stream));
}

int pv_conv3d_wide_horizon_bwd_weight_workspace_bytes(int32_t n, int32_t d_in, int32_t h, int32_t w_img, int32_t c_out,
                                                      size_t* bytes) {
  const char* who = "pv_conv3d_wide_horizon_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, d_in, h, w_img, c_out);
  if (rc) return rc;
  *bytes = wg_plan(n, 4, 1, c_out, d_in - 1, h, w_img, 0).ws;
  return PV_OK;
}

int pv_conv3d_wide_horizon_bwd_weight_f32(const float* history, const float* horizon, const float* dy, float* dw,
                                          float* dbias, int32_t n, int32_t d_in, int32_t h, int32_t w_img, int32_t c_out,
                                          void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv3d_wide_horizon_bwd_weight_f32";
  PV_REQUIRE(history && horizon && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, d_in, h, w_img, c_out);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, 4, 1, c_out, d_in - 1, h, w_img, 0);
  return run_wgrad<SRC3_HORIZON>(who, horizon_in3(history, horizon, d_in, h, w_img),
                                 plain_in3(dy, nullptr, c_out, d_in - 1, h, w_img), 0, p, dw, dbias, ws, ws_bytes,
                                 as_stream(stream));
}

int pv_conv2d_head_s2p1_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                                int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_head_s2p1_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  const int ho = head_out(h_in), wo = head_out(w_in), total = n * ho * wo;
  head_p1_fwd<<<dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream)>>>(
      x, w, bias, y, total, c_in, h_in, w_in, ho, wo, relu ? 1 : 0);
  return check_launch(who);
}

int pv_conv2d_head_s2p1_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                     int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_head_s2p1_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(!dy_gate, PV_EINVAL, "%s: the head has no ReLU, so it takes no dy_gate", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(c_in <= 65535 && n <= 65535, PV_ESIZE, "%s: more than 65535 channels or images (grid axes)", who);
  head_p1_bwd_data<<<dim3((unsigned)((h_in * w_in + kHeadDxPerBlock - 1) / kHeadDxPerBlock), (unsigned)c_in, (unsigned)n),
                     dim3(kBlock), 0, as_stream(stream)>>>(dy, w, dx, x_gate, c_in, h_in, w_in, head_out(h_in),
                                                           head_out(w_in));
  return check_launch(who);
}

int pv_conv2d_head_s2p1_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                   size_t* bytes) {
  const char* who = "pv_conv2d_head_s2p1_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  *bytes = head_plan(n, c_in, h_in, w_in).ws;
  return PV_OK;
}

int pv_conv2d_head_s2p1_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                       int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                       size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_head_s2p1_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(!dy_gate, PV_EINVAL, "%s: the head has no ReLU, so it takes no dy_gate", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  const HeadPlan p = head_plan(n, c_in, h_in, w_in);
  rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  head_p1_wgrad<<<dim3((unsigned)c_in, (unsigned)p.n_slabs), dim3(kBlock), 0, st>>>(x, dy, (float*)ws, c_in, h_in, w_in,
                                                                                      p.ho, p.wo, p.n_rb, p.items, p.per);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, dbias, 1, c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

}  // extern "C"
