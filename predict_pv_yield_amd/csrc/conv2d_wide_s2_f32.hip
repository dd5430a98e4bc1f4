// The stride-2 Conv2d / ConvTranspose2d autoencoder of notebooks/09_horizon_represented_as_a_stripe.ipynb (the
// LitAutoEncoder cell, raw lines 1356-1416 of the .ipynb file: encoder_conv = Conv2d 5 -> 64 -> 128 -> 128, all 3x3 stride 2,
// at 1366-1370; decoder_conv = ConvTranspose2d 128 -> 128 -> 128 stride 2 and 128 -> 1 stride 1 at 1375-1379; the stripe plane
// at 1382-1395; the loss at 1402-1403) in exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per product,
// f32 accumulation).  Planes are up to 128 wide on the wide side (a Conv2d's input, a ConvTranspose2d's output).
//
// The passes are the three forms of conv2d_s2_f32.hip, but 64 / 128-channel weights (up to 590 KB) do not fit the VGPRs, so K
// is streamed through LDS in channel chunks as in conv2d_wide_f32.hip (the chunk layout, band_stride and the whole
// weight-gradient tile of form C are conv_wide_f32.h's; forms A and B keep their own loops and parity layouts):
//   A  strided gather   D[m][oh][ow] = sum_{tap, c} W[m][c][tap] X[c][2 oh + kh][2 ow + kw]
//      Conv2d forward (also the stripe first layer); ConvTranspose2d data gradient (over dy, weights [c_in][c_out] read as
//      [m][c], unmirrored).  Per chunk of 8 channels the (2 tr + 1) x (2 tc + 1) band is staged split by column parity (even
//      columns, then odd columns of a row), so each kw tap is a unit-stride read over the 16 positions of an MFMA tile.
//   B  parity-class scatter   Y[m][2 i + kh][2 j + kw] += W[c][m][tap] X[c][i][j]
//      ConvTranspose2d forward; Conv2d data gradient (over dy, weights [c_out][c_in] read as [c][m]).  The output splits by
//      (row parity, column parity) into four stride-1 sub-convolutions over the class grid (a, b) -> (2 a + pr, 2 b + pc) with
//      4, 2, 2 and 1 taps.  A block owns tr x tc class-grid positions of all four classes (up to 2 tr x 2 tc outputs); a 16
//      -position MFMA tile holds positions of one class and issues only that class's taps: 9 tap products per 2 x 2 output
//      quad, no staged zeros of an upsampled plane.  The source band is staged plain with one row / column of halo before it.
//      Every output element belongs to one class and is written once; where no tap reaches a source (the last row / column
//      of an even-sized Conv2d input) the staged zeros give exactly 0.
//   C  strided weight gradient   D[m][(c, tap)] = sum_pos G[m][pos] X[c][2 pos + tap]  (+ a ones column)
//      Conv2d: G = dy, X = x, the ones column is the bias gradient.  ConvTranspose2d: G = x, X = dy, so D[ci][(co, tap)] is
//      the [c_in][c_out][3][3] layout as it stands; its ones column is not stored and the bias gradient (sums of dy over all
//      of its positions) is a plane sum in slabs of its own.  Block = (slab of tiles, chunk of 14 sliding channels); slabs
//      are cut across images and tiles, so small planes still fill the device.  Fixed slabs, added in slab order by the
//      shared conv2d_slab_sum_f32: no atomics, identical bits run to run.
// The model's last layer, the one-output-channel ConvTranspose2d head pv_convt2d_head_*, is in conv2d_head_f32.hip.
// pv_mse_pred_window_f32 is the loss over a window of the prediction.
#include "conv2d_stripe_f32.h"
#include "conv_wide_f32.h"

namespace pv {
namespace {

// A / B: the 4 x 16 output channels per block, 8 input channels per chunk and 80-float weight rows of conv_wide_f32.h; here
// the taps are 644 floats apart (4 mod 32), so the nine taps of one (c, m), which neighbouring threads stage, fall on
// different banks
constexpr int kTapStride = kCC * kMBP + 4;
constexpr int kWPer = 9 * kCC * kMB / 256;   // weights per thread and chunk (18)
constexpr int kBandSlots = 6;                // B: elements of the staged source band per thread and chunk
constexpr int kWantBlocks = 512;             // two blocks per CU: below this the planner takes smaller tiles
// C: the 14-channel chunks of conv_wide_f32.h over tiles of at most 64 positions and 24 columns
constexpr int kWgPos = 64, kWgDps = kWgPos + 2, kWgMaxTc = 24;
constexpr size_t kLdsBytes = 64 * 1024;    // per block: every tile below is planned inside it
constexpr int kMaxWgBlocks = 768;            // three blocks per CU

inline int conv_out(int s) { return (s - 3) / 2 + 1; }

// Stage channels [c0, c0 + cc) x rows [r0, r0 + rows) x columns [col0, col0 + ncols) of image n as lds[ch * cs + r * sw +
// slot]; outside the image and beyond c_in: 0.  slot = the column's offset, or with SPLIT the even offsets first (offset / 2)
// and the odd ones from eoff on.  Lanes run along columns; narrow bands put 2 or 4 rows on a wave.
template <int SRC, bool SPLIT>
__device__ __forceinline__ void stage_band(float* lds, const In& s, const Stripe& sp, int n, int c0, int cc, int r0,
                                           int rows, int col0, int ncols, int sw, int cs, int eoff) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sh = ncols <= 16 ? 4 : ncols <= 32 ? 5 : 6;
  const int lc = lane & ((1 << sh) - 1), rp = 64 >> sh, total = cc * rows;
  for (int i = wave * rp + (lane >> sh); i < total; i += 4 * rp) {
    const int ch = i / rows, r = i - ch * rows;
    const int gc = c0 + ch, ir = r0 + r;
    const bool row_ok = gc < s.c_in && ir >= 0 && ir < s.h;
    float* dst = lds + ch * cs + r * sw;
    for (int col = lc; col < ncols; col += 1 << sh) {
      const int ic = col0 + col;
      float v = 0.0f;
      if (row_ok && ic >= 0 && ic < s.w) v = load_in<SRC>(s, sp, n, gc, ir, ic);
      dst[SPLIT ? ((col & 1) ? eoff + (col >> 1) : (col >> 1)) : col] = v;
    }
  }
}

struct Fwd {
  In in;
  Stripe sp;
  const float* w;          // element (m, c, tap) at w[m * w_sm + c * w_sc + tap]
  const float* bias;       // [m_out] or null
  float* y;                // [n][m_out][h_out][w_out]
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int m_out, h_out, w_out, tr, tc, n_rb, n_cb, n_mg, w_sm, w_sc, cm, relu;   // cm: weights stored [c][m] (w_sm = 9)
};

// One chunk of weights, wl[tap][c][m], through registers: the global array is walked along its contiguous axis, and the
// next chunk's loads are in flight while the current chunk is multiplied.
__device__ __forceinline__ void weight_slot(const Fwd& a, int j, int& tap, int& c, int& ml) {
  const int i = threadIdx.x + j * kBlock;
  tap = i % 9;
  if (a.cm) c = i / (kMB * 9), ml = (i / 9) % kMB;
  else ml = i / (kCC * 9), c = (i / 9) % kCC;
}

__device__ __forceinline__ void load_weights(float (&wr)[kWPer], const Fwd& a, int m0, int k0) {
#pragma unroll
  for (int j = 0; j < kWPer; ++j) {
    int tap, c, ml;
    weight_slot(a, j, tap, c, ml);
    const int m = m0 + ml, gc = k0 + c;
    wr[j] = (m < a.m_out && gc < a.in.c_in) ? a.w[(size_t)m * a.w_sm + (size_t)gc * a.w_sc + tap] : 0.0f;
  }
}

__device__ __forceinline__ void store_weights(float* wl, const float (&wr)[kWPer], const Fwd& a) {
#pragma unroll
  for (int j = 0; j < kWPer; ++j) {
    int tap, c, ml;
    weight_slot(a, j, tap, c, ml);
    wl[tap * kTapStride + c * kMBP + ml] = wr[j];
  }
}

__device__ __forceinline__ void store_out(const Fwd& a, int n, int m, int r, int c, float v) {
  const size_t off = (((size_t)n * a.m_out + m) * a.h_out + r) * a.w_out + c;
  v += a.bias ? a.bias[m] : 0.0f;
  if (a.relu) v = v > 0.0f ? v : 0.0f;
  if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
  a.y[off] = v;
}

__device__ __forceinline__ void block_coords(const Fwd& a, int& n, int& rb, int& cb, int& mg) {
  int bid = blockIdx.x;
  mg = bid % a.n_mg; bid /= a.n_mg;
  cb = bid % a.n_cb; bid /= a.n_cb;
  rb = bid % a.n_rb;
  n = bid / a.n_rb;
}

// A.  Block = (image, row band, column band, group of 64 output channels); the band is tr x tc output positions (<= 64 NTW)
// flattened row-major, wave w takes the 16-position tiles NTW w .. NTW w + NTW - 1.
template <int SRC, int NTW>
__global__ __launch_bounds__(kBlock) void wide_s2_gather(Fwd a) {
  constexpr int MT = kMT, CC = kCC, KS = CC / 4, MBP = kMBP;
  extern __shared__ float lds[];
  float* wl = lds;                     // [9][kTapStride]: [tap][CC][MBP]
  float* xl = lds + 9 * kTapStride;    // [CC][csp], a row = tc + 1 even columns, then tc odd columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n, rb, cb, mg;
  block_coords(a, n, rb, cb, mg);
  const int m0 = mg * kMB, r0 = rb * a.tr, c0 = cb * a.tc;
  const int rows = min(a.tr, a.h_out - r0), cols = min(a.tc, a.w_out - c0), npos = rows * cols;
  const int sw = 2 * a.tc + 1, eoff = a.tc + 1, csp = band_stride(2 * a.tr + 1, sw);

  int xoff[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int p = (wave * NTW + j) * 16 + (lane & 15);
    const int pp = p < npos ? p : 0;
    const int oh = pp / cols, ow = pp - oh * cols;
    xoff[j] = (lane >> 4) * csp + 2 * oh * sw + ow;
  }
  acc4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
  const int live = min(NTW, (npos - wave * NTW * 16 + 15) / 16);   // this wave's tiles that hold a position (may be <= 0)

  float wr[kWPer];
  load_weights(wr, a, m0, 0);
  for (int k0 = 0; k0 < a.in.c_in; k0 += CC) {
    __syncthreads();   // the previous chunk's reads are done
    store_weights(wl, wr, a);
    stage_band<SRC, true>(xl, a.in, a.sp, n, k0, CC, 2 * r0, 2 * rows + 1, 2 * c0, 2 * cols + 1, sw, csp, eoff);
    __syncthreads();
    if (k0 + CC < a.in.c_in) load_weights(wr, a, m0, k0 + CC);
    if (live <= 0) continue;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kw = tap % 3;
      const int toff = (tap / 3) * sw + (kw == 1 ? eoff : kw >> 1);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        float av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = wl[tap * kTapStride + (s * 4 + (lane >> 4)) * MBP + mt * 16 + (lane & 15)];
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          if (j >= live) continue;
          const float b = xl[xoff[j] + s * 4 * csp + toff];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt][j], 0, 0, 0);
        }
      }
    }
  }

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
        if (m < a.m_out) store_out(a, n, m, r0 + oh, c0 + ow, acc[mt][j][i]);
      }
  }
}

// B.  Block = (image, row band, column band, group of 64 output channels) of tr x tc class-grid positions (<= 64 NT): each
// class has at most 4 NT tiles, wave w takes tiles NT w .. NT w + NT - 1 of every class.  The source rows [a0 - 1, a0 + tr)
// and columns [b0 - 1, b0 + tc) are staged as xl[ch][tr + 1][tc + 1] (zero outside the source) through registers: a thread
// owns up to kBandSlots elements of the band, whose offsets it works out once, and loads the next chunk's while the current
// chunk is multiplied.  The source has a multiple of 8 channels.
template <int NT>
__global__ __launch_bounds__(kBlock) void wide_s2_scatter(Fwd a) {
  constexpr int MT = kMT, CC = kCC, KS = CC / 4, MBP = kMBP;
  extern __shared__ float lds[];
  float* wl = lds;                     // [9][kTapStride]: [tap][CC][MBP]
  float* xl = lds + 9 * kTapStride;    // [CC][cs]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n, rb, cb, mg;
  block_coords(a, n, rb, cb, mg);
  const int m0 = mg * kMB, a0 = rb * a.tr, b0 = cb * a.tc;
  const int sw = a.tc + 1, cs = band_stride(a.tr + 1, sw);

  // this thread's elements of the band: offset in a chunk of the source (-1: outside the source) and in xl (-1: no element)
  int goff[kBandSlots], loff[kBandSlots];
  {
    const int band = (a.tr + 1) * sw;
#pragma unroll
    for (int j = 0; j < kBandSlots; ++j) {
      const int e = threadIdx.x + j * kBlock;
      const int ch = e / band, rem = e - ch * band;
      const int r = rem / sw, col = rem - r * sw;
      const int ir = a0 - 1 + r, ic = b0 - 1 + col;
      const bool has = ch < CC;
      loff[j] = has ? ch * cs + r * sw + col : -1;
      goff[j] = (has && ir >= 0 && ir < a.in.h && ic >= 0 && ic < a.in.w) ? (ch * a.in.h + ir) * a.in.w + ic : -1;
    }
  }
  const size_t chunk_elems = (size_t)CC * a.in.h * a.in.w;
  const float* xn = a.in.x + (size_t)n * a.in.c_in * a.in.h * a.in.w;
  const float* gn = a.in.gate ? a.in.gate + (size_t)n * a.in.c_in * a.in.h * a.in.w : nullptr;
  auto load_band = [&](float (&br)[kBandSlots], int k0) {
    const size_t base = (size_t)(k0 / CC) * chunk_elems;
#pragma unroll
    for (int j = 0; j < kBandSlots; ++j) {
      float v = 0.0f;
      if (goff[j] >= 0) {
        v = xn[base + goff[j]];
        if (gn && !(gn[base + goff[j]] > 0.0f)) v = 0.0f;
      }
      br[j] = v;
    }
  };

  // class cl = 2 pr + pc: its positions inside the block are those with 2 a + pr < h_out, 2 b + pc < w_out
  int soff[4][NT], npos[4], ccols[4];
#pragma unroll
  for (int cl = 0; cl < 4; ++cl) {
    const int pr = cl >> 1, pc = cl & 1;
    const int rows = max(0, min(a.tr, (a.h_out - pr + 1) / 2 - a0)), cols = max(0, min(a.tc, (a.w_out - pc + 1) / 2 - b0));
    npos[cl] = rows * cols, ccols[cl] = max(cols, 1);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int p = (wave * NT + t) * 16 + (lane & 15);
      const int pp = p < npos[cl] ? p : 0;
      const int la = pp / ccols[cl], lb = pp - la * ccols[cl];
      soff[cl][t] = (lane >> 4) * cs + (la + 1) * sw + lb + 1;
    }
  }
  acc4 acc[4][NT][MT];
#pragma unroll
  for (int cl = 0; cl < 4; ++cl)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[cl][t][mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};

  float wr[kWPer], br[kBandSlots];
  load_weights(wr, a, m0, 0);
  load_band(br, 0);
  for (int k0 = 0; k0 < a.in.c_in; k0 += CC) {
    __syncthreads();   // the previous chunk's reads are done
    store_weights(wl, wr, a);
#pragma unroll
    for (int j = 0; j < kBandSlots; ++j)
      if (loff[j] >= 0) xl[loff[j]] = br[j];
    __syncthreads();
    if (k0 + CC < a.in.c_in) {
      load_weights(wr, a, m0, k0 + CC);
      load_band(br, k0 + CC);
    }
#pragma unroll
    for (int cl = 0; cl < 4; ++cl) {
      if (wave * NT * 16 >= npos[cl]) continue;   // none of this wave's tiles of the class holds a position
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap % 3;
        if ((kh & 1) != (cl >> 1) || (kw & 1) != (cl & 1)) continue;
        const int toff = (kh >> 1) * sw + (kw >> 1);   // source (a - kh / 2, b - kw / 2)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          float av[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) av[mt] = wl[tap * kTapStride + (s * 4 + (lane >> 4)) * MBP + mt * 16 + (lane & 15)];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if ((wave * NT + t) * 16 >= npos[cl]) continue;
            const float b = xl[soff[cl][t] + s * 4 * cs - toff];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              acc[cl][t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[cl][t][mt], 0, 0, 0);
          }
        }
      }
    }
  }

#pragma unroll
  for (int cl = 0; cl < 4; ++cl)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int p = (wave * NT + t) * 16 + (lane & 15);
      if (p >= npos[cl]) continue;
      const int la = p / ccols[cl], lb = p - la * ccols[cl];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m0 + mt * 16 + (lane >> 4) * 4 + i;
          if (m < a.m_out) store_out(a, n, m, 2 * (a0 + la) + (cl >> 1), 2 * (b0 + lb) + (cl & 1), acc[cl][t][mt][i]);
        }
    }
}

// C.  Block = (slab, chunk of 14 sliding channels) over the slab's items (image, row band, column band); the tile is that of
// conv_wide_f32.h at position stride 2, its ones column written by chunk 0.  The tile's G lives in LDS as [M][66] (zero
// beyond the tile), the sliding operand as [14][2 tr + 1][2 tc + 1].
struct Wg {
  In in;                    // the sliding operand (SRC_PLAIN with its gate, or SRC_STRIPE)
  Stripe sp;
  In g;                     // the D rows' operand over the position grid (SRC_PLAIN with its gate), c_in = M
  float* slabs;             // [n_slabs][M][in.c_in * 9 + 1]
  int h_out, w_out, tr, tc, n_rb, n_cb, items, per;
};

template <int SRC, int MT>
__global__ __launch_bounds__(kBlock) void wide_s2_wgrad(Wg q) {
  constexpr int CC = kWgCC, DPS = kWgDps, M = MT * 16;
  extern __shared__ float lds[];
  const int slab = blockIdx.x, chunk = blockIdx.y, ci0 = chunk * CC;
  const int sw = 2 * q.tc + 1, cs = (2 * q.tr + 1) * sw;
  float* xl = lds;                     // [CC][cs]
  float* dl = xl + CC * cs;            // [M][DPS]
  int* xo = (int*)(dl + M * DPS);      // [DPS]
  const Stripe none = {};

  int coff[kWgNTW];
  float bmul[kWgNTW], badd[kWgNTW];
  wg_columns(ci0, q.in.c_in, cs, sw, coff, bmul, badd);
  bool any = false;                    // a wave whose 32 columns are all padding only stages
#pragma unroll
  for (int j = 0; j < kWgNTW; ++j) any = any || bmul[j] != 0.0f || badd[j] != 0.0f;
  any = __any(any);
  acc4 acc[MT][kWgNTW];
  zero_acc(acc);

  const int it0 = slab * q.per, it1 = min(it0 + q.per, q.items);
  for (int it = it0; it < it1; ++it) {
    const int cb = it % q.n_cb, rb = (it / q.n_cb) % q.n_rb, n = it / (q.n_cb * q.n_rb);
    const int r0 = rb * q.tr, c0 = cb * q.tc;
    const int rows = min(q.tr, q.h_out - r0), cols = min(q.tc, q.w_out - c0), npos = rows * cols;
    __syncthreads();   // the previous item's reads are done
    stage_band<SRC, false>(xl, q.in, q.sp, n, ci0, CC, 2 * r0, 2 * q.tr + 1, 2 * c0, sw, sw, cs, 0);
    // G rows [m][oh] of the tile, packed to cols per row
    stage_band<SRC_PLAIN, false>(dl, q.g, none, n, 0, M, r0, rows, c0, cols, cols, DPS, 0);
    wg_item_tail<MT, 2, DPS>(dl, xo, npos, cols, sw);
    __syncthreads();
    if (!any) continue;
    wg_ksteps<MT, DPS>(xl, dl, xo, npos, coff, bmul, badd, 1.0f, acc);
  }
  const int ncols = q.in.c_in * 9 + 1;
  wg_store<MT>(q.slabs + (size_t)slab * M * ncols, ncols, ci0, q.in.c_in, chunk == 0, nullptr,
               [&](int col) { return ci0 * 9 + col; }, acc);
}

// The ConvTranspose2d bias gradient's slabs: block (channel, slab) adds dy (zeroed where the gate <= 0) over the channel's
// planes of the slab's images: strided partial sums per thread, then a tree sum in LDS (fixed order).  slabs [n_slabs][c].
__global__ __launch_bounds__(kBlock) void plane_sum_slabs(const float* __restrict__ dy, const float* __restrict__ gate,
                                                         float* __restrict__ slabs, int n, int per, int c, int plane) {
  __shared__ float part[kBlock];
  const int ch = blockIdx.x, n0 = blockIdx.y * per, n1 = min(n0 + per, n);
  float s = 0.0f;
  for (int img = n0; img < n1; ++img) {
    const size_t base = ((size_t)img * c + ch) * plane;
    for (int i = threadIdx.x; i < plane; i += kBlock) {
      const float v = dy[base + i];
      s += (gate && !(gate[base + i] > 0.0f)) ? 0.0f : v;
    }
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) slabs[(size_t)blockIdx.y * c + ch] = part[0];
}

// ---- the loss over a window of the prediction ------------------------------------------------------------------------------
// block = example: squared differences over the window (strided partial sums per thread, a tree sum in LDS), the gradient
// everywhere on y_hat (exactly 0 outside the window)
__global__ __launch_bounds__(kBlock) void mse_pred_window_partial(const float* __restrict__ y_hat,
                                                                 const float* __restrict__ target, int oh, int ow, int th,
                                                                 int tw, int row0, int col0, float inv_count,
                                                                 float* __restrict__ dy_hat, float* __restrict__ partials) {
  __shared__ float part[kBlock];
  const int b = blockIdx.x, tot = oh * ow;
  float s = 0.0f;
  for (int i = threadIdx.x; i < tot; i += kBlock) {
    const int r = i / ow - row0, c = i % ow - col0;
    float g = 0.0f;
    if (r >= 0 && r < th && c >= 0 && c < tw) {
      const float d = y_hat[(size_t)b * tot + i] - target[((size_t)b * th + r) * tw + c];
      g = 2.0f * d * inv_count;
      s += d * d;
    }
    if (dy_hat) dy_hat[(size_t)b * tot + i] = g;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[b] = part[0];
}

// the per-example sums added in index order
__global__ void mse_pred_window_final(const float* __restrict__ partials, int n, float inv_count, float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float s = 0.0f;
  for (int i = 0; i < n; ++i) s += partials[i];
  loss[0] = s * inv_count;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

size_t fwd_lds_bytes(int band_rows, int band_sw) {
  return ((size_t)9 * kTapStride + (size_t)kCC * band_stride(band_rows, band_sw)) * sizeof(float);
}

// A: bands of at most 32 output columns (65 staged), 64 rows and 64 ntw positions, of equal size (at most 61 KB of LDS).  The planes are small (15 x 15 to
// 63 x 63), so the tile decides how many CUs are busy: from 256 positions per block down to 64 while the grid stays under
// kWantBlocks.
int gather_tiles(Fwd& a, int n) {
  a.n_cb = (a.w_out + 31) / 32;
  a.tc = (a.w_out + a.n_cb - 1) / a.n_cb;
  a.n_mg = (a.m_out + kMB - 1) / kMB;
  int ntw = 4;
  for (;; ntw >>= 1) {
    a.tr = std::max(1, std::min(std::min(a.h_out, 64), 64 * ntw / a.tc));
    a.n_rb = (a.h_out + a.tr - 1) / a.tr;
    a.tr = (a.h_out + a.n_rb - 1) / a.n_rb;
    if (ntw == 1 || (long long)n * a.n_rb * a.n_cb * a.n_mg >= kWantBlocks) return ntw;
  }
}

template <int SRC>
int run_gather(const char* who, Fwd a, int n, hipStream_t st) {
  const int ntw = gather_tiles(a, n);
  const long long blocks = (long long)n * a.n_rb * a.n_cb * a.n_mg;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  const size_t lds = fwd_lds_bytes(2 * a.tr + 1, 2 * a.tc + 1);
  PV_REQUIRE(lds <= kLdsBytes, PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, lds);
  const dim3 grid((unsigned)blocks), block(kBlock);
  if (ntw == 4) wide_s2_gather<SRC, 4><<<grid, block, lds, st>>>(a);
  else if (ntw == 2) wide_s2_gather<SRC, 2><<<grid, block, lds, st>>>(a);
  else wide_s2_gather<SRC, 1><<<grid, block, lds, st>>>(a);
  return check_launch(who);
}

// B: bands of at most 32 class columns, 32 class rows and 64 nt class positions (up to 4 x as many outputs), of equal size;
// 128 class positions per block where that still leaves kWantBlocks blocks.  The staged band, (tr + 1) x (tc + 1) x 8, is at
// most 165 x 8 elements: within kBandSlots per thread.
int run_scatter(const char* who, Fwd a, int n, hipStream_t st) {
  const int ga = (a.h_out + 1) / 2, gb = (a.w_out + 1) / 2;   // class grid of the even rows / columns (the larger one)
  a.n_cb = (gb + 31) / 32;
  a.tc = (gb + a.n_cb - 1) / a.n_cb;
  a.n_mg = (a.m_out + kMB - 1) / kMB;
  int nt = 2;
  for (;; nt >>= 1) {
    a.tr = std::max(1, std::min(std::min(ga, 32), 64 * nt / a.tc));
    a.n_rb = (ga + a.tr - 1) / a.tr;
    a.tr = (ga + a.n_rb - 1) / a.n_rb;
    if (nt == 1 || (long long)n * a.n_rb * a.n_cb * a.n_mg >= kWantBlocks) break;
  }
  const long long blocks = (long long)n * a.n_rb * a.n_cb * a.n_mg;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  const size_t lds = fwd_lds_bytes(a.tr + 1, a.tc + 1);
  PV_REQUIRE(a.in.c_in % kCC == 0 && kCC * (a.tr + 1) * (a.tc + 1) <= kBandSlots * kBlock, PV_ESIZE,
             "%s: source band of %d x %d x %d channels beyond the staging slots", who, a.tr + 1, a.tc + 1, a.in.c_in);
  PV_REQUIRE(lds <= kLdsBytes, PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, lds);
  const dim3 grid((unsigned)blocks), block(kBlock);
  if (nt == 2) wide_s2_scatter<2><<<grid, block, lds, st>>>(a);
  else wide_s2_scatter<1><<<grid, block, lds, st>>>(a);
  return check_launch(who);
}

// the gather form's Fwd: out [m_out] over the conv_out grid of a [c] x h_src x w_src source, weights stored [m_out][c][3][3]
Fwd gather_args(const float* w, const float* bias, float* y, int c, int m_out, int h_src, int w_src, int relu) {
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = m_out, a.h_out = conv_out(h_src), a.w_out = conv_out(w_src);
  a.w_sm = c * 9, a.w_sc = 9, a.cm = 0, a.relu = relu ? 1 : 0;
  return a;
}

// the scatter form's Fwd: out [m_out][h_out][w_out]; weights stored [c][m_out][3][3], taps as they stand
Fwd scatter_args(const float* w, const float* bias, float* y, int m_out, int h_out, int w_out, int relu) {
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = m_out, a.h_out = h_out, a.w_out = w_out;
  a.w_sm = 9, a.w_sc = m_out * 9, a.cm = 1, a.relu = relu ? 1 : 0;
  return a;
}

struct WgPlan : WgTiles {
  size_t lds, ws;
};

// C: (h_out, w_out) = the positions the sum runs over, rows = the D rows, c = the sliding operand's channels.  Tiles of at
// most 24 columns and 64 positions (at most 56 KB of LDS, so three blocks fit a CU); the items (image, row band, column band)
// are dealt to at most kMaxWgBlocks blocks over (slab, chunk), so a slab may hold a part of one image or several images.
WgPlan wg_plan(int n, int c, int rows, int h_out, int w_out) {
  WgPlan p;
  (WgTiles&)p = wg_tiles(n, c, h_out, w_out, kWgMaxTc, kWgPos, kWgPos, kMaxWgBlocks, 1);   // rows bounded by positions only
  p.lds = ((size_t)kWgCC * (2 * p.tr + 1) * (2 * p.tc + 1) + (size_t)rows * kWgDps) * sizeof(float) + kWgDps * sizeof(int);
  p.ws = (size_t)p.n_slabs * rows * (c * 9 + 1) * sizeof(float);
  return p;
}

// slabs into ws, then the ordered sum into dw [rows][c * 9] and (unless null) db [rows]
template <int SRC>
int run_wgrad(const char* who, const In& in, const Stripe& sp, const In& g, const WgPlan& p, float* dw, float* db, void* ws,
              hipStream_t st) {
  PV_REQUIRE(p.lds <= kLdsBytes, PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, p.lds);
  Wg q;
  q.in = in, q.sp = sp, q.g = g, q.slabs = (float*)ws;
  q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per;
  const dim3 grid((unsigned)p.n_slabs, (unsigned)p.n_chunks), block(kBlock);
  if (g.c_in == 64) wide_s2_wgrad<SRC, 4><<<grid, block, p.lds, st>>>(q);
  else wide_s2_wgrad<SRC, 8><<<grid, block, p.lds, st>>>(q);
  int rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, db, g.c_in, in.c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

enum Kind { KIND_CONV, KIND_CONVT };

// (h_in, w_in) = the extent of x, the layer's input
int check_dims(const char* who, int n, int c_in, int c_out, int h_in, int w_in, Kind kind) {
  if (kind == KIND_CONVT) {
    PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
    PV_REQUIRE(2 * w_in + 1 <= kMaxW, PV_ESIZE, "%s: output width %d beyond %d", who, 2 * w_in + 1, kMaxW);
    PV_REQUIRE((long long)n * std::max(c_in, c_out) * (2 * h_in + 1) * (2 * w_in + 1) < (1LL << 31), PV_ESIZE,
               "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
    return PV_OK;
  }
  int rc = check_conv_dims(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(w_in <= kMaxW, PV_ESIZE, "%s: width %d beyond %d", who, w_in, kMaxW);
  return PV_OK;
}

int check_ws2(const char* who, int n, int c_in, int c_out, int h_in, int w_in, Kind kind) {
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, kind);
  if (rc) return rc;
  if (kind == KIND_CONV) return check_wide_channels(who, c_in, c_out);
  PV_REQUIRE(c_in == 128 && c_out == 128, PV_ESIZE, "%s: unsupported channel counts c_in=%d c_out=%d (128 -> 128)", who,
             c_in, c_out);
  return PV_OK;
}

int check_stripe(const char* who, int n, int n_hist, int h, int w, int c_out, int stripe_width) {
  int rc = check_stripe_args(who, n_hist, c_out, stripe_width);
  if (rc) return rc;
  return check_dims(who, n, n_hist + 1, c_out, h, w, KIND_CONV);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the bias slabs of the ConvTranspose2d weight gradient: one per group of `per` images, at most 32
void bias_slabs(int n, int& n_slabs, int& per) {
  const int want = std::min(n, 32);
  per = (n + want - 1) / want;
  n_slabs = (n + per - 1) / per;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_wide_s2_stripe_fwd_f32(const float* history, const int32_t* stripe_start, const float* w, const float* bias,
                                     float* y, int32_t n, int32_t n_hist, int32_t h, int32_t w_img, int32_t c_out,
                                     int32_t stripe_width, void* stream) {
  const char* who = "pv_conv2d_wide_s2_stripe_fwd_f32";
  PV_REQUIRE(history && stripe_start && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_stripe(who, n, n_hist, h, w_img, c_out, stripe_width);
  if (rc) return rc;
  Fwd a = gather_args(w, bias, y, n_hist + 1, c_out, h, w_img, 1);
  a.in = stripe_in(history, n_hist, h, w_img);
  a.sp.start = stripe_start, a.sp.width = stripe_width, a.sp.n_hist = n_hist;
  return run_gather<SRC_STRIPE>(who, a, n, as_stream(stream));
}

int pv_conv2d_wide_s2_stripe_bwd_weight_f32(const float* history, const int32_t* stripe_start, const float* dy, float* dw,
                                            float* dbias, int32_t n, int32_t n_hist, int32_t h, int32_t w_img,
                                            int32_t c_out, int32_t stripe_width, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_wide_s2_stripe_bwd_weight_f32";
  PV_REQUIRE(history && stripe_start && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_stripe(who, n, n_hist, h, w_img, c_out, stripe_width);
  if (rc) return rc;
  const int ho = conv_out(h), wo = conv_out(w_img);
  const WgPlan p = wg_plan(n, n_hist + 1, c_out, ho, wo);
  rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  Stripe sp;
  sp.start = stripe_start, sp.width = stripe_width, sp.n_hist = n_hist;
  return run_wgrad<SRC_STRIPE>(who, stripe_in(history, n_hist, h, w_img), sp, plain_in(dy, nullptr, c_out, ho, wo), p, dw,
                               dbias, ws, as_stream(stream));
}

int pv_conv2d_wide_s2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                              int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_wide_s2_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  Fwd a = gather_args(w, bias, y, c_in, c_out, h_in, w_in, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  return run_gather<SRC_PLAIN>(who, a, n, as_stream(stream));
}

int pv_conv2d_wide_s2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                   int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_wide_s2_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  // the scatter of dy [n][c_out][ho][wo] with the weights [c_out][c_in][3][3] read as [c][m]
  Fwd a = scatter_args(w, nullptr, dx, c_in, h_in, w_in, 0);
  a.in = plain_in(dy, dy_gate, c_out, conv_out(h_in), conv_out(w_in));
  a.out_gate = x_gate;
  return run_scatter(who, a, n, as_stream(stream));
}

int pv_conv2d_wide_s2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                 size_t* bytes) {
  const char* who = "pv_conv2d_wide_s2_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  const bool wide = (c_in == 64 || c_in == 128) && c_out == 128;
  const bool stripe = c_in >= 2 && c_in <= kMaxHist + 1 && c_out == 64;
  PV_REQUIRE(wide || stripe, PV_ESIZE,
             "%s: unsupported channel counts c_in=%d c_out=%d ((64 | 128) -> 128, or n_hist + 1 -> 64)", who, c_in, c_out);
  *bytes = wg_plan(n, c_in, c_out, conv_out(h_in), conv_out(w_in)).ws;
  return PV_OK;
}

int pv_conv2d_wide_s2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                     int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                     size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_wide_s2_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  const int ho = conv_out(h_in), wo = conv_out(w_in);
  const WgPlan p = wg_plan(n, c_in, c_out, ho, wo);
  rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  const Stripe none = {};
  return run_wgrad<SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in), none, plain_in(dy, dy_gate, c_out, ho, wo), p, dw,
                              dbias, ws, as_stream(stream));
}

int pv_convt2d_wide_s2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                               int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_wide_s2_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  Fwd a = scatter_args(w, bias, y, c_out, 2 * h_in + 1, 2 * w_in + 1, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  return run_scatter(who, a, n, as_stream(stream));
}

int pv_convt2d_wide_s2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                    int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_convt2d_wide_s2_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  // a stride-2 valid conv of dy [n][c_out][2 h + 1][2 w + 1] with the unmirrored weights, [c_in][c_out][3][3] read as [m][c]
  Fwd a = gather_args(w, nullptr, dx, c_out, c_in, 2 * h_in + 1, 2 * w_in + 1, 0);
  a.in = plain_in(dy, dy_gate, c_out, 2 * h_in + 1, 2 * w_in + 1);
  a.out_gate = x_gate;
  return run_gather<SRC_PLAIN>(who, a, n, as_stream(stream));
}

int pv_convt2d_wide_s2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                  size_t* bytes) {
  const char* who = "pv_convt2d_wide_s2_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  int nb, per;
  bias_slabs(n, nb, per);
  *bytes = align256(wg_plan(n, c_out, c_in, h_in, w_in).ws) + (size_t)nb * c_out * sizeof(float);
  return PV_OK;
}

int pv_convt2d_wide_s2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                      int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                      size_t ws_bytes, void* stream) {
  const char* who = "pv_convt2d_wide_s2_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ws2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  // D[ci][(co, tap)] = sum_pos x[ci][pos] dy[co][2 pos + tap]: rows = c_in, the sliding operand is dy
  const WgPlan p = wg_plan(n, c_out, c_in, h_in, w_in);
  int nb, per;
  bias_slabs(n, nb, per);
  const size_t bias_off = align256(p.ws);
  rc = check_workspace(who, ws, ws_bytes, bias_off + (size_t)nb * c_out * sizeof(float));
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int ho = 2 * h_in + 1, wo = 2 * w_in + 1;
  const Stripe none = {};
  rc = run_wgrad<SRC_PLAIN>(who, plain_in(dy, dy_gate, c_out, ho, wo), none, plain_in(x, nullptr, c_in, h_in, w_in), p, dw,
                            nullptr, ws, st);
  if (rc) return rc;
  float* bslabs = (float*)((char*)ws + bias_off);
  plane_sum_slabs<<<dim3((unsigned)c_out, (unsigned)nb), dim3(kBlock), 0, st>>>(dy, dy_gate, bslabs, n, per, c_out, ho * wo);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(bslabs, nullptr, dbias, c_out, 0, nb, st);
  return check_launch(who);
}

int pv_mse_pred_window_f32(const float* y_hat, const float* target, int32_t n, int32_t out_h, int32_t out_w,
                           int32_t target_h, int32_t target_w, int32_t row0, int32_t col0, float* loss, float* dy_hat,
                           void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_mse_pred_window_f32";
  PV_REQUIRE(y_hat && target && loss, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(n > 0 && out_h > 0 && out_w > 0 && target_h > 0 && target_w > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(row0 >= 0 && col0 >= 0 && (long long)row0 + target_h <= out_h && (long long)col0 + target_w <= out_w, PV_ESIZE,
             "%s: the %d x %d window at (%d, %d) leaves the %d x %d prediction", who, target_h, target_w, row0, col0, out_h,
             out_w);
  PV_REQUIRE((long long)n * out_h * out_w < (1LL << 31), PV_ESIZE, "%s: tensor beyond 2^31 elements", who);
  int rc = check_workspace(who, ws, ws_bytes, (size_t)n * sizeof(float));
  if (rc) return rc;
  const float inv_count = (float)(1.0 / ((double)n * target_h * target_w));
  hipStream_t st = as_stream(stream);
  mse_pred_window_partial<<<dim3((unsigned)n), dim3(kBlock), 0, st>>>(y_hat, target, out_h, out_w, target_h, target_w, row0,
                                                                     col0, inv_count, dy_hat, (float*)ws);
  rc = check_launch(who);
  if (rc) return rc;
  mse_pred_window_final<<<dim3(1), dim3(64), 0, st>>>((const float*)ws, n, inv_count, loss);
  return check_launch(who);
}

}  // extern "C"
