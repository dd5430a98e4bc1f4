// What the three exact-f32 64 / 128-channel MFMA conv files share: conv2d_wide_f32.hip (notebook 10, stride 1),
// conv2d_wide_s2_f32.hip (notebook 09, stride 2) and conv3d_wide_f32.hip (notebook 12, kernel (2, 3, 3)).  Every pass is an
// implicit GEMM over LDS tiles with K streamed in channel chunks (v_mfma_f32_16x16x4_f32).  This header holds
//   the layout constants and band_stride;
//   stage_rows: the row-per-wave band staging of the two stride-1 files, over a load functor;
//   the stride-1 forward / dgrad tile in four steps (fwd_band, fwd_stage_weights, fwd_multiply, fwd_store), which
//   wide_fwd calls inside its chunk loop and wide3_fwd inside its depth-tap and chunk loops;
//   the weight-gradient tile of all three files at position stride 1 or 2 (wg_columns, wg_item_tail, wg_ksteps, wg_store);
//   the host side they repeat: fwd_tiles, wg_tiles, check_wide_channels, check_stripe_args.
// The __global__ kernels, their item decode, their sources and what only one family does (the 3-D ones factor and bias1,
// the stride-2 early-out, the stride-2 gather / scatter with their parity layouts) stay in the three files.
// LDS images are laid out against bank conflicts of the 32-lane read groups: the weight rows [tap][c] are 80 floats apart
// and the input channel stride is 16 mod 32, so the two k-rows a half wave reads fall on disjoint banks; the staged dy rows
// of the weight gradient are DPS = positions + 2 floats apart (2 mod 32).
#pragma once
#include "conv2d_f32_common.h"

namespace pv {
namespace {

// forward / dgrad: 4 x 16 output channels per block, 8 input channels per chunk, weight rows padded to 80 floats
constexpr int kMT = 4, kMB = kMT * 16, kMBP = kMB + 16, kCC = 8;
// wgrad: 14 input channels per chunk -> 126 (ci, tap) columns + a ones column + a zero column = 8 tiles, 2 per wave
constexpr int kWgCC = 14, kWgNTW = 2;
constexpr int kMaxW = 128;                   // widest plane of the wide families
// the stride-1 tiles: 4 x 16 positions per wave (256 per block); the staged band is at most 64 columns (one lane each)
// x 66 rows; wgrad tiles of at most 96 positions, 48 columns, 32 rows, dealt to at most 512 blocks
constexpr int kNTW = 4, kPos = 4 * kNTW * 16, kMaxTc = 62, kMaxTr = 64;
constexpr int kWg1Pos = 96, kWg1Dps = kWg1Pos + 2, kWg1MaxTc = 48, kWg1MaxTr = 32, kWg1MaxBlocks = 512;

// channel stride of a staged band: >= rows * sw and 16 mod 32
__host__ __device__ inline int band_stride(int rows, int sw) {
  const int cs = rows * sw;
  return cs + ((16 - cs % 32) + 32) % 32;
}

template <int MT, int NTW>
__device__ __forceinline__ void zero_acc(acc4 (&acc)[MT][NTW]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
}

// Stage channels [c0, c0 + cc) x rows [r0, r0 + rows) x columns [col0, col0 + cols) of a c_in x h x w source as lds[c * cs +
// r * sw + col]; outside the source (padding), beyond c_in and where the whole band's source does not exist (!exists): 0.
// load(ch, r, c) reads inside the source.  One row per wave and pass, one column per lane: cols <= 64.
template <class Load>
__device__ __forceinline__ void stage_rows(float* lds, Load load, bool exists, int c_in, int h, int w, int c0, int cc,
                                           int r0, int rows, int col0, int cols, int sw, int cs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ic = col0 + lane;
  const bool ok = ic >= 0 && ic < w && exists;
  if (lane >= cols) return;
  int ch = 0, r = wave;
  while (r >= rows) r -= rows, ++ch;
  while (ch < cc) {
    const int gc = c0 + ch, ir = r0 + r;
    float v = 0.0f;
    if (ok && gc < c_in && ir >= 0 && ir < h) v = load(gc, ir, ic);
    lds[ch * cs + r * sw + lane] = v;
    r += 4;
    while (r >= rows) r -= rows, ++ch;
  }
}

// ---- the stride-1 forward / dgrad tile ---------------------------------------------------------------------------------------
// A is the family's argument struct: w, bias, y, out_gate, m_out, h_out, w_out, tr, tc, w_sm, w_sc, flip, relu.  The band is
// tr x tc output positions (<= 256) flattened row-major, wave w takes the 16-position tiles 4 w .. 4 w + 3.  LDS: weights
// wl [9][kCC][kMBP], input band xl [kCC][csp] of (tr + 2) x (tc + 2).  Per chunk of 8 input channels the caller stages the
// weights and the band, then 18 k-steps each read 4 A and 4 B values and issue 16 MFMAs.  The steps take A and the band by
// value: through a reference to the kernel-argument struct the compiler kept 12 more AGPRs in wide_fwd.
struct FwdBand {
  int m0, r0, c0, rows, cols, sw, csp, npos;
  bool busy;               // this wave holds a position
};

// the block's band and the wave's positions in it: xoff[j] = offset of tile j's position in xl (k-row of the lane included)
template <class A>
__device__ __forceinline__ FwdBand fwd_band(const A a, int rb, int cb, int mg, int (&xoff)[kNTW], acc4 (&acc)[kMT][kNTW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  FwdBand t;
  t.m0 = mg * kMB, t.r0 = rb * a.tr, t.c0 = cb * a.tc;
  t.rows = min(a.tr, a.h_out - t.r0), t.cols = min(a.tc, a.w_out - t.c0);
  t.sw = t.cols + 2, t.csp = band_stride(a.tr + 2, a.tc + 2), t.npos = t.rows * t.cols;
#pragma unroll
  for (int j = 0; j < kNTW; ++j) {
    const int p = (wave * kNTW + j) * 16 + (lane & 15);
    const int pp = p < t.npos ? p : 0;
    const int oh = pp / t.cols, ow = pp - oh * t.cols;
    xoff[j] = (lane >> 4) * t.csp + oh * t.sw + ow;
  }
  zero_acc(acc);
  t.busy = wave * kNTW * 16 < t.npos;
  return t;
}

// one chunk of weights, wl[tap][c][m] of channels [k0, k0 + 8) x outputs [m0, m0 + 64), from w + wbase: the global array is
// walked along its contiguous axis, (c, tap) per m forward, (m, tap) per c mirrored (flip: tap 8 - tap, channel roles swapped)
template <class A>
__device__ __forceinline__ void fwd_stage_weights(float* wl, const A a, int c_in, int m0, int k0, int wbase) {
  for (int i = threadIdx.x; i < 9 * kCC * kMB; i += kBlock) {
    int ml, c, tap;
    if (a.flip) c = i / (kMB * 9), ml = (i % (kMB * 9)) / 9, tap = i % 9;
    else ml = i / (kCC * 9), c = (i % (kCC * 9)) / 9, tap = i % 9;
    const int m = m0 + ml, gc = k0 + c;
    const float v = (m < a.m_out && gc < c_in) ? a.w[(size_t)m * a.w_sm + (size_t)gc * a.w_sc + wbase + tap] : 0.0f;
    wl[((a.flip ? 8 - tap : tap) * kCC + c) * kMBP + ml] = v;
  }
}

// the staged chunk times the staged band: 9 taps x 2 k-steps x 16 MFMAs
__device__ __forceinline__ void fwd_multiply(const float* wl, const float* xl, const FwdBand t, const int (&xoff)[kNTW],
                                             acc4 (&acc)[kMT][kNTW]) {
  constexpr int KS = kCC / 4;
  const int lane = threadIdx.x & 63;
  if (!t.busy) return;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int toff = (tap / 3) * t.sw + (tap % 3);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      float av[kMT], bv[kNTW];
#pragma unroll
      for (int mt = 0; mt < kMT; ++mt) av[mt] = wl[(tap * kCC + s * 4 + (lane >> 4)) * kMBP + mt * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < kNTW; ++j) bv[j] = xl[xoff[j] + s * 4 * t.csp + toff];
#pragma unroll
      for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
        for (int j = 0; j < kNTW; ++j) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[j], acc[mt][j], 0, 0, 0);
    }
  }
}

// bias, ReLU, out_gate and the store: y is [n][m_out][planes][h_out][w_out], the block writes plane `slice` of image n
template <class A>
__device__ __forceinline__ void fwd_store(const A a, const FwdBand t, int n, int planes, int slice,
                                          const acc4 (&acc)[kMT][kNTW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (!t.busy) return;
#pragma unroll
  for (int j = 0; j < kNTW; ++j) {
    const int p = (wave * kNTW + j) * 16 + (lane & 15);
    if (p >= t.npos) continue;
    const int oh = p / t.cols, ow = p - oh * t.cols;
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = t.m0 + mt * 16 + (lane >> 4) * 4 + i;
        if (m < a.m_out) {
          const size_t off = ((((size_t)n * a.m_out + m) * planes + slice) * a.h_out + t.r0 + oh) * a.w_out + t.c0 + ow;
          float v = acc[mt][j][i] + (a.bias ? a.bias[m] : 0.0f);
          if (a.relu) v = v > 0.0f ? v : 0.0f;
          if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
          a.y[off] = v;
        }
      }
  }
}

// ---- the weight-gradient tile ----------------------------------------------------------------------------------------------
// D[m][col] over every position of a block's items, col = ci * 9 + tap (local to the chunk of 14 sliding channels from ci0)
// for col < 126, col 126 a column of ones (the bias gradient), col 127 zero.  Wave w owns the 16-column tiles 2 w, 2 w + 1
// against all MT row tiles; a k-step is 4 positions (A: 16 rows x 4 positions; B: 4 positions x 16 columns).  Per item the
// caller stages the sliding band xl [14][cs] (rows sw apart) and the row operand dl [M][DPS] packed to cols per row; xo[pos]
// is the position's offset in the band, STRIDE (1 or 2) band elements per position step.

// the wave's columns: coff = the column's (channel, tap) offset in the band, bmul = 1 on a real column, badd = 1 on the ones
// column
__device__ __forceinline__ void wg_columns(int ci0, int c_in, int cs, int sw, int (&coff)[kWgNTW], float (&bmul)[kWgNTW],
                                           float (&badd)[kWgNTW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kWgNTW; ++j) {
    const int col = (wave * kWgNTW + j) * 16 + (lane & 15);
    const bool real = col < kWgCC * 9 && ci0 + col / 9 < c_in;
    const int ci = real ? col / 9 : 0, tap = real ? col % 9 : 0;
    coff[j] = ci * cs + (tap / 3) * sw + tap % 3;
    bmul[j] = real ? 1.0f : 0.0f;
    badd[j] = col == kWgCC * 9 ? 1.0f : 0.0f;
  }
}

// after the item's dl rows are staged: the (up to 3) positions that round the tile to a k-step are 0, and the xo table
template <int MT, int STRIDE, int DPS>
__device__ __forceinline__ void wg_item_tail(float* dl, int* xo, int npos, int cols, int sw) {
  for (int i = threadIdx.x; i < MT * 16 * 4; i += kBlock) {
    const int p = npos + (i & 3);
    if (p < DPS) dl[(i >> 2) * DPS + p] = 0.0f;
  }
  for (int p = threadIdx.x; p < DPS; p += kBlock) {
    const int oh = p / cols, ow = p - oh * cols;
    xo[p] = p < npos ? STRIDE * oh * sw + STRIDE * ow : 0;
  }
}

// the item's k-steps; the ones column counts `ones` (1, or 0 where this block does not own the item's bias gradient)
template <int MT, int DPS>
__device__ __forceinline__ void wg_ksteps(const float* xl, const float* dl, const int* xo, int npos,
                                          const int (&coff)[kWgNTW], const float (&bmul)[kWgNTW],
                                          const float (&badd)[kWgNTW], float ones, acc4 (&acc)[MT][kWgNTW]) {
  const int lane = threadIdx.x & 63;
  const int steps = (npos + 3) / 4;
  for (int s = 0; s < steps; ++s) {
    const int p = s * 4 + (lane >> 4);
    const int xoff = xo[p];
    float av[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) av[mt] = dl[(mt * 16 + (lane & 15)) * DPS + p];
#pragma unroll
    for (int j = 0; j < kWgNTW; ++j) {
      const float b = xl[coff[j] + xoff] * bmul[j] + badd[j] * ones;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt][j], 0, 0, 0);
    }
  }
}

// the block's partial sums into its slab out [M][ncols]: row = mt * 16 + (lane / 16) * 4 + i; a real column goes to
// gcol(col), the ones column to the last one where `bias` (the block owns the slab's bias column), else to side [M] where
// the family has such a side output (null: it is dropped)
template <int MT, class GCol>
__device__ __forceinline__ void wg_store(float* out, int ncols, int ci0, int c_in, bool bias, float* side, GCol gcol,
                                         const acc4 (&acc)[MT][kWgNTW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kWgNTW; ++j) {
    const int col = (wave * kWgNTW + j) * 16 + (lane & 15);
    int g = -1;
    if (col < kWgCC * 9 && ci0 + col / 9 < c_in) g = gcol(col);
    else if (col == kWgCC * 9 && bias) g = ncols - 1;
    else if (col == kWgCC * 9 && side) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) side[mt * 16 + (lane >> 4) * 4 + i] = acc[mt][j][i];
    }
    if (g < 0) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[(size_t)(mt * 16 + (lane >> 4) * 4 + i) * ncols + g] = acc[mt][j][i];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

inline size_t wide_fwd_lds_bytes(int tr, int tc) {
  return ((size_t)9 * kCC * kMBP + (size_t)kCC * band_stride(tr + 2, tc + 2)) * sizeof(float);
}

// stride-1 forward tile: up to 62 columns x (256 / columns, at most 64) rows, bands of equal size
struct FwdTiles {
  int tr, tc, n_rb, n_cb, n_mg;
};

inline FwdTiles fwd_tiles(int m_out, int h_out, int w_out) {
  FwdTiles t;
  t.n_cb = (w_out + kMaxTc - 1) / kMaxTc;
  t.tc = (w_out + t.n_cb - 1) / t.n_cb;
  t.tr = std::max(1, std::min(std::min(h_out, kMaxTr), kPos / t.tc));
  t.n_rb = (h_out + t.tr - 1) / t.tr;
  t.tr = (h_out + t.n_rb - 1) / t.n_rb;
  t.n_mg = (m_out + kMB - 1) / kMB;
  return t;
}

// Weight-gradient tiles over `planes` h_out x w_out position grids (images, or images x output slices): tiles of at most
// max_tc columns, max_tr rows and max_pos positions, bands of equal size; the items (plane, row band, column band) are dealt
// to fixed slabs, at most max_blocks blocks over (slab, chunk of 14 of the c sliding channels, the family's blocks_per_chunk).
struct WgTiles {
  int h_out, w_out, tr, tc, n_rb, n_cb, items, n_chunks, n_slabs, per;
};

inline WgTiles wg_tiles(int planes, int c, int h_out, int w_out, int max_tc, int max_tr, int max_pos, int max_blocks,
                        int blocks_per_chunk) {
  WgTiles p;
  p.h_out = h_out, p.w_out = w_out;
  p.n_cb = (w_out + max_tc - 1) / max_tc;
  p.tc = (w_out + p.n_cb - 1) / p.n_cb;
  p.tr = std::max(1, std::min(std::min(h_out, max_tr), max_pos / p.tc));
  p.n_rb = (h_out + p.tr - 1) / p.tr;
  p.tr = (h_out + p.n_rb - 1) / p.n_rb;
  p.items = planes * p.n_rb * p.n_cb;
  p.n_chunks = (c + kWgCC - 1) / kWgCC;
  const int want = std::max(1, std::min(p.items, max_blocks / (p.n_chunks * blocks_per_chunk)));
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  return p;
}

inline int check_wide_channels(const char* who, int c_in, int c_out) {
  PV_REQUIRE((c_in == 64 || c_in == 128) && c_out == 128, PV_ESIZE,
             "%s: unsupported channel counts c_in=%d c_out=%d ((64 | 128) -> 128)", who, c_in, c_out);
  return PV_OK;
}

}  // namespace
}  // namespace pv
