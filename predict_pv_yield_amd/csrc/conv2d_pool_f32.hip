// Conv2d 3x3, stride 1, no padding, 144 output channels, in exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one
// rounding per product, f32 accumulation), with MaxPool2d(3) fused into the forward, for the image encoder of
// experiments/001_CNN_concat_all_timesteps_as_channels.py (sat_conv1..3 and maxpool at :241-245, the stacked-frame input
// with its five synthesised channels at :266-301, the conv / pool chain at :306-310).
//
// All passes are implicit GEMMs over a tile of output positions of one image staged in LDS, K streamed in channel chunks
// (conv2's weight alone is 746 KB, the LDS of a CU 160 KB):
//   forward / dgrad  D[m][pos]  = sum_{tap, c} A[m][(tap, c)] * X[c][pos + tap]    A = weights (chunk in LDS)
//   wgrad            D[co][col] = sum_{pos} dy[co][pos] * X[ci][pos + tap]          col = (ci, tap), plus a ones column
// Pooling.  relu(pool(z)) == pool(relu(z)), and a window whose maximum is <= 0 passes no gradient through either form, so
// the forward pools the pre-activations of a tile of whole 3x3 windows, applies ReLU to the maxima and writes the pooled
// value plus one byte per pooled output: the window position 0..8 of the first maximum in row-major order (where torch
// CPU's max_pool2d backward routes the gradient) or kDead when the maximum is <= 0.  Rows / columns beyond the last whole
// window (floor pooling) are neither computed nor given a gradient.  Backward passes read the pooled gradient and the
// codes and expand them to the pre-activation gradient while staging; that expansion is never stored.
// dgrad is the forward of the pre-activation gradient zero-padded by 2 with mirrored, channel-swapped weights; its
// epilogue may gate dx by the layer input (> 0).  The first layer reads frames 0..n_frames-1 of sat_data [B][T][H][W][1]
// in place and computes the five extra channels while staging (forward and weight gradient).  wgrad splits the tiles
// into fixed slabs, each block writing its partial sums to its own workspace slab, then adds the slabs in index order:
// no atomics, identical bits run to run.  The slab sum, the pooling rule (pool3_relu, pool3_expand), the input descriptor,
// the synthesised channels and the shared argument checks are in conv2d_f32_common.h.
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int kM = 144;       // output channels of every layer

// forward / dgrad tiles: MT 16-channel tiles of the output channels per block, NTW 16-position tiles per wave
constexpr int kFwdMT = 3, kFwdNTW = 2, kFwdCC = 12, kFwdPos = 4 * kFwdNTW * 16;   // 128 positions per block
// wgrad: CC input channels per chunk -> 126 (ci, tap) columns + a ones column + a zero column = 8 tiles, 2 per wave
constexpr int kWgCC = 14, kWgNTW = 2, kWgMT = kM / 16, kWgPos = 84;

// input channel ch (0 <= ch < c_in) of image n at (r, c), which the caller has checked lies inside [0, h) x [0, w).  SRC_SAT
// here: sat[b][t_total][h][w] frames 0..n_frames-1 stacked as channels, then the five synthesised channels.
template <int SRC>
__device__ __forceinline__ float load_in(const In& s, int n, int ch, int r, int c) {
  if (SRC == SRC_SAT) {
    if (ch < s.n_frames) return s.x[(((size_t)n * s.t_total + ch) * s.h + r) * s.w + c];
    // the channels of experiments/001...py:278-301.  The reference takes the centre and the pixel ramps from the row count
    // (`width`, :266-267) on both axes, so the centre is (h / 2, h / 2).
    return synth_channel(ch - s.n_frames, r, c, s.h / 2, s.h / 2, s.xc + (size_t)n * s.w, s.yc + (size_t)n * s.h);
  }
  return SRC == SRC_POOLED ? load_pooled(s, n, ch, r, c) : load_plain(s, n, ch, r, c);
}

// Stage channels [c0, c0 + cc) x rows [r0, r0 + rows) x columns [col0, col0 + cols) of image n as lds[c][r][col];
// outside the image (padding) and beyond c_in: 0.
template <int SRC>
__device__ void stage_in(float* lds, const In& s, int n, int c0, int cc, int r0, int rows, int col0, int cols) {
  const int tot = cc * rows * cols;
  for (int i = threadIdx.x; i < tot; i += kBlock) {
    const int col = i % cols, r = (i / cols) % rows, ch = i / (cols * rows);
    const int ir = r0 + r, ic = col0 + col, gc = c0 + ch;
    float v = 0.0f;
    if (gc < s.c_in && ir >= 0 && ir < s.h && ic >= 0 && ic < s.w) v = load_in<SRC>(s, n, gc, ir, ic);
    lds[i] = v;
  }
}

struct Fwd {
  In in;
  const float* w;          // element (m, c, tap) at w[m * w_sm + c * w_sc + (flip ? 8 - tap : tap)]
  const float* bias;       // [m_out] or null
  float* y;                // POOL: pooled [n][m_out][h_out / 3][w_out / 3]; else [n][m_out][h_out][w_out]
  uint8_t* codes;          // POOL: [n][m_out][h_out / 3][w_out / 3]
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int m_out, pad, h_out, w_out, tr, tc, n_rb, n_cb, n_mg, w_sm, w_sc, flip, relu;
};

// Forward / dgrad.  Block = (image, row band, column band, group of MT output-channel tiles); the band is tr x tc output
// positions (<= 128) flattened row-major, wave w takes the 16-position tiles w * NTW .. w * NTW + NTW - 1.  Per channel
// chunk of CC: the weights [tap][c][m] and the input band [c][tr + 2][tc + 2] are staged in LDS, then 9 * CC / 4 k-steps
// each read MT A values and NTW B values and issue MT * NTW MFMAs.  POOL: the pre-activations go to LDS (over the staged
// chunk) and every thread takes one (channel, window) of the tile: bias, max over the window in row-major order (first
// maximum wins), ReLU.
template <int SRC, bool POOL>
__global__ __launch_bounds__(kBlock) void conv144_fwd(Fwd a) {
  constexpr int MT = kFwdMT, NTW = kFwdNTW, CC = kFwdCC, KS = CC / 4, MB = MT * 16;
  extern __shared__ float lds[];
  float* wl = lds;                    // [9][CC][MB]
  float* xl = lds + 9 * CC * MB;      // [CC][tr + 2][tc + 2]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bid = blockIdx.x;
  const int mg = bid % a.n_mg; bid /= a.n_mg;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int n = bid / a.n_rb;
  const int m0 = mg * MB, r0 = rb * a.tr, c0 = cb * a.tc;
  const int rows = min(a.tr, a.h_out - r0), cols = min(a.tc, a.w_out - c0);
  const int sw = cols + 2, cs = (rows + 2) * sw, npos = rows * cols;

  int xoff[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int p = (wave * NTW + j) * 16 + (lane & 15);
    const int pp = p < npos ? p : 0;
    const int oh = pp / cols, ow = pp - oh * cols;
    xoff[j] = (lane >> 4) * cs + oh * sw + ow;
  }
  acc4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[mt][j] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
  const bool busy = wave * NTW * 16 < npos;

  for (int k0 = 0; k0 < a.in.c_in; k0 += CC) {
    __syncthreads();   // the previous chunk's reads are done
    for (int i = threadIdx.x; i < 9 * CC * MB; i += kBlock) {
      const int ml = i % MB, c = (i / MB) % CC, tap = i / (MB * CC);
      const int m = m0 + ml, gc = k0 + c;
      wl[i] = (m < a.m_out && gc < a.in.c_in) ? a.w[(size_t)m * a.w_sm + (size_t)gc * a.w_sc + (a.flip ? 8 - tap : tap)]
                                               : 0.0f;
    }
    stage_in<SRC>(xl, a.in, n, k0, CC, r0 - a.pad, rows + 2, c0 - a.pad, sw);
    __syncthreads();
    if (busy) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int toff = (tap / 3) * sw + (tap % 3);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          float av[MT], bv[NTW];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) av[mt] = wl[(tap * CC + s * 4 + (lane >> 4)) * MB + mt * 16 + (lane & 15)];
#pragma unroll
          for (int j = 0; j < NTW; ++j) bv[j] = xl[xoff[j] + s * 4 * cs + toff];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < NTW; ++j) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[j], acc[mt][j], 0, 0, 0);
        }
      }
    }
  }

  if (!POOL) {
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
            const size_t off = (((size_t)n * a.m_out + m) * a.h_out + r0 + oh) * a.w_out + c0 + ow;
            float v = acc[mt][j][i] + (a.bias ? a.bias[m] : 0.0f);
            if (a.relu) v = v > 0.0f ? v : 0.0f;
            if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
            a.y[off] = v;
          }
        }
    }
    return;
  }

  // POOL: pre-activations [MB][kFwdPos] over the staged chunk (fwd_lds_bytes sizes LDS for both), then one (channel,
  // window) per thread.  The tile is whole windows: rows == 3, cols a multiple of 3.
  __syncthreads();
  float* pre = lds;
  if (busy) {
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int p = (wave * NTW + j) * 16 + (lane & 15);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[(mt * 16 + (lane >> 4) * 4 + i) * kFwdPos + p] = acc[mt][j][i];
    }
  }
  __syncthreads();
  const int pw_tile = cols / 3, ph = a.h_out / 3, pw = a.w_out / 3;
  for (int e = threadIdx.x; e < MB * pw_tile; e += kBlock) {
    const int ml = e / pw_tile, wc = e - ml * pw_tile;
    const int m = m0 + ml;
    if (m >= a.m_out) continue;
    const float bm = a.bias ? a.bias[m] : 0.0f;
    const float* win = pre + ml * kFwdPos + wc * 3;
    const size_t off = (((size_t)n * a.m_out + m) * ph + rb) * pw + cb * (a.tc / 3) + wc;
    a.y[off] = pool3_relu([&](int k) { return win[(k / 3) * cols + k % 3] + bm; }, a.codes[off]);
  }
}

// wgrad.  Block = (slab, chunk of kWgCC input channels); D[co][col] over every position of the slab's tiles, col = ci * 9
// + tap (local to the chunk) for col < 126, col 126 a column of ones (dbias, written by chunk 0), col 127 zero.  Wave w
// owns the 16-column tiles 2w, 2w + 1 against all 9 output-channel tiles; a k-step is 4 positions (A: dy, 16 channels x 4
// positions; B: 4 positions x 16 columns).  The tile's dy lives in LDS as [144][dps] (zero beyond the tile), x as
// [kWgCC][tr + 2][tc + 2], plus xo[pos] = the position's offset in the x tile.
struct Wg {
  In in;                    // layer input (SRC_PLAIN or SRC_SAT)
  In dy;                    // pre-activation gradient source (SRC_PLAIN with gate, or SRC_POOLED), c_in = 144
  float* slabs;             // [n_slabs][144][c_in * 9 + 1]
  int h_out, w_out, tr, tc, n_rb, n_cb, items, per;
};

template <int SRC, int DSRC>
__global__ __launch_bounds__(kBlock) void conv144_wgrad(Wg q) {
  constexpr int MT = kWgMT, NTW = kWgNTW, CC = kWgCC;
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slab = blockIdx.x, chunk = blockIdx.y, ci0 = chunk * CC;
  const int sw = q.tc + 2, cs = (q.tr + 2) * sw;
  const int dps = (q.tr * q.tc + 3) & ~3;
  float* xl = lds;
  float* dl = xl + CC * cs;
  int* xo = (int*)(dl + kM * dps);

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
    const int cb = it % q.n_cb, rb = (it / q.n_cb) % q.n_rb, n = it / (q.n_cb * q.n_rb);
    const int r0 = rb * q.tr, c0 = cb * q.tc;
    const int rows = min(q.tr, q.h_out - r0), cols = min(q.tc, q.w_out - c0), npos = rows * cols;
    __syncthreads();   // the previous item's reads are done
    stage_in<SRC>(xl, q.in, n, ci0, CC, r0, q.tr + 2, c0, sw);
    for (int i = threadIdx.x; i < kM * dps; i += kBlock) {
      const int co = i / dps, p = i - co * dps;
      float v = 0.0f;
      if (p < npos) {
        const int oh = p / cols, ow = p - oh * cols;
        v = load_in<DSRC>(q.dy, n, co, r0 + oh, c0 + ow);
      }
      dl[i] = v;
    }
    for (int p = threadIdx.x; p < dps; p += kBlock) {
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
      for (int mt = 0; mt < MT; ++mt) av[mt] = dl[(mt * 16 + (lane & 15)) * dps + p];
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        const float b = xl[coff[j] + xoff] * bmul[j] + badd[j];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt][j], 0, 0, 0);
      }
    }
  }
  // this slab's partial sums of the chunk's columns: row co = mt * 16 + (lane / 16) * 4 + i
  const int ncols = q.in.c_in * 9 + 1;
  float* out = q.slabs + (size_t)slab * kM * ncols;
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int col = (wave * NTW + j) * 16 + (lane & 15);
    int gcol = -1;
    if (col < CC * 9 && ci0 + col / 9 < q.in.c_in) gcol = ci0 * 9 + col;
    else if (col == CC * 9 && chunk == 0) gcol = ncols - 1;
    if (gcol < 0) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[(size_t)(mt * 16 + (lane >> 4) * 4 + i) * ncols + gcol] = acc[mt][j][i];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

constexpr int kMaxSatFrames = 27;     // c_in = n_frames + 5 <= 32
constexpr int kMaxWgBlocks = 512;

size_t fwd_lds_bytes(int tr, int tc) {
  const size_t stage = (size_t)9 * kFwdCC * kFwdMT * 16 + (size_t)kFwdCC * (tr + 2) * (tc + 2);
  return std::max(stage, (size_t)kFwdMT * 16 * kFwdPos) * sizeof(float);
}

// forward tile: POOL = one window row (3 output rows) x up to 14 windows; else up to 42 columns x (128 / columns) rows,
// bands of equal size
void fwd_tiles(Fwd& a, bool pool) {
  if (pool) {
    const int pw = a.w_out / 3;
    a.n_cb = (pw + 13) / 14;
    a.tc = 3 * ((pw + a.n_cb - 1) / a.n_cb);
    a.n_cb = (pw * 3 + a.tc - 1) / a.tc;
    a.tr = 3, a.n_rb = a.h_out / 3;
    a.h_out = a.n_rb * 3, a.w_out = pw * 3;   // floor pooling: the last rows / columns are not computed
  } else {
    a.n_cb = (a.w_out + 41) / 42;
    a.tc = (a.w_out + a.n_cb - 1) / a.n_cb;
    a.tr = std::max(1, std::min(a.h_out, kFwdPos / a.tc));
    a.n_rb = (a.h_out + a.tr - 1) / a.tr;
    a.tr = (a.h_out + a.n_rb - 1) / a.n_rb;
  }
  a.n_mg = (a.m_out + kFwdMT * 16 - 1) / (kFwdMT * 16);
}

struct WgPlan {
  int h_out, w_out, tr, tc, n_rb, n_cb, items, n_chunks, n_slabs, per;
  size_t lds, ws;
};

// (h_out, w_out) = the extent that carries a gradient: the conv output, or its whole pool windows
WgPlan wg_plan(int n, int c_in, int h_out, int w_out) {
  WgPlan p;
  p.h_out = h_out, p.w_out = w_out;
  p.n_cb = (w_out + 41) / 42;
  p.tc = (w_out + p.n_cb - 1) / p.n_cb;
  p.tr = std::max(1, std::min(h_out, kWgPos / p.tc));
  p.n_rb = (h_out + p.tr - 1) / p.tr;
  p.tr = (h_out + p.n_rb - 1) / p.n_rb;
  p.items = n * p.n_rb * p.n_cb;
  p.n_chunks = (c_in + kWgCC - 1) / kWgCC;
  // fixed slabs: at most kMaxWgBlocks blocks over (slab, chunk); the workspace is n_slabs partials of 144 x (9 c_in + 1)
  // floats, at most 46 slabs x 747 KB = 34 MB for conv2, 512 x 63 KB = 32 MB for conv1
  const int want = std::max(1, std::min(p.items, kMaxWgBlocks / p.n_chunks));
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  const size_t dps = ((size_t)p.tr * p.tc + 3) & ~(size_t)3;
  p.lds = ((size_t)kWgCC * (p.tr + 2) * (p.tc + 2) + (size_t)kM * dps) * sizeof(float) + dps * sizeof(int);
  p.ws = (size_t)p.n_slabs * kM * (c_in * 9 + 1) * sizeof(float);
  return p;
}

int check_common(const char* who, int n, int c_in, int c_out, int h_in, int w_in, bool pooled) {
  int rc = check_conv_dims(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(c_out == kM, PV_ESIZE, "%s: unsupported channel count c_out=%d (144)", who, c_out);
  if (pooled)
    PV_REQUIRE(h_in >= 5 && w_in >= 5, PV_ESIZE, "%s: spatial extent %d x %d gives no whole 3x3 pool window", who, h_in,
               w_in);
  return PV_OK;
}

int check_plain(const char* who, int n, int c_in, int c_out, int h_in, int w_in, bool pooled) {
  int rc = check_common(who, n, c_in, c_out, h_in, w_in, pooled);
  if (rc) return rc;
  PV_REQUIRE(c_in == kM, PV_ESIZE, "%s: unsupported channel counts c_in=%d c_out=%d (144 -> 144)", who, c_in, c_out);
  return PV_OK;
}

int check_sat(const char* who, int b, int t_total, int n_frames, int h, int w, int c_out) {
  PV_REQUIRE(b > 0 && t_total > 0 && n_frames > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(n_frames <= t_total, PV_EINVAL, "%s: n_frames=%d beyond the %d frames of sat_data", who, n_frames, t_total);
  PV_REQUIRE(n_frames <= kMaxSatFrames, PV_ESIZE, "%s: unsupported channel count: %d frames (at most %d)", who, n_frames,
             kMaxSatFrames);
  int rc = check_common(who, b, n_frames + 5, c_out, h, w, true);
  if (rc) return rc;
  PV_REQUIRE((long long)b * t_total * h * w < (1LL << 31), PV_ESIZE, "%s: sat_data beyond 2^31 elements (32-bit indexing)",
             who);
  return PV_OK;
}

In sat_in(const float* sat, const float* xc, const float* yc, int t_total, int n_frames, int h, int w) {
  In s = {};
  s.x = sat, s.xc = xc, s.yc = yc, s.c_in = n_frames + 5, s.h = h, s.w = w, s.t_total = t_total, s.n_frames = n_frames;
  return s;
}

template <int SRC, bool POOL>
int run_fwd(const char* who, Fwd a, int n, hipStream_t st) {
  fwd_tiles(a, POOL);
  const long long blocks = (long long)n * a.n_rb * a.n_cb * a.n_mg;
  PV_REQUIRE(blocks < (1LL << 31), PV_ESIZE, "%s: grid beyond 2^31 blocks", who);
  conv144_fwd<SRC, POOL><<<dim3((unsigned)blocks), dim3(kBlock), fwd_lds_bytes(a.tr, a.tc), st>>>(a);
  return check_launch(who);
}

template <int SRC, int DSRC>
int run_wgrad(const char* who, const In& in, const In& dy, const WgPlan& p, float* dw, float* db, void* ws,
              size_t ws_bytes, hipStream_t st) {
  int rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  Wg q;
  q.in = in, q.dy = dy, q.slabs = (float*)ws;
  q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per;
  conv144_wgrad<SRC, DSRC><<<dim3((unsigned)p.n_slabs, (unsigned)p.n_chunks), dim3(kBlock), p.lds, st>>>(q);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, db, kM, in.c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d144_sat_pool_fwd_f32(const float* sat, const float* x_coords, const float* y_coords, const float* w,
                                  const float* bias, float* y, uint8_t* codes, int32_t b, int32_t t_total,
                                  int32_t n_frames, int32_t h, int32_t w_img, int32_t c_out, void* stream) {
  const char* who = "pv_conv2d144_sat_pool_fwd_f32";
  PV_REQUIRE(sat && x_coords && y_coords && w && bias && y && codes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_sat(who, b, t_total, n_frames, h, w_img, c_out);
  if (rc) return rc;
  Fwd a = {};
  a.in = sat_in(sat, x_coords, y_coords, t_total, n_frames, h, w_img);
  a.w = w, a.bias = bias, a.y = y, a.codes = codes;
  a.m_out = c_out, a.pad = 0, a.h_out = h - 2, a.w_out = w_img - 2;
  a.w_sm = (n_frames + 5) * 9, a.w_sc = 9, a.flip = 0, a.relu = 1;
  return run_fwd<SRC_SAT, true>(who, a, b, as_stream(stream));
}

int pv_conv2d144_pool_fwd_f32(const float* x, const float* w, const float* bias, float* y, uint8_t* codes, int32_t n,
                              int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d144_pool_fwd_f32";
  PV_REQUIRE(x && w && bias && y && codes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_plain(who, n, c_in, c_out, h_in, w_in, true);
  if (rc) return rc;
  Fwd a = {};
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  a.w = w, a.bias = bias, a.y = y, a.codes = codes;
  a.m_out = c_out, a.pad = 0, a.h_out = h_in - 2, a.w_out = w_in - 2;
  a.w_sm = c_in * 9, a.w_sc = 9, a.flip = 0, a.relu = 1;
  return run_fwd<SRC_PLAIN, true>(who, a, n, as_stream(stream));
}

int pv_conv2d144_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                         int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d144_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_plain(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  Fwd a = {};
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  a.w = w, a.bias = bias, a.y = y;
  a.m_out = c_out, a.pad = 0, a.h_out = h_in - 2, a.w_out = w_in - 2;
  a.w_sm = c_in * 9, a.w_sc = 9, a.flip = 0, a.relu = relu ? 1 : 0;
  return run_fwd<SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d144_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                              int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d144_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_plain(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  // the forward of dy [n][c_out][h_in - 2][w_in - 2] padded by 2, weights mirrored with the channel roles swapped
  Fwd a = {};
  a.in = plain_in(dy, dy_gate, c_out, h_in - 2, w_in - 2);
  a.w = w, a.y = dx, a.out_gate = x_gate;
  a.m_out = c_in, a.pad = 2, a.h_out = h_in, a.w_out = w_in;
  a.w_sm = 9, a.w_sc = c_in * 9, a.flip = 1, a.relu = 0;
  return run_fwd<SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d144_pool_bwd_data_f32(const float* dy_pooled, const uint8_t* codes, const float* w, float* dx,
                                   const float* x_gate, int32_t n, int32_t c_in, int32_t c_out, int32_t h_in,
                                   int32_t w_in, void* stream) {
  const char* who = "pv_conv2d144_pool_bwd_data_f32";
  PV_REQUIRE(dy_pooled && codes && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_plain(who, n, c_in, c_out, h_in, w_in, true);
  if (rc) return rc;
  Fwd a = {};
  a.in = pooled_in(dy_pooled, codes, c_out, h_in - 2, w_in - 2);
  a.w = w, a.y = dx, a.out_gate = x_gate;
  a.m_out = c_in, a.pad = 2, a.h_out = h_in, a.w_out = w_in;
  a.w_sm = 9, a.w_sc = c_in * 9, a.flip = 1, a.relu = 0;
  return run_fwd<SRC_POOLED, false>(who, a, n, as_stream(stream));
}

int pv_conv2d144_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                            int32_t pooled, size_t* bytes) {
  const char* who = "pv_conv2d144_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_common(who, n, c_in, c_out, h_in, w_in, pooled != 0);
  if (rc) return rc;
  PV_REQUIRE(c_in == kM || (c_in > 5 && c_in <= kMaxSatFrames + 5), PV_ESIZE,
             "%s: unsupported channel counts c_in=%d c_out=%d (144 or n_frames + 5 -> 144)", who, c_in, c_out);
  const int ho = pooled ? (h_in - 2) / 3 * 3 : h_in - 2, wo = pooled ? (w_in - 2) / 3 * 3 : w_in - 2;
  *bytes = wg_plan(n, c_in, ho, wo).ws;
  return PV_OK;
}

int pv_conv2d144_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d144_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_plain(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, c_in, h_in - 2, w_in - 2);
  return run_wgrad<SRC_PLAIN, SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                         plain_in(dy, dy_gate, c_out, h_in - 2, w_in - 2), p, dw, dbias, ws, ws_bytes,
                                         as_stream(stream));
}

int pv_conv2d144_pool_bwd_weight_f32(const float* x, const float* dy_pooled, const uint8_t* codes, float* dw,
                                     float* dbias, int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                     void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d144_pool_bwd_weight_f32";
  PV_REQUIRE(x && dy_pooled && codes && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_plain(who, n, c_in, c_out, h_in, w_in, true);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, c_in, (h_in - 2) / 3 * 3, (w_in - 2) / 3 * 3);
  return run_wgrad<SRC_PLAIN, SRC_POOLED>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                          pooled_in(dy_pooled, codes, c_out, h_in - 2, w_in - 2), p, dw, dbias, ws,
                                          ws_bytes, as_stream(stream));
}

int pv_conv2d144_sat_pool_bwd_weight_f32(const float* sat, const float* x_coords, const float* y_coords,
                                         const float* dy_pooled, const uint8_t* codes, float* dw, float* dbias,
                                         int32_t b, int32_t t_total, int32_t n_frames, int32_t h, int32_t w_img,
                                         int32_t c_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d144_sat_pool_bwd_weight_f32";
  PV_REQUIRE(sat && x_coords && y_coords && dy_pooled && codes && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_sat(who, b, t_total, n_frames, h, w_img, c_out);
  if (rc) return rc;
  const WgPlan p = wg_plan(b, n_frames + 5, (h - 2) / 3 * 3, (w_img - 2) / 3 * 3);
  return run_wgrad<SRC_SAT, SRC_POOLED>(who, sat_in(sat, x_coords, y_coords, t_total, n_frames, h, w_img),
                                        pooled_in(dy_pooled, codes, c_out, h - 2, w_img - 2), p, dw, dbias, ws, ws_bytes,
                                        as_stream(stream));
}

}  // extern "C"
