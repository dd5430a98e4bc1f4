// Conv2d 3x3 on wide channel counts in exact f32 (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation) for
// the frame predictor of notebooks/10_just_conv.ipynb (the nn.Sequential of LitAutoEncoder, raw lines 1386-1392 of the
// .ipynb file: Conv2d 5 -> 64 -> 128 -> 128 (padding 2) -> 1 (stride 2, padding 2); forward with the stripe channel at
// 1395-1410).  Two groups of entry points (the model's last layer, pv_conv2d_head_s2_*, is in conv2d_head_f32.hip):
//   pv_conv2d_wide_*         stride 1, padding 0 or 2, (c_in, c_out) = (64, 128) or (128, 128); the weights (up to 590 KB)
//                            do not fit the VGPRs, so all passes are implicit GEMMs over LDS tiles with K streamed in
//                            channel chunks, as in conv2d_pool_f32.hip:
//     forward / dgrad  D[m][pos]  = sum_{tap, c} A[m][(tap, c)] * X[c][pos + tap]     64 x 256 outputs per block
//     wgrad            D[co][col] = sum_{pos} dy[co][pos] * X[ci][pos + tap]           col = (ci, tap) + a ones column
//                            Padding is staged as zeros and never addressed.  dgrad is the forward of dy padded by 2 - pad
//                            with mirrored, channel-swapped weights (so it also runs 128 -> 64).  wgrad keeps fixed slabs
//                            of tiles in a workspace and adds them in slab order: no atomics, identical bits run to run.
//   pv_conv2d_wide_stripe_*  the first layer, (n_hist + 1) -> 64, padding 0, ReLU: the forecast-horizon stripe channel (1 on
//                            columns [start, start + width), 0 elsewhere) is synthesised while staging, in the forward and
//                            in the weight gradient, and never stored.
// The tiles of both passes, their LDS layouts, the band staging (whole rows per wave, lanes along columns: no per-element
// division) and the tile planners are those of conv_wide_f32.h, shared with conv2d_wide_s2_f32.hip and conv3d_wide_f32.hip;
// this file holds the two kernels' block and item decode, the 2-D source, the extents checks and the entry points.  The slab
// sum, the input descriptor and the workspace check are shared (conv2d_f32_common.h), the stripe source with the stride-2
// file (conv2d_stripe_f32.h).
#include "conv2d_stripe_f32.h"
#include "conv_wide_f32.h"

namespace pv {
namespace {

// the band of stage_rows (conv_wide_f32.h) from image n of a 2-D source
template <int SRC>
__device__ __forceinline__ void stage_rows2(float* lds, const In& s, const Stripe& sp, int n, int c0, int cc, int r0,
                                            int rows, int col0, int cols, int sw, int cs) {
  stage_rows(lds, [&](int ch, int r, int c) { return load_in<SRC>(s, sp, n, ch, r, c); }, true, s.c_in, s.h, s.w, c0, cc, r0,
             rows, col0, cols, sw, cs);
}

struct Fwd {
  In in;
  Stripe sp;
  const float* w;          // element (m, c, tap) at w[m * w_sm + c * w_sc + (flip ? 8 - tap : tap)]
  const float* bias;       // [m_out] or null
  float* y;                // [n][m_out][h_out][w_out]
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int m_out, pad, h_out, w_out, tr, tc, n_rb, n_cb, n_mg, w_sm, w_sc, flip, relu;
};

// Forward / dgrad.  Block = (image, row band, column band, group of 64 output channels); the tile and its steps are those
// of conv_wide_f32.h, once per chunk of 8 input channels.
template <int SRC>
__global__ __launch_bounds__(kBlock) void wide_fwd(Fwd a) {
  extern __shared__ float lds[];
  float* wl = lds;                       // [9][kCC][kMBP]
  float* xl = lds + 9 * kCC * kMBP;      // [kCC][csp]
  int bid = blockIdx.x;
  const int mg = bid % a.n_mg; bid /= a.n_mg;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int n = bid / a.n_rb;
  int xoff[kNTW];
  acc4 acc[kMT][kNTW];
  const FwdBand t = fwd_band(a, rb, cb, mg, xoff, acc);

  for (int k0 = 0; k0 < a.in.c_in; k0 += kCC) {
    __syncthreads();   // the previous chunk's reads are done
    fwd_stage_weights(wl, a, a.in.c_in, t.m0, k0, 0);
    stage_rows2<SRC>(xl, a.in, a.sp, n, k0, kCC, t.r0 - a.pad, t.rows + 2, t.c0 - a.pad, t.sw, t.sw, t.csp);
    __syncthreads();
    fwd_multiply(wl, xl, t, xoff, acc);
  }
  fwd_store(a, t, n, 1, 0, acc);
}

// wgrad.  Block = (slab, chunk of 14 input channels) over the slab's items (image, row band, column band); the tile is that
// of conv_wide_f32.h at position stride 1: the tile's dy lives in LDS as [c_out][98] (zero beyond the tile), x as
// [14][tr + 2][tc + 2].  The ones column (dbias) is written by chunk 0.
struct Wg {
  In in;                    // layer input (SRC_PLAIN or SRC_STRIPE)
  Stripe sp;
  In dy;                    // pre-activation gradient (SRC_PLAIN with its gate), c_in = c_out of the layer
  float* slabs;             // [n_slabs][c_out][c_in * 9 + 1]
  int pad, h_out, w_out, tr, tc, n_rb, n_cb, items, per;
};

template <int SRC, int MT>
__global__ __launch_bounds__(kBlock) void wide_wgrad(Wg q) {
  constexpr int CC = kWgCC, DPS = kWg1Dps, M = MT * 16;
  extern __shared__ float lds[];
  const int slab = blockIdx.x, chunk = blockIdx.y, ci0 = chunk * CC;
  const int sw = q.tc + 2, cs = (q.tr + 2) * sw;
  float* xl = lds;                     // [CC][cs]
  float* dl = xl + CC * cs;            // [M][DPS]
  int* xo = (int*)(dl + M * DPS);      // [DPS]
  const Stripe none = {};

  int coff[kWgNTW];
  float bmul[kWgNTW], badd[kWgNTW];
  wg_columns(ci0, q.in.c_in, cs, sw, coff, bmul, badd);
  acc4 acc[MT][kWgNTW];
  zero_acc(acc);

  const int it0 = slab * q.per, it1 = min(it0 + q.per, q.items);
  for (int it = it0; it < it1; ++it) {
    const int cb = it % q.n_cb, rb = (it / q.n_cb) % q.n_rb, n = it / (q.n_cb * q.n_rb);
    const int r0 = rb * q.tr, c0 = cb * q.tc;
    const int rows = min(q.tr, q.h_out - r0), cols = min(q.tc, q.w_out - c0), npos = rows * cols;
    __syncthreads();   // the previous item's reads are done
    stage_rows2<SRC>(xl, q.in, q.sp, n, ci0, CC, r0 - q.pad, q.tr + 2, c0 - q.pad, sw, sw, cs);
    // dy rows [co][oh] of the tile, packed to cols per row
    stage_rows2<SRC_PLAIN>(dl, q.dy, none, n, 0, M, r0, rows, c0, cols, cols, DPS);
    wg_item_tail<MT, 1, DPS>(dl, xo, npos, cols, sw);
    __syncthreads();
    wg_ksteps<MT, DPS>(xl, dl, xo, npos, coff, bmul, badd, 1.0f, acc);
  }
  const int ncols = q.in.c_in * 9 + 1;
  wg_store<MT>(q.slabs + (size_t)slab * M * ncols, ncols, ci0, q.in.c_in, chunk == 0, nullptr,
               [&](int col) { return ci0 * 9 + col; }, acc);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

struct WgPlan : WgTiles {
  size_t lds, ws;
};

// fixed slabs: at most kWg1MaxBlocks blocks over (slab, chunk); 128 -> 128 at 64 x 126 x 126: 51 slabs x 590 KB = 30 MB
WgPlan wg_plan(int n, int c_in, int c_out, int h_out, int w_out) {
  WgPlan p;
  (WgTiles&)p = wg_tiles(n, c_in, h_out, w_out, kWg1MaxTc, kWg1MaxTr, kWg1Pos, kWg1MaxBlocks, 1);
  p.lds = ((size_t)kWgCC * (p.tr + 2) * (p.tc + 2) + (size_t)c_out * kWg1Dps) * sizeof(float) + kWg1Dps * sizeof(int);
  p.ws = (size_t)p.n_slabs * c_out * (c_in * 9 + 1) * sizeof(float);
  return p;
}

// extents of a padded 3x3 stride-1 conv and 32-bit indexing of every tensor
int check_wide_dims(const char* who, int n, int c_in, int c_out, int h_in, int w_in, int pad) {
  PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(pad == 0 || pad == 2, PV_ESIZE, "%s: unsupported padding %d (0 or 2)", who, pad);
  PV_REQUIRE(h_in + 2 * pad >= 3 && w_in + 2 * pad >= 3, PV_ESIZE,
             "%s: spatial extent %d x %d smaller than the 3x3 kernel", who, h_in, w_in);
  PV_REQUIRE(w_in <= kMaxW, PV_ESIZE, "%s: planes wider than %d columns are not supported (w_in=%d)", who, kMaxW, w_in);
  const long long plane = std::max((long long)h_in * w_in, (long long)(h_in + 2 * pad - 2) * (w_in + 2 * pad - 2));
  PV_REQUIRE((long long)n * std::max(c_in, c_out) * plane < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

int check_wide(const char* who, int n, int c_in, int c_out, int h_in, int w_in, int pad) {
  int rc = check_wide_dims(who, n, c_in, c_out, h_in, w_in, pad);
  if (rc) return rc;
  return check_wide_channels(who, c_in, c_out);
}

int check_stripe(const char* who, int n, int n_hist, int h, int w, int c_out, int stripe_width) {
  int rc = check_stripe_args(who, n_hist, c_out, stripe_width);
  if (rc) return rc;
  return check_wide_dims(who, n, n_hist + 1, c_out, h, w, 0);
}

template <int SRC>
int run_fwd(const char* who, Fwd a, int n, hipStream_t st) {
  const FwdTiles t = fwd_tiles(a.m_out, a.h_out, a.w_out);
  a.tr = t.tr, a.tc = t.tc, a.n_rb = t.n_rb, a.n_cb = t.n_cb, a.n_mg = t.n_mg;
  const long long blocks = (long long)n * a.n_rb * a.n_cb * a.n_mg;
  PV_REQUIRE(blocks < (1LL << 31), PV_ESIZE, "%s: grid beyond 2^31 blocks", who);
  wide_fwd<SRC><<<dim3((unsigned)blocks), dim3(kBlock), wide_fwd_lds_bytes(a.tr, a.tc), st>>>(a);
  return check_launch(who);
}

template <int SRC>
int run_wgrad(const char* who, const In& in, const Stripe& sp, const In& dy, int pad, const WgPlan& p, float* dw,
              float* db, void* ws, size_t ws_bytes, hipStream_t st) {
  int rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  Wg q;
  q.in = in, q.sp = sp, q.dy = dy, q.slabs = (float*)ws, q.pad = pad;
  q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per;
  const dim3 grid((unsigned)p.n_slabs, (unsigned)p.n_chunks), block(kBlock);
  if (dy.c_in == 64) wide_wgrad<SRC, 4><<<grid, block, p.lds, st>>>(q);
  else wide_wgrad<SRC, 8><<<grid, block, p.lds, st>>>(q);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, db, dy.c_in, in.c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_wide_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                           int32_t c_out, int32_t h_in, int32_t w_in, int32_t pad, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_wide_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide(who, n, c_in, c_out, h_in, w_in, pad);
  if (rc) return rc;
  Fwd a = {};
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  a.w = w, a.bias = bias, a.y = y;
  a.m_out = c_out, a.pad = pad, a.h_out = h_in + 2 * pad - 2, a.w_out = w_in + 2 * pad - 2;
  a.w_sm = c_in * 9, a.w_sc = 9, a.flip = 0, a.relu = relu ? 1 : 0;
  return run_fwd<SRC_PLAIN>(who, a, n, as_stream(stream));
}

int pv_conv2d_wide_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, int32_t pad,
                                void* stream) {
  const char* who = "pv_conv2d_wide_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide(who, n, c_in, c_out, h_in, w_in, pad);
  if (rc) return rc;
  // the forward of dy [n][c_out][h_in + 2 pad - 2][w_in + 2 pad - 2] padded by 2 - pad, weights mirrored with the channel
  // roles swapped
  Fwd a = {};
  a.in = plain_in(dy, dy_gate, c_out, h_in + 2 * pad - 2, w_in + 2 * pad - 2);
  a.w = w, a.y = dx, a.out_gate = x_gate;
  a.m_out = c_in, a.pad = 2 - pad, a.h_out = h_in, a.w_out = w_in;
  a.w_sm = 9, a.w_sc = c_in * 9, a.flip = 1, a.relu = 0;
  return run_fwd<SRC_PLAIN>(who, a, n, as_stream(stream));
}

int pv_conv2d_wide_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                              int32_t pad, size_t* bytes) {
  const char* who = "pv_conv2d_wide_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide_dims(who, n, c_in, c_out, h_in, w_in, pad);
  if (rc) return rc;
  const bool wide = (c_in == 64 || c_in == 128) && c_out == 128;
  const bool stripe = c_in >= 2 && c_in <= kMaxHist + 1 && c_out == 64 && pad == 0;
  PV_REQUIRE(wide || stripe, PV_ESIZE,
             "%s: unsupported channel counts c_in=%d c_out=%d ((64 | 128) -> 128, or n_hist + 1 -> 64 without padding)", who,
             c_in, c_out);
  *bytes = wg_plan(n, c_in, c_out, h_in + 2 * pad - 2, w_in + 2 * pad - 2).ws;
  return PV_OK;
}

int pv_conv2d_wide_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                  int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, int32_t pad,
                                  void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_wide_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_wide(who, n, c_in, c_out, h_in, w_in, pad);
  if (rc) return rc;
  const int ho = h_in + 2 * pad - 2, wo = w_in + 2 * pad - 2;
  const WgPlan p = wg_plan(n, c_in, c_out, ho, wo);
  const Stripe none = {};
  return run_wgrad<SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in), none, plain_in(dy, dy_gate, c_out, ho, wo), pad,
                              p, dw, dbias, ws, ws_bytes, as_stream(stream));
}

int pv_conv2d_wide_stripe_fwd_f32(const float* history, const int32_t* stripe_start, const float* w, const float* bias,
                                  float* y, int32_t n, int32_t n_hist, int32_t h, int32_t w_img, int32_t c_out,
                                  int32_t stripe_width, void* stream) {
  const char* who = "pv_conv2d_wide_stripe_fwd_f32";
  PV_REQUIRE(history && stripe_start && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_stripe(who, n, n_hist, h, w_img, c_out, stripe_width);
  if (rc) return rc;
  Fwd a = {};
  a.in = stripe_in(history, n_hist, h, w_img);
  a.sp.start = stripe_start, a.sp.width = stripe_width, a.sp.n_hist = n_hist;
  a.w = w, a.bias = bias, a.y = y;
  a.m_out = c_out, a.pad = 0, a.h_out = h - 2, a.w_out = w_img - 2;
  a.w_sm = (n_hist + 1) * 9, a.w_sc = 9, a.flip = 0, a.relu = 1;
  return run_fwd<SRC_STRIPE>(who, a, n, as_stream(stream));
}

int pv_conv2d_wide_stripe_bwd_weight_f32(const float* history, const int32_t* stripe_start, const float* dy, float* dw,
                                         float* dbias, int32_t n, int32_t n_hist, int32_t h, int32_t w_img, int32_t c_out,
                                         int32_t stripe_width, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_wide_stripe_bwd_weight_f32";
  PV_REQUIRE(history && stripe_start && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_stripe(who, n, n_hist, h, w_img, c_out, stripe_width);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, n_hist + 1, c_out, h - 2, w_img - 2);
  Stripe sp;
  sp.start = stripe_start, sp.width = stripe_width, sp.n_hist = n_hist;
  return run_wgrad<SRC_STRIPE>(who, stripe_in(history, n_hist, h, w_img), sp, plain_in(dy, nullptr, c_out, h - 2, w_img - 2),
                               0, p, dw, dbias, ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
