// Conv3d (2, 3, 3) on wide channel counts in exact f32 (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation)
// for the frame predictor of notebooks/12_just_3d_conv.ipynb (the nn.Sequential of LitAutoEncoder, raw lines 1397-1407 of the
// .ipynb file: Conv3d 2 -> 64 -> 128 -> 128 -> 128 -> 1, kernel (2, 3, 3), spatial padding 1; forward at 1409-1420).  A
// (2, 3, 3) stride-1 Conv3d is the sum of two padded 3x3 Conv2d's over adjacent depth slices, so the passes are the tiles of
// conv_wide_f32.h (shared with conv2d_wide_f32.hip) with the depth tap kd as one more K axis and (image, output slice) where
// that file has the image:
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
// The last layer on depth 2 is a 3x3 stride-2 padding-1 Conv2d on the free views x [n][2 c][h][w] and w [1][2 c][3][3]:
// pv_conv2d_head_s2p1_* in conv2d_head_f32.hip.  This file holds the two kernels' block and item decode, the depth-tap loop,
// the ones / bias1 rule of the bias gradient, the depth-sliced input's own descriptor, the extents checks and the entry
// points.  The slab sum and the workspace check are shared (conv2d_f32_common.h).
#include "conv_wide_f32.h"

namespace pv {
namespace {

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

// the band of stage_rows (conv_wide_f32.h) from slice ds of image n; a slice outside [0, d_in) is padding: all 0
template <int SRC>
__device__ __forceinline__ void stage_rows3(float* lds, const In3& s, int n, int ds, int c0, int cc, int r0, int rows,
                                            int col0, int cols, int sw, int cs) {
  stage_rows(lds, [&](int ch, int r, int c) { return load_in3<SRC>(s, n, ch, ds, r, c); },
             SRC == SRC3_HORIZON || (ds >= 0 && ds < s.d_in), s.c_in, s.h, s.w, c0, cc, r0, rows, col0, cols, sw, cs);
}

struct Fwd3 {
  In3 in;
  const float* w;          // element (m, c, kd, tap) at w[m * w_sm + c * w_sc + (flip ? 1 - kd : kd) * 9 + (flip ? 8 - tap : tap)]
  const float* bias;       // [m_out] or null
  float* y;                // [n][m_out][d_out][h_out][w_out]
  const float* out_gate;   // y zeroed where out_gate <= 0 (same layout as y); may be null
  int m_out, pd, d_out, h_out, w_out, tr, tc, n_rb, n_cb, n_mg, w_sm, w_sc, flip, relu;
};

// Forward / dgrad.  Block = (image, output slice, row band, column band, group of 64 output channels); the tile and its
// steps are those of conv_wide_f32.h, once per depth tap whose source slice exists and per chunk of 8 input channels.
// SRC3_HORIZON: one depth tap (both are folded into the pseudo-channels), one chunk.
template <int SRC>
__global__ __launch_bounds__(kBlock) void wide3_fwd(Fwd3 a) {
  constexpr int NKD = SRC == SRC3_HORIZON ? 1 : 2;
  extern __shared__ float lds[];
  float* wl = lds;                       // [9][kCC][kMBP]
  float* xl = lds + 9 * kCC * kMBP;      // [kCC][csp]
  int bid = blockIdx.x;
  const int mg = bid % a.n_mg; bid /= a.n_mg;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb; bid /= a.n_rb;
  const int dz = bid % a.d_out;
  const int n = bid / a.d_out;
  int xoff[kNTW];
  acc4 acc[kMT][kNTW];
  const FwdBand t = fwd_band(a, rb, cb, mg, xoff, acc);

  for (int kd = 0; kd < NKD; ++kd) {
    const int ds = SRC == SRC3_HORIZON ? dz : dz + kd - a.pd;
    if (SRC == SRC3_PLAIN && (ds < 0 || ds >= a.in.d_in)) continue;   // a padding slice: the same for the whole block
    const int wkd = (a.flip ? 1 - kd : kd) * 9;
    for (int k0 = 0; k0 < a.in.c_in; k0 += kCC) {
      __syncthreads();   // the previous chunk's reads are done
      fwd_stage_weights(wl, a, a.in.c_in, t.m0, k0, wkd);
      stage_rows3<SRC>(xl, a.in, n, ds, k0, kCC, t.r0 - 1, t.rows + 2, t.c0 - 1, t.sw, t.sw, t.csp);
      __syncthreads();
      fwd_multiply(wl, xl, t, xoff, acc);
    }
  }
  fwd_store(a, t, n, a.d_out, dz, acc);
}

// wgrad.  Block = (slab, chunk of 14 input channels, depth tap); D[co][col] over every position of the slab's tiles, col =
// ci * 9 + tap (local to the chunk) for col < 126, col 126 a column of ones (dbias, chunk 0 only), col 127 zero.  An item is
// (image, output slice, row band, column band); an item whose source slice d + kd - pd is padding is skipped.  dbias needs
// every item once, so an item's ones column belongs to depth tap 0, or to depth tap 1 where tap 0's source is padding
// (output slice 0 under depth padding 1; tap 1 then reads slice 0, which exists): no block visits an item for the bias alone
// (that would give those blocks 3 items for the others' 2 under depth padding 1, and a launch lasts as long as its slowest
// block).  Tap 0's sum goes to the slab's bias column, tap 1's to bias1[slab], which bias1_add adds to dbias after the slab
// sum.  The tile is that of conv_wide_f32.h at position stride 1, the ones column weighted by `ones`.  A slab row is
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
  constexpr int CC = kWgCC, DPS = kWg1Dps, M = MT * 16;
  extern __shared__ float lds[];
  const int slab = blockIdx.x, chunk = blockIdx.y, kd = blockIdx.z, ci0 = chunk * CC;
  const int sw = q.tc + 2, cs = (q.tr + 2) * sw;
  float* xl = lds;                     // [CC][cs]
  float* dl = xl + CC * cs;            // [M][DPS]
  int* xo = (int*)(dl + M * DPS);      // [DPS]

  int coff[kWgNTW];
  float bmul[kWgNTW], badd[kWgNTW];
  wg_columns(ci0, q.in.c_in, cs, sw, coff, bmul, badd);
  acc4 acc[MT][kWgNTW];
  zero_acc(acc);

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
    // dy rows [co][oh] of the tile, packed to cols per row
    stage_rows3<SRC3_PLAIN>(dl, q.dy, n, dz, 0, M, r0, rows, c0, cols, cols, DPS);
    wg_item_tail<MT, 1, DPS>(dl, xo, npos, cols, sw);
    __syncthreads();
    wg_ksteps<MT, DPS>(xl, dl, xo, npos, coff, bmul, badd, ones, acc);
  }
  // chunk 0's ones column: depth tap 0's into the slab's bias column, depth tap 1's into the slab's bias1 row
  const int ncols = q.in.c_in * q.nkd * 9 + 1;
  wg_store<MT>(q.slabs + (size_t)slab * M * ncols, ncols, ci0, q.in.c_in, chunk == 0 && kd == 0,
               (chunk == 0 && q.bias1) ? q.bias1 + (size_t)slab * M : nullptr,
               [&](int col) { return ((ci0 + col / 9) * q.nkd + kd) * 9 + col % 9; }, acc);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

struct WgPlan : WgTiles {
  int d_out, nkd;
  size_t lds, ws, ws_slabs;
};

// c_in: the channels the kernel stages (4 pseudo-channels for the horizon layer, with nkd = 1).  Fixed slabs: at most
// kWg1MaxBlocks blocks over (slab, chunk, kd); 128 -> 128: 25 slabs x 1.18 MB = 30 MB
WgPlan wg_plan(int n, int c_in, int nkd, int c_out, int d_out, int h_out, int w_out, int pad_d) {
  WgPlan p;
  (WgTiles&)p = wg_tiles(n * d_out, c_in, h_out, w_out, kWg1MaxTc, kWg1MaxTr, kWg1Pos, kWg1MaxBlocks, nkd);
  p.d_out = d_out, p.nkd = nkd;
  p.lds = ((size_t)kWgCC * (p.tr + 2) * (p.tc + 2) + (size_t)c_out * kWg1Dps) * sizeof(float) + kWg1Dps * sizeof(int);
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
  return check_wide_channels(who, c_in, c_out);
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
  const FwdTiles t = fwd_tiles(a.m_out, a.h_out, a.w_out);
  a.tr = t.tr, a.tc = t.tc, a.n_rb = t.n_rb, a.n_cb = t.n_cb, a.n_mg = t.n_mg;
  const long long blocks = (long long)n * a.d_out * a.n_rb * a.n_cb * a.n_mg;
  PV_REQUIRE(blocks < (1LL << 31), PV_ESIZE, "%s: grid beyond 2^31 blocks", who);
  wide3_fwd<SRC><<<dim3((unsigned)blocks), dim3(kBlock), wide_fwd_lds_bytes(a.tr, a.tc), st>>>(a);
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

}  // extern "C"
