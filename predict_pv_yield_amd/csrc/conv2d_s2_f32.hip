// The stride-2 Conv2d / ConvTranspose2d autoencoder of notebooks/14_back_to_2d_conv_AE.ipynb and 15_int16.ipynb (the
// LitAutoEncoder cell: nn.Sequential of Conv2d 6 -> 16 -> 32 -> 32 -> 32 and ConvTranspose2d 32 -> 32 -> 16 -> 1, all 3x3,
// stride 2, no padding) in exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per product, f32
// accumulation).  Planes are up to 128 wide on the wide side (a Conv2d's input, a ConvTranspose2d's output).
//
// The six passes are three implicit GEMMs over a tile of one image staged in LDS:
//   A  strided gather   D[m][oh][ow] = sum_{tap, c} W[m][c][tap] X[c][2 oh + kh][2 ow + kw]
//      Conv2d forward; ConvTranspose2d data gradient (over dy, weights [c_in][c_out] read as [m][c], unmirrored).
//      conv2d_tile_fwd<.., STRIDE = 2> of conv2d_tile_f32.h: the (2 tr + 1) x (2 tc + 1) tile is staged split by column
//      parity, so each of the three kw taps is a unit-stride ds_read_b32 over the 16 positions of an MFMA tile (the plain
//      layout read at stride 2 puts two lanes on every one of the 64 banks).
//   B  parity-class scatter   Y[m][2 i + kh][2 j + kw] += W[c][m][tap] X[c][i][j]
//      ConvTranspose2d forward; Conv2d data gradient (over dy, weights [c_out][c_in] read as [c][m]).  The output splits by
//      (row parity, column parity) into four stride-1 sub-convolutions over the class grid (a, b) -> (2 a + pr, 2 b + pc)
//      with 4, 2, 2 and 1 taps (even parity: kh = 0, 2 reading rows a, a - 1; odd: kh = 1 reading row a).  A 16-position
//      MFMA tile holds positions of one class, so its k-loop is uniform and only the class's taps are issued: 9 tap
//      products per 2 x 2 output quad.  The source tile is staged plain with one row / column of halo before it; reads are
//      unit stride.  Every output element belongs to exactly one class and is written once: where no tap reaches a source
//      (the last row / column of an even-sized Conv2d input) the staged zeros give exactly 0.
//   C  strided weight gradient   D[m][(c, tap)] = sum_pos G[m][pos] X[c][2 pos + tap]  (+ a ones column)
//      conv2d_tile_wgrad<.., STRIDE = 2>.  Conv2d: G = dy, X = x, the ones column is the bias gradient.  ConvTranspose2d: G
//      = x, X = dy, so D[ci][(co, tap)] is the [c_in][c_out][3][3] layout as it stands; its ones column (sums of x) is not
//      stored, and the bias gradient (sums of dy over all of its positions, which no position grid of x covers evenly) is
//      a per-image plane sum written as slabs of its own.  Fixed slabs, added in slab order by the shared
//      conv2d_slab_sum_f32: no atomics, identical bits run to run.
// First layer: load_in<SRC_COUNTS> of conv2d_counts_f32.h, as in conv2d_ae_f32.hip.
#include "conv2d_counts_f32.h"
#include "conv2d_s2_plan_f32.h"

namespace pv {
namespace {

constexpr int kMaxWidth = 128, kMinCountsSide = 31;   // 31 -> 15 -> 7 -> 3 -> 1: the smallest image four layers accept

// B.  Block = (image, row band, column band) of tr x tc class-grid positions = up to 2 tr x 2 tc outputs.  The source rows
// [a0 - 1, a0 + tr) and columns [b0 - 1, b0 + tc) are staged as lds[ch][tr + 1][tc + 1] (zero outside the source).  The
// 16-position tiles of the four classes are numbered through and dealt to the waves in turn.
template <int CINP, int MT, int PR, int PC>
__device__ __forceinline__ void scatter_class(const Fwd& a, const float* lds, const float (&wa)[MT][9][CINP / 4], int n,
                                              int a0, int b0, int cs, int sw, int& first_tile) {
  constexpr int KS = CINP / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // class positions inside the block: 2 a + PR < h_out, 2 b + PC < w_out
  const int rows = max(0, min(a.tr, (a.h_out - PR + 1) / 2 - a0)), cols = max(0, min(a.tc, (a.w_out - PC + 1) / 2 - b0));
  const int npos = rows * cols, tiles = (npos + 15) / 16;
  const int start = (wave - first_tile) & 3;
  first_tile += tiles;
  for (int t = start; t < tiles; t += 4) {
    const int p = t * 16 + (lane & 15);
    const bool valid = p < npos;
    const int pp = valid ? p : 0;
    const int la = pp / cols, lb = pp - la * cols;
    const float* src = lds + (lane >> 4) * cs + (la + 1) * sw + lb + 1;
    acc4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      if ((kh & 1) != PR) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        if ((kw & 1) != PC) continue;
        const float* st = src - (kh >> 1) * sw - (kw >> 1);   // source (a - kh / 2, b - kw / 2)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float b = st[s * 4 * cs];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][kh * 3 + kw][s], b, acc[mt], 0, 0, 0);
        }
      }
    }
    if (!valid) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt * 16 + (lane >> 4) * 4 + i;
        if (m < a.m_out) store_out(a, n, m, 2 * (a0 + la) + PR, 2 * (b0 + lb) + PC, acc[mt][i]);
      }
  }
}

template <int CINP, int MT>
__global__ __launch_bounds__(kBlock) void conv2d_s2_scatter(Fwd a) {
  extern __shared__ float lds[];
  int bid = blockIdx.x;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int n = bid / a.n_rb;
  const int a0 = rb * a.tr, b0 = cb * a.tc;
  const int sw = a.tc + 1, cs = (a.tr + 1) * sw;

  float wa[MT][9][CINP / 4];
  load_weights<MT, CINP / 4>(wa, a, threadIdx.x & 63);
  stage_in<SRC_PLAIN>(lds, a.in, n, CINP, a0 - 1, a.tr + 1, b0 - 1, sw);
  __syncthreads();

  int first_tile = 0;
  scatter_class<CINP, MT, 0, 0>(a, lds, wa, n, a0, b0, cs, sw, first_tile);
  scatter_class<CINP, MT, 0, 1>(a, lds, wa, n, a0, b0, cs, sw, first_tile);
  scatter_class<CINP, MT, 1, 0>(a, lds, wa, n, a0, b0, cs, sw, first_tile);
  scatter_class<CINP, MT, 1, 1>(a, lds, wa, n, a0, b0, cs, sw, first_tile);
}

// ---- host side (the gather form's tiles and both forms' Fwd are in conv2d_s2_plan_f32.h) -------------------------------

// B: at most 64 output columns = 32 class columns per band; rows: the staged (tr + 1) x (tc + 1) tile within 64 KB, about
// 512 outputs (128 class positions).
template <int CINP, int MT>
int run_scatter(const char* who, Fwd a, int n, hipStream_t st) {
  const int ga = (a.h_out + 1) / 2, gb = (a.w_out + 1) / 2;   // class grid of the even rows / columns (the larger one)
  a.n_cb = (a.w_out + 63) / 64;
  a.tc = (gb + a.n_cb - 1) / a.n_cb;
  a.n_cb = (gb + a.tc - 1) / a.tc;
  const int fit = kLdsFloats / (CINP * (a.tc + 1)) - 1;
  a.tr = std::max(1, std::min(std::min(ga, fit), (128 + a.tc - 1) / a.tc));
  a.n_rb = (ga + a.tr - 1) / a.tr;
  a.tr = (ga + a.n_rb - 1) / a.n_rb;
  const size_t lds = (size_t)CINP * (a.tr + 1) * (a.tc + 1) * sizeof(float);
  PV_REQUIRE(lds <= kLdsFloats * sizeof(float), PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, lds);
  const long long blocks = (long long)n * a.n_rb * a.n_cb;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  conv2d_s2_scatter<CINP, MT><<<dim3((unsigned)blocks), dim3(kBlock), lds, st>>>(a);
  return check_launch(who);
}

template <int XSRC>
int run_wgrad_s2(const char* who, const In& in, const In& g, const WgPlan& p, float* dw, float* db, void* ws, size_t ws_bytes,
                 hipStream_t st) {
  // column tiles ceil((9 c + 1) / 16) over 4 waves: 1 (c = 1, 6), 3 (c = 16), 5 (c = 32)
  const int ntw = ((in.c_in * 9 + 1 + 15) / 16 + 3) / 4;
#define PV_WG(MT, NTW) \
  if (p.mt == MT && ntw == NTW) \
  return launch_wgrad<MT, NTW, XSRC, SRC_PLAIN, 2>(who, in, g, 0, p, dw, db, false, ws, ws_bytes, st)
  PV_WG(2, 5);
  PV_WG(2, 3);
  PV_WG(1, 1);
#undef PV_WG
  return fail(PV_ESIZE, "%s: no weight-gradient tile for %d rows x %d channels", who, g.c_in, in.c_in);
}

enum Kind { KIND_CONV, KIND_COUNTS, KIND_CONVT };

// (h_in, w_in) = the extent of x, the layer's input
int check_s2(const char* who, int n, int c_in, int c_out, int h_in, int w_in, Kind kind) {
  if (kind == KIND_CONVT) {
    PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
    PV_REQUIRE(2 * w_in + 1 <= kMaxWidth, PV_ESIZE, "%s: output width %d beyond %d", who, 2 * w_in + 1, kMaxWidth);
    PV_REQUIRE((long long)n * std::max(c_in, c_out) * (2 * h_in + 1) * (2 * w_in + 1) < (1LL << 31), PV_ESIZE,
               "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
    PV_REQUIRE((c_in == 32 && (c_out == 32 || c_out == 16)) || (c_in == 16 && c_out == 1), PV_ESIZE,
               "%s: unsupported channel counts c_in=%d c_out=%d (32 -> 32, 32 -> 16 or 16 -> 1)", who, c_in, c_out);
    return PV_OK;
  }
  int rc = check_conv_dims(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(w_in <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w_in, kMaxWidth);
  if (kind == KIND_COUNTS) {
    PV_REQUIRE(c_in == 6 && c_out == 16, PV_ESIZE, "%s: unsupported channel count c_out=%d (the counts layer has 16)", who,
               c_out);
    PV_REQUIRE(h_in >= kMinCountsSide && w_in >= kMinCountsSide, PV_ESIZE,
               "%s: spatial extent %d x %d leaves nothing after four 3x3 stride-2 convolutions (%d at least)", who, h_in, w_in,
               kMinCountsSide);
  } else {
    PV_REQUIRE((c_in == 16 || c_in == 32) && c_out == 32, PV_ESIZE,
               "%s: unsupported channel counts c_in=%d c_out=%d (16 -> 32 or 32 -> 32)", who, c_in, c_out);
  }
  return PV_OK;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_s2_counts_fwd_f32(const void* history, int32_t history_is_i16, const void* flow_pred, int32_t flow_is_i16,
                                const float* horizon, const float* w, const float* bias, float* y, int32_t n, int32_t h,
                                int32_t w_img, int32_t c_out, void* stream) {
  const char* who = "pv_conv2d_s2_counts_fwd_f32";
  PV_REQUIRE(history && flow_pred && horizon && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, 6, c_out, h, w_img, KIND_COUNTS);
  if (rc) return rc;
  Fwd a = gather_args(w, bias, y, 6, c_out, h, w_img, 1);
  a.in = counts_in(history, history_is_i16, flow_pred, flow_is_i16, horizon, h, w_img);
  return run_gather<8, 1, SRC_COUNTS>(who, a, n, as_stream(stream));
}

int pv_conv2d_s2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                         int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_s2_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  Fwd a = gather_args(w, bias, y, c_in, c_out, h_in, w_in, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  if (c_in == 16) return run_gather<16, 2, SRC_PLAIN>(who, a, n, as_stream(stream));
  return run_gather<32, 2, SRC_PLAIN>(who, a, n, as_stream(stream));
}

int pv_conv2d_s2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                              int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_s2_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  Fwd a = scatter_args(w, nullptr, dx, c_in, h_in, w_in, 0);
  a.in = plain_in(dy, dy_gate, c_out, conv_out(h_in), conv_out(w_in));
  a.out_gate = x_gate;
  if (c_in == 16) return run_scatter<32, 1>(who, a, n, as_stream(stream));
  return run_scatter<32, 2>(who, a, n, as_stream(stream));
}

int pv_conv2d_s2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                            size_t* bytes) {
  const char* who = "pv_conv2d_s2_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, c_in == 6 ? KIND_COUNTS : KIND_CONV);
  if (rc) return rc;
  *bytes = wg_plan_s2(n, c_in, c_out, conv_out(h_in), conv_out(w_in)).ws;
  return PV_OK;
}

int pv_conv2d_s2_counts_bwd_weight_f32(const void* history, int32_t history_is_i16, const void* flow_pred,
                                       int32_t flow_is_i16, const float* horizon, const float* dy, float* dw, float* dbias,
                                       int32_t n, int32_t h, int32_t w_img, int32_t c_out, void* ws, size_t ws_bytes,
                                       void* stream) {
  const char* who = "pv_conv2d_s2_counts_bwd_weight_f32";
  PV_REQUIRE(history && flow_pred && horizon && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, 6, c_out, h, w_img, KIND_COUNTS);
  if (rc) return rc;
  const int ho = conv_out(h), wo = conv_out(w_img);
  const WgPlan p = wg_plan_s2(n, 6, c_out, ho, wo);
  return run_wgrad_s2<SRC_COUNTS>(who, counts_in(history, history_is_i16, flow_pred, flow_is_i16, horizon, h, w_img),
                                  plain_in(dy, nullptr, c_out, ho, wo), p, dw, dbias, ws, ws_bytes, as_stream(stream));
}

int pv_conv2d_s2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                                int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                void* stream) {
  const char* who = "pv_conv2d_s2_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  const int ho = conv_out(h_in), wo = conv_out(w_in);
  const WgPlan p = wg_plan_s2(n, c_in, c_out, ho, wo);
  return run_wgrad_s2<SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in), plain_in(dy, dy_gate, c_out, ho, wo), p, dw,
                                 dbias, ws, ws_bytes, as_stream(stream));
}

int pv_convt2d_s2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                          int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_s2_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  Fwd a = scatter_args(w, bias, y, c_out, 2 * h_in + 1, 2 * w_in + 1, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  hipStream_t st = as_stream(stream);
  if (c_in == 32 && c_out == 32) return run_scatter<32, 2>(who, a, n, st);
  if (c_in == 32) return run_scatter<32, 1>(who, a, n, st);
  return run_scatter<16, 1>(who, a, n, st);
}

int pv_convt2d_s2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                               int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_convt2d_s2_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  // a stride-2 valid conv of dy [n][c_out][2 h + 1][2 w + 1] with the unmirrored weights, [c_in][c_out][3][3] read as [m][c]
  Fwd a = gather_args(w, nullptr, dx, c_out, c_in, 2 * h_in + 1, 2 * w_in + 1, 0);
  a.in = plain_in(dy, dy_gate, c_out, 2 * h_in + 1, 2 * w_in + 1);
  a.out_gate = x_gate;
  hipStream_t st = as_stream(stream);
  if (c_in == 32 && c_out == 32) return run_gather<32, 2, SRC_PLAIN>(who, a, n, st);
  if (c_in == 32) return run_gather<16, 2, SRC_PLAIN>(who, a, n, st);
  return run_gather<4, 1, SRC_PLAIN>(who, a, n, st);
}

int pv_convt2d_s2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                             size_t* bytes) {
  const char* who = "pv_convt2d_s2_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  int nb, per;
  bias_slabs(n, nb, per);
  *bytes = align256(wg_plan_s2(n, c_out, c_in, h_in, w_in).ws) + (size_t)nb * c_out * sizeof(float);
  return PV_OK;
}

int pv_convt2d_s2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                                 int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                 void* stream) {
  const char* who = "pv_convt2d_s2_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_s2(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  // D[ci][(co, tap)] = sum_pos x[ci][pos] dy[co][2 pos + tap]: rows = c_in, the sliding operand is dy
  const WgPlan p = wg_plan_s2(n, c_out, c_in, h_in, w_in);
  int nb, per;
  bias_slabs(n, nb, per);
  const size_t bias_off = align256(p.ws);
  rc = check_workspace(who, ws, ws_bytes, bias_off + (size_t)nb * c_out * sizeof(float));
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int ho = 2 * h_in + 1, wo = 2 * w_in + 1;
  rc = run_wgrad_s2<SRC_PLAIN>(who, plain_in(dy, dy_gate, c_out, ho, wo), plain_in(x, nullptr, c_in, h_in, w_in), p, dw,
                               nullptr, ws, ws_bytes, st);
  if (rc) return rc;
  float* bslabs = (float*)((char*)ws + bias_off);
  plane_sum_slabs_f32<<<dim3((unsigned)nb), dim3(kBlock), 0, st>>>(dy, dy_gate, bslabs, n, per, c_out, ho * wo);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(bslabs, nullptr, dbias, c_out, 0, nb, st);
  return check_launch(who);
}

}  // extern "C"
