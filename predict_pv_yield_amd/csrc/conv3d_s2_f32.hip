// The strided depth-2 Conv3d encoder and the horizon ConvTranspose2d of notebooks/08_multiple_historical_images_as_separate_
// channels.ipynb (the LitAutoEncoder cell: nn.Conv3d 1 -> 8 -> 32 -> 32, kernel (2, 3, 3), stride (1, 2, 2), no padding;
// nn.ConvTranspose2d 33 -> 32, 3x3, stride 2, whose 33rd input channel is the forecast horizon as a constant plane) in exact
// f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation).  Planes up to 128 wide.
//
// The depth-pair view: a depth-2 strided Conv3d on x [n][c][d][h][w] is the stride-2 Conv2d of conv2d_s2_f32.hip over 2 c
// virtual channels, v = 2 c + kd being the plane (c, z + kd) of image (n, z), z < d - 1; the [m][c][2][3][3] weight as it
// lies in memory is that Conv2d's [m][2 c][3][3].  Nothing is copied: SRC_DEPTH reads one depth slice of an NCDHW tensor
// (channel stride d h w, the depth tap an offset of h w) and the outputs are stored with channel stride d_out h_out w_out.
// The three passes are those of conv2d_s2_f32.hip:
//   A  strided gather (forward): K = (kd, tap, c) is run as two passes, one per depth tap, each staging c channels and
//      holding that tap's weights in VGPRs (at 32 -> 32: 144 registers, where both taps at once would be 288); the passes
//      add into the same accumulators, a wave keeping all of its TPW position tiles' accumulators across them.
//   B  parity-class scatter (data gradient, and the horizon ConvTranspose2d's forward with one pass): input depth z receives
//      from output depths z (kd = 0) and z - 1 (kd = 1); at the two depth edges the absent tap's pass is skipped whole.  A
//      wave keeps the accumulators of its (class, tile) slots across the passes.  Every element of dx is written once; where
//      no tap reaches (the last row / column of an even-sized input) the staged zeros give exactly 0.
//   C  strided weight gradient: conv2d_tile_wgrad<.., STRIDE = 2> once per depth tap over the (n, z) images, D[m][(c, tap)]
//      summed by the shared ordered slab sum into the tap's half of dw (strided destination); the ones column of tap 0 is
//      the bias gradient.  Fixed slabs, no atomics.
// The horizon ConvTranspose2d synthesises its 33rd channel while the source tile is staged (SRC_HORIZON: horizon[n] inside
// the source extent, 0 in the halo); in its weight gradient the same source kind is the operand at the output positions, so
// row 32 is sum_n horizon[n] sum_pos dy[n][co][2 pos + tap].
#include "conv2d_horizon_f32.h"
#include "conv2d_s2_plan_f32.h"

namespace pv {
namespace {

// one depth slice of an NCDHW tensor
template <>
__device__ __forceinline__ float load_in<SRC_DEPTH>(const In& s, int img, int ch, int r, int col) {
  const int b = img / s.n_frames, z = img - b * s.n_frames + s.t_per_ex;
  const size_t off = ((((size_t)b * s.c_in + ch) * s.t_total + z) * s.h + r) * s.w + col;
  const float v = s.x[off];
  return (s.gate && !(s.gate[off] > 0.0f)) ? 0.0f : v;
}

constexpr int kMaxWidth = 128;

// A.  Block = (image (b, z), row band, column band) of tr x tc <= 64 TPW output positions; wave w owns the 16-position tiles
// w, w + 4, ... (TPW at most) and keeps their accumulators over both depth-tap passes.  CP = the real input channels rounded
// up to 4.  Per pass the (2 rows + 1) x (2 cols + 1) tile of depth slice z + kd is staged split by column parity.
template <int CP, int MT, int TPW>
__global__ __launch_bounds__(kBlock) void conv3d_s2_gather(Fwd a, int dst_d) {
  extern __shared__ float lds[];
  constexpr int KS = CP / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bid = blockIdx.x;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int img = bid / a.n_rb;
  const int r0 = rb * a.tr, c0 = cb * a.tc;
  const int rows = min(a.tr, a.h_out - r0), cols = min(a.tc, a.w_out - c0);
  const int sw = 2 * cols + 1, sr = 2 * rows + 1, cs = sr * sw, npos = rows * cols, tiles = (npos + 15) / 16;

  acc4 acc[TPW][MT];
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[ti][mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
  for (int kd = 0; kd < 2; ++kd) {
    Fwd b = a;
    b.w = a.w + kd * 9, b.in.t_per_ex = kd;
    int wl = lane;
    asm volatile("" : "+v"(wl));   // this pass's weight offsets are formed here, not kept live from the pass before
    float wa[MT][9][KS];
    load_weights<MT, KS>(wa, b, wl);
    __syncthreads();   // the previous pass's reads are done
    stage_in_split<SRC_DEPTH>(lds, b.in, img, CP, 2 * r0, sr, 2 * c0, sw);
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
      const int t = wave + 4 * ti;
      if (t >= tiles) continue;
      const int p = t * 16 + (lane & 15);
      const int pp = p < npos ? p : 0;
      const int oh = pp / cols, ow = pp - oh * cols;
      const float* src = lds + (lane >> 4) * cs + 2 * oh * sw + ow;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float* st = src + (tap / 3) * sw + (tap % 3 == 1 ? cols + 1 : tap % 3 / 2);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float bv = st[s * 4 * cs];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[ti][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][tap][s], bv, acc[ti][mt], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti) {
    const int t = wave + 4 * ti;
    const int p = t * 16 + (lane & 15);
    if (t >= tiles || p >= npos) continue;
    const int oh = p / cols, ow = p - oh * cols;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt * 16 + (lane >> 4) * 4 + i;
        if (m < a.m_out) store_out_depth(a, img, dst_d, m, r0 + oh, c0 + ow, acc[ti][mt][i]);
      }
  }
}

// B.  scatter_classes3 of conv2d_s2_plan_f32.h, one pass per depth tap.
// Block = (image, row band, column band) of tr x tc <= 128 class-grid positions.  SRC_DEPTH (NKD = 2): the image is (b, z),
// z < dst_d = d_in, the source dy [n][c][d_out][..] read at depth z - kd (in.n_frames = d_in, in.t_total = d_out); a pass
// whose depth is outside [0, d_out) is skipped.  SRC_HORIZON (NKD = 1, dst_d = 1): one pass over the 33 channels.
template <int CP, int MT, int SRC, int NKD>
__global__ __launch_bounds__(kBlock) void conv3d_s2_scatter(Fwd a, int dst_d) {
  extern __shared__ float lds[];
  int bid = blockIdx.x;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int img = bid / a.n_rb;
  const int a0 = rb * a.tr, b0 = cb * a.tc;
  const int sw = a.tc + 1, cs = (a.tr + 1) * sw;
  const int z = img % dst_d;

  acc4 acc[4][kClassTiles][MT];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int ti = 0; ti < kClassTiles; ++ti)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[k][ti][mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};

  float wa[MT][9][CP / 4];
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd) {
    if (NKD == 2 && (z - kd < 0 || z - kd >= a.in.t_total)) continue;   // the same for the whole block
    Fwd b = a;
    b.w = a.w + kd * 9, b.in.t_per_ex = -kd;
    int wl = threadIdx.x & 63;
    asm volatile("" : "+v"(wl));   // this pass's weight offsets are formed here, not kept live from the pass before
    load_weights<MT, CP / 4>(wa, b, wl);
    __syncthreads();   // the previous pass's reads are done
    stage_in<SRC>(lds, b.in, img, CP, a0 - 1, a.tr + 1, b0 - 1, sw);
    __syncthreads();
    scatter_classes3<CP, MT, false>(a, lds, wa, img, dst_d, a0, b0, cs, sw, acc);
  }
  scatter_classes3<CP, MT, true>(a, lds, wa, img, dst_d, a0, b0, cs, sw, acc);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// depth slice z + tap of x [n][c][d][h][w], the pass's image index running over (n, per) with z < per
In depth_in(const float* x, const float* gate, int c, int d, int per, int tap, int h, int w) {
  In s = {};
  s.x = x, s.gate = gate, s.c_in = c, s.t_total = d, s.n_frames = per, s.t_per_ex = tap, s.h = h, s.w = w;
  return s;
}

// A: bands of at most 64 output columns, of equal width; rows: the staged tile within 64 KB and at most 64 TPW positions
template <int CP, int MT, int TPW>
int run_gather3(const char* who, Fwd a, int images, int dst_d, hipStream_t st) {
  a.n_cb = (a.w_out + 63) / 64;
  a.tc = (a.w_out + a.n_cb - 1) / a.n_cb;
  const int fit = (kLdsFloats / (CP * (2 * a.tc + 1)) - 1) / 2;
  a.tr = std::max(1, std::min(std::min(a.h_out, fit), 64 * TPW / a.tc));
  a.n_rb = (a.h_out + a.tr - 1) / a.tr;
  a.tr = (a.h_out + a.n_rb - 1) / a.n_rb;
  const size_t lds = (size_t)CP * (2 * a.tr + 1) * (2 * a.tc + 1) * sizeof(float);
  PV_REQUIRE(lds <= kLdsFloats * sizeof(float) && a.tr * a.tc <= 64 * TPW, PV_ESIZE, "%s: no tile of %d x %d within the LDS budget",
             who, a.tr, a.tc);
  const long long blocks = (long long)images * a.n_rb * a.n_cb;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  conv3d_s2_gather<CP, MT, TPW><<<dim3((unsigned)blocks), dim3(kBlock), lds, st>>>(a, dst_d);
  return check_launch(who);
}

// B: the tiles of scatter_slot_tiles
template <int CP, int MT, int SRC, int NKD>
int run_scatter3(const char* who, Fwd a, int images, int dst_d, hipStream_t st) {
  size_t lds;
  int rc = scatter_slot_tiles(who, a, CP, lds);
  if (rc) return rc;
  const long long blocks = (long long)images * a.n_rb * a.n_cb;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  conv3d_s2_scatter<CP, MT, SRC, NKD><<<dim3((unsigned)blocks), dim3(kBlock), lds, st>>>(a, dst_d);
  return check_launch(who);
}

// the shared ordered slab sum into one depth tap's half of the gradient: dw = the [c_out][c_in][2][3][3] gradient + tap * 9
void launch_slab_sum_depth2(const void* ws, float* dw, float* db, int c_out, int k9, int n_slabs, hipStream_t st) {
  const int total = c_out * (k9 + 1);
  const dim3 grid((unsigned)((total + kSumElems - 1) / kSumElems)), block(kBlock);
  conv2d_slab_sum_f32<false, true><<<grid, block, 0, st>>>((const float*)ws, dw, db, c_out, k9, n_slabs);
}

// C: the 2-D plan over the n (d - 1) images; both depth taps use the same slabs, one after the other
WgPlan wg_plan3(int n, int c_in, int c_out, int d, int h, int w) {
  return wg_plan_s2(n * (d - 1), c_in, c_out, conv_out(h), conv_out(w));
}

template <int MT, int NTW>
int run_wgrad3(const char* who, const float* x, const float* dy, const float* dy_gate, float* dw, float* db, int n, int c_in,
               int c_out, int d, int h, int w, const WgPlan& p, void* ws, hipStream_t st) {
  Wg q;
  q.g = depth_in(dy, dy_gate, c_out, d - 1, d - 1, 0, p.h_out, p.w_out);
  q.slabs = (float*)ws, q.pad = 0;
  q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per, q.cinp = p.cinp;
  for (int kd = 0; kd < 2; ++kd) {
    q.in = depth_in(x, nullptr, c_in, d, d - 1, kd, h, w);
    conv2d_tile_wgrad<MT, NTW, SRC_DEPTH, SRC_DEPTH, 2><<<dim3((unsigned)p.n_slabs), dim3(kBlock), p.lds, st>>>(q);
    int rc = check_launch(who);
    if (rc) return rc;
    launch_slab_sum_depth2(ws, dw + kd * 9, kd == 0 ? db : nullptr, c_out, c_in * 9, p.n_slabs, st);
    rc = check_launch(who);
    if (rc) return rc;
  }
  return PV_OK;
}

// (d, h, w) = the extent of x, the layer's input
int check3(const char* who, int n, int c_in, int c_out, int d, int h, int w, bool data_gradient) {
  PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(d >= 2 && h >= 3 && w >= 3, PV_ESIZE, "%s: extent %d x %d x %d smaller than the (2, 3, 3) kernel", who, d, h, w);
  PV_REQUIRE(w <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w, kMaxWidth);
  PV_REQUIRE((long long)n * std::max(c_in, c_out) * d * h * w < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  PV_REQUIRE((c_in == 1 && c_out == 8 && !data_gradient) || ((c_in == 8 || c_in == 32) && c_out == 32), PV_ESIZE,
             "%s: unsupported channel counts c_in=%d c_out=%d (1 -> 8%s, 8 -> 32 or 32 -> 32)", who, c_in, c_out,
             data_gradient ? " has no data gradient" : "");
  return PV_OK;
}

constexpr int kHorizonReal = 32, kHorizonOut = 32;   // ConvTranspose2d(33, 32): 32 real channels and the horizon

int check_horizon(const char* who, int n, int h, int w) {
  PV_REQUIRE(n > 0 && h > 0 && w > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(2 * w + 1 <= kMaxWidth, PV_ESIZE, "%s: output width %d beyond %d", who, 2 * w + 1, kMaxWidth);
  PV_REQUIRE((long long)n * (kHorizonReal + 1) * (2 * h + 1) * (2 * w + 1) < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv3d_s2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in, int32_t c_out,
                         int32_t d_in, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv3d_s2_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check3(who, n, c_in, c_out, d_in, h_in, w_in, false);
  if (rc) return rc;
  const int d_out = d_in - 1;
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = c_out, a.h_out = conv_out(h_in), a.w_out = conv_out(w_in);
  a.w_sm = c_in * 18, a.w_sc = 18, a.relu = relu ? 1 : 0;
  a.in = depth_in(x, nullptr, c_in, d_in, d_out, 0, h_in, w_in);
  hipStream_t st = as_stream(stream);
  if (c_in == 1) return run_gather3<4, 1, 4>(who, a, n * d_out, d_out, st);
  if (c_in == 8) return run_gather3<8, 2, 4>(who, a, n * d_out, d_out, st);
  return run_gather3<32, 2, 2>(who, a, n * d_out, d_out, st);
}

int pv_conv3d_s2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate, int32_t n,
                              int32_t c_in, int32_t c_out, int32_t d_in, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv3d_s2_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check3(who, n, c_in, c_out, d_in, h_in, w_in, true);
  if (rc) return rc;
  // out dx [c_in] over (h_in, w_in) from dy [c_out]; weights [c_out][c_in][2][3][3] read as [c][m], one depth tap at a time
  Fwd a = {};
  a.w = w, a.y = dx, a.m_out = c_in, a.h_out = h_in, a.w_out = w_in, a.w_sm = 18, a.w_sc = c_in * 18;
  a.out_gate = x_gate;
  a.in = depth_in(dy, dy_gate, c_out, d_in - 1, d_in, 0, conv_out(h_in), conv_out(w_in));
  hipStream_t st = as_stream(stream);
  if (c_in == 8) return run_scatter3<32, 1, SRC_DEPTH, 2>(who, a, n * d_in, d_in, st);
  return run_scatter3<32, 2, SRC_DEPTH, 2>(who, a, n * d_in, d_in, st);
}

int pv_conv3d_s2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t d_in, int32_t h_in, int32_t w_in,
                                            size_t* bytes) {
  const char* who = "pv_conv3d_s2_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check3(who, n, c_in, c_out, d_in, h_in, w_in, false);
  if (rc) return rc;
  *bytes = wg_plan3(n, c_in, c_out, d_in, h_in, w_in).ws;
  return PV_OK;
}

int pv_conv3d_s2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                                int32_t c_in, int32_t c_out, int32_t d_in, int32_t h_in, int32_t w_in, void* ws,
                                size_t ws_bytes, void* stream) {
  const char* who = "pv_conv3d_s2_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check3(who, n, c_in, c_out, d_in, h_in, w_in, false);
  if (rc) return rc;
  const WgPlan p = wg_plan3(n, c_in, c_out, d_in, h_in, w_in);
  rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  PV_REQUIRE(p.lds <= kLdsFloats * sizeof(float), PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, p.lds);
  hipStream_t st = as_stream(stream);
  // column tiles ceil((9 c + 1) / 16) over 4 waves: 1 (c = 1), 5 -> 2 per wave (c = 8), 19 -> 5 per wave (c = 32)
  if (c_in == 1) return run_wgrad3<1, 1>(who, x, dy, dy_gate, dw, dbias, n, c_in, c_out, d_in, h_in, w_in, p, ws, st);
  if (c_in == 8) return run_wgrad3<2, 2>(who, x, dy, dy_gate, dw, dbias, n, c_in, c_out, d_in, h_in, w_in, p, ws, st);
  return run_wgrad3<2, 5>(who, x, dy, dy_gate, dw, dbias, n, c_in, c_out, d_in, h_in, w_in, p, ws, st);
}

int pv_convt2d_s2_horizon_fwd_f32(const float* x, const float* horizon, const float* w, const float* bias, float* y, int32_t n,
                                  int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_s2_horizon_fwd_f32";
  PV_REQUIRE(x && horizon && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, h_in, w_in);
  if (rc) return rc;
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = kHorizonOut, a.h_out = 2 * h_in + 1, a.w_out = 2 * w_in + 1;
  a.w_sm = 9, a.w_sc = kHorizonOut * 9, a.relu = relu ? 1 : 0;
  a.in = horizon_in(x, horizon, kHorizonReal, h_in, w_in);
  return run_scatter3<36, 2, SRC_HORIZON, 1>(who, a, n, 1, as_stream(stream));
}

int pv_convt2d_s2_horizon_bwd_weight_workspace_bytes(int32_t n, int32_t h_in, int32_t w_in, size_t* bytes) {
  const char* who = "pv_convt2d_s2_horizon_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, h_in, w_in);
  if (rc) return rc;
  int nb, per;
  bias_slabs(n, nb, per);
  *bytes = align256(wg_plan_s2(n, kHorizonOut, kHorizonReal + 1, h_in, w_in).ws) + (size_t)nb * kHorizonOut * sizeof(float);
  return PV_OK;
}

int pv_convt2d_s2_horizon_bwd_weight_f32(const float* x, const float* horizon, const float* dy, const float* dy_gate, float* dw,
                                         float* dbias, int32_t n, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                         void* stream) {
  const char* who = "pv_convt2d_s2_horizon_bwd_weight_f32";
  PV_REQUIRE(x && horizon && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, h_in, w_in);
  if (rc) return rc;
  // D[ci][(co, tap)] = sum_pos x33[ci][pos] dy[co][2 pos + tap]: rows = the 33 input channels, the sliding operand is dy
  const WgPlan p = wg_plan_s2(n, kHorizonOut, kHorizonReal + 1, h_in, w_in);
  int nb, per;
  bias_slabs(n, nb, per);
  const size_t bias_off = align256(p.ws);
  rc = check_workspace(who, ws, ws_bytes, bias_off + (size_t)nb * kHorizonOut * sizeof(float));
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int ho = 2 * h_in + 1, wo = 2 * w_in + 1;
  rc = launch_wgrad<3, 5, SRC_PLAIN, SRC_HORIZON, 2>(who, plain_in(dy, dy_gate, kHorizonOut, ho, wo),
                                                     horizon_in(x, horizon, kHorizonReal, h_in, w_in), 0, p, dw, nullptr, false,
                                                     ws, ws_bytes, st);
  if (rc) return rc;
  float* bslabs = (float*)((char*)ws + bias_off);
  plane_sum_slabs_f32<<<dim3((unsigned)nb), dim3(kBlock), 0, st>>>(dy, dy_gate, bslabs, n, per, kHorizonOut, ho * wo);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(bslabs, nullptr, dbias, kHorizonOut, 0, nb, st);
  return check_launch(who);
}

}  // extern "C"
