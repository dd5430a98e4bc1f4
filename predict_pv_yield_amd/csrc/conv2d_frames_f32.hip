// The weight-shared per-frame encoder's first layer and the 128 -> 32 ConvTranspose2d of notebooks/07_multiple_historical_
// images.ipynb (the LitAutoEncoder cell: encoder_conv = nn.Conv2d 2 -> 32 -> 32 -> 32, 3x3, stride 2, applied to each of the
// N_HIST_IMAGES = 4 history frames with the forecast horizon as a constant second channel; decoder_conv.0 = nn.ConvTranspose2d
// (128, 32, 3, stride=2) over the four encoder outputs concatenated along the channels) in exact f32 on the matrix cores
// (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation).  Planes up to 128 wide on the wide side.
//
// The frames are folded into the batch: image i = frames b + f.  Layers 2 and 3 of the encoder are then pv_conv2d_s2_* at n =
// frames B, whose weight gradient over all images is the shared one, and [frames B][32][e][f] contiguous is the concatenation
// [B][frames 32][e][f].  What this file adds:
//   first layer   conv2d_tile_fwd / conv2d_tile_wgrad <.., STRIDE = 2> of conv2d_tile_f32.h over SRC_FRAME_HORIZON: channel 0
//                 of image i is plane i of history [B][frames][h][w] read in place, channel 1 is horizon[i / frames] inside
//                 the plane, synthesised while the tile is staged.  In the weight gradient the horizon is an ordinary column
//                 of the D tile.  K is one group of 4 channels of which 2 are real, and 19 of the 32 D columns are used.
//   128 -> 32     along the frame seam: the 128 input channels are four groups of 32, one per frame.
//     forward     B of conv2d_s2_f32.hip (parity-class scatter) in one K pass per frame: each pass stages the frame's 32
//                 channels (SRC_CH_GROUP) and holds its weight slice [32 f, 32 f + 32) in VGPRs (144 registers; all of K at
//                 once would be 576); the passes add into the same accumulators, as conv3d_s2_f32.hip runs one pass per
//                 depth tap, with the same lane-index laundering before each pass's weight load.  (Left rolled, the pass
//                 loop spilled: 256 VGPRs and 368 bytes of scratch; unrolled it is 185 VGPRs + 64 AGPRs and none.)
//     data grad   A (strided gather) at 32 -> 32 over the frames B images of dx [B][128][h][w] = [frames B][32][h][w]: image
//                 (b, f) reads dy[b] (SRC_FRAME_SHARED) and the weight slice f, a block-uniform offset.
//     weight grad C, conv2d_tile_wgrad<2, 5, .., 2>, four independent 32-row problems in one launch (grid.y = the frame): rows
//                 = the frame's 32 channels of x (SRC_CH_GROUP), the sliding operand dy.  A slab holds the four frames' rows
//                 one after the other, [128][32 * 9 + 1], so one ordered slab sum writes dw [128][32][3][3] as it lies.  The
//                 bias gradient is the plane sum of dy in slabs, as for pv_convt2d_s2_*.
// Fixed slabs added in slab order, no atomics: identical bits run to run.
#include "conv2d_s2_plan_f32.h"

namespace pv {
namespace {

constexpr int kMaxWidth = 128;
constexpr int kFrameC = 32;                          // CHANNELS: what the encoder leaves per frame
constexpr int kHistFrames = 4;                       // N_HIST_IMAGES
constexpr int kCatC = kHistFrames * kFrameC;         // decoder_conv.0's input channels

template <>
__device__ __forceinline__ float load_in<SRC_FRAME_HORIZON>(const In& s, int img, int ch, int r, int col) {
  if (ch == 1) return s.horizon[img / s.n_frames];
  return s.x[((size_t)img * s.h + r) * s.w + col];
}

template <>
__device__ __forceinline__ float load_in<SRC_CH_GROUP>(const In& s, int n, int ch, int r, int col) {
  const size_t off = (((size_t)n * s.t_total + s.t_per_ex + ch) * s.h + r) * s.w + col;
  const float v = s.x[off];
  return (s.gate && !(s.gate[off] > 0.0f)) ? 0.0f : v;
}

template <>
__device__ __forceinline__ float load_in<SRC_FRAME_SHARED>(const In& s, int img, int ch, int r, int col) {
  return load_plain(s, img / s.n_frames, ch, r, col);
}

// 128 -> 32 forward.  Block = (image, row band, column band) of tr x tc <= 128 class-grid positions; pass f stages channels
// [CP f, CP f + CP) of the image with one row / column of halo and scatters them through rows [CP f, CP f + CP) of the
// [c_in][m_out][3][3] weight.
template <int CP, int MT, int FRAMES>
__global__ __launch_bounds__(kBlock) void convt2d_s2_frames_scatter(Fwd a) {
  extern __shared__ float lds[];
  int bid = blockIdx.x;
  const int cb = bid % a.n_cb; bid /= a.n_cb;
  const int rb = bid % a.n_rb;
  const int img = bid / a.n_rb;
  const int a0 = rb * a.tr, b0 = cb * a.tc;
  const int sw = a.tc + 1, cs = (a.tr + 1) * sw;

  acc4 acc[4][kClassTiles][MT];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int ti = 0; ti < kClassTiles; ++ti)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[k][ti][mt] = (acc4){0.0f, 0.0f, 0.0f, 0.0f};

  float wa[MT][9][CP / 4];
  Fwd b = a;
#pragma unroll
  for (int f = 0; f < FRAMES; ++f) {
    b.w = a.w + (size_t)f * CP * a.w_sc, b.in.t_per_ex = f * CP;
    int wl = threadIdx.x & 63;
    asm volatile("" : "+v"(wl));   // this pass's weight offsets are formed here, not kept live from the pass before
    load_weights<MT, CP / 4>(wa, b, wl);
    __syncthreads();   // the previous pass's reads are done
    stage_in<SRC_CH_GROUP>(lds, b.in, img, CP, a0 - 1, a.tr + 1, b0 - 1, sw);
    __syncthreads();
    scatter_classes3<CP, MT, false>(a, lds, wa, img, 1, a0, b0, cs, sw, acc);
  }
  scatter_classes3<CP, MT, true>(a, lds, wa, img, 1, a0, b0, cs, sw, acc);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

In frame_horizon_in(const float* history, const float* horizon, int frames, int h, int w) {
  In s = {};
  s.x = history, s.horizon = horizon, s.c_in = 2, s.n_frames = frames, s.h = h, s.w = w;
  return s;
}

// channels [c f, c f + c) of x [n][total][h][w]
In group_in(const float* x, const float* gate, int c, int total, int f, int h, int w) {
  In s = plain_in(x, gate, c, h, w);
  s.t_total = total, s.t_per_ex = f * c;
  return s;
}

In frame_shared_in(const float* x, const float* gate, int c, int frames, int h, int w) {
  In s = plain_in(x, gate, c, h, w);
  s.n_frames = frames;
  return s;
}

// (h, w) = the extent of a history frame
int check_first(const char* who, int n, int frames, int h, int w) {
  PV_REQUIRE(n > 0 && frames > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(h >= 3 && w >= 3, PV_ESIZE, "%s: spatial extent %d x %d smaller than the 3x3 kernel", who, h, w);
  PV_REQUIRE(w <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w, kMaxWidth);
  PV_REQUIRE((long long)n * frames * kFrameC * h * w < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

// (h_in, w_in) = the extent of x, the layer's input
int check_frames(const char* who, int n, int c_in, int c_out, int h_in, int w_in) {
  PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(c_in == kCatC && c_out == kFrameC, PV_ESIZE, "%s: unsupported channel counts c_in=%d c_out=%d (%d -> %d)", who,
             c_in, c_out, kCatC, kFrameC);
  PV_REQUIRE(2 * w_in + 1 <= kMaxWidth, PV_ESIZE, "%s: output width %d beyond %d", who, 2 * w_in + 1, kMaxWidth);
  PV_REQUIRE((long long)n * kCatC * (2 * h_in + 1) * (2 * w_in + 1) < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_s2_frame_horizon_fwd_f32(const float* history, const float* horizon, const float* w, const float* bias, float* y,
                                       int32_t n, int32_t frames, int32_t h, int32_t w_img, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_s2_frame_horizon_fwd_f32";
  PV_REQUIRE(history && horizon && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_first(who, n, frames, h, w_img);
  if (rc) return rc;
  Fwd a = gather_args(w, bias, y, 2, kFrameC, h, w_img, relu);
  a.in = frame_horizon_in(history, horizon, frames, h, w_img);
  return run_gather<4, 2, SRC_FRAME_HORIZON>(who, a, n * frames, as_stream(stream));
}

int pv_conv2d_s2_frame_horizon_bwd_weight_workspace_bytes(int32_t n, int32_t frames, int32_t h, int32_t w_img, size_t* bytes) {
  const char* who = "pv_conv2d_s2_frame_horizon_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_first(who, n, frames, h, w_img);
  if (rc) return rc;
  *bytes = wg_plan_s2(n * frames, 2, kFrameC, conv_out(h), conv_out(w_img)).ws;
  return PV_OK;
}

int pv_conv2d_s2_frame_horizon_bwd_weight_f32(const float* history, const float* horizon, const float* dy, const float* dy_gate,
                                              float* dw, float* dbias, int32_t n, int32_t frames, int32_t h, int32_t w_img,
                                              void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_s2_frame_horizon_bwd_weight_f32";
  PV_REQUIRE(history && horizon && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_first(who, n, frames, h, w_img);
  if (rc) return rc;
  const int ho = conv_out(h), wo = conv_out(w_img);
  const WgPlan p = wg_plan_s2(n * frames, 2, kFrameC, ho, wo);
  // 9 * 2 + 1 = 19 columns: two column tiles, one per wave
  return launch_wgrad<2, 1, SRC_FRAME_HORIZON, SRC_PLAIN, 2>(who, frame_horizon_in(history, horizon, frames, h, w_img),
                                                             plain_in(dy, dy_gate, kFrameC, ho, wo), 0, p, dw, dbias, false, ws,
                                                             ws_bytes, as_stream(stream));
}

int pv_convt2d_s2_frames_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                                 int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_s2_frames_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frames(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  Fwd a = scatter_args(w, bias, y, kFrameC, 2 * h_in + 1, 2 * w_in + 1, relu);
  a.in = group_in(x, nullptr, kFrameC, kCatC, 0, h_in, w_in);
  size_t lds;
  rc = scatter_slot_tiles(who, a, kFrameC, lds);
  if (rc) return rc;
  const long long blocks = (long long)n * a.n_rb * a.n_cb;
  PV_REQUIRE(blocks > 0 && blocks < (1LL << 31), PV_ESIZE, "%s: grid of %lld blocks", who, blocks);
  convt2d_s2_frames_scatter<kFrameC, 2, kHistFrames><<<dim3((unsigned)blocks), dim3(kBlock), lds, as_stream(stream)>>>(a);
  return check_launch(who);
}

int pv_convt2d_s2_frames_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                      int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_convt2d_s2_frames_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frames(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  // per frame a stride-2 valid conv of dy [n][32][2 h + 1][2 w + 1] with the unmirrored weights, rows [32 f, 32 f + 32) of
  // [128][32][3][3] read as [m][c]; dx [n][128][h][w] is [4 n][32][h][w]
  const int ho = 2 * h_in + 1, wo = 2 * w_in + 1;
  Fwd a = gather_args(w, nullptr, dx, kFrameC, kFrameC, ho, wo, 0);
  a.in = frame_shared_in(dy, dy_gate, kFrameC, kHistFrames, ho, wo);
  a.out_gate = x_gate;
  return run_gather<kFrameC, 2, SRC_FRAME_SHARED>(who, a, n * kHistFrames, as_stream(stream));
}

int pv_convt2d_s2_frames_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                    size_t* bytes) {
  const char* who = "pv_convt2d_s2_frames_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frames(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  int nb, per;
  bias_slabs(n, nb, per);
  *bytes = align256(kHistFrames * wg_plan_s2(n, kFrameC, kFrameC, h_in, w_in).ws) + (size_t)nb * kFrameC * sizeof(float);
  return PV_OK;
}

int pv_convt2d_s2_frames_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                        int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                        size_t ws_bytes, void* stream) {
  const char* who = "pv_convt2d_s2_frames_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frames(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  // per frame D[ci][(co, tap)] = sum_pos x[32 f + ci][pos] dy[co][2 pos + tap]: rows = the frame's channels of x, the sliding
  // operand is dy
  const WgPlan p = wg_plan_s2(n, kFrameC, kFrameC, h_in, w_in);
  int nb, per;
  bias_slabs(n, nb, per);
  const size_t bias_off = align256(kHistFrames * p.ws);
  rc = check_workspace(who, ws, ws_bytes, bias_off + (size_t)nb * kFrameC * sizeof(float));
  if (rc) return rc;
  PV_REQUIRE(p.lds <= kLdsFloats * sizeof(float), PV_ESIZE, "%s: tile of %zu bytes beyond the LDS budget", who, p.lds);
  hipStream_t st = as_stream(stream);
  const int ho = 2 * h_in + 1, wo = 2 * w_in + 1;
  Wg q;
  q.in = plain_in(dy, dy_gate, kFrameC, ho, wo), q.g = group_in(x, nullptr, kFrameC, kCatC, 0, h_in, w_in);
  q.slabs = (float*)ws, q.pad = 0;
  q.h_out = p.h_out, q.w_out = p.w_out, q.tr = p.tr, q.tc = p.tc, q.n_rb = p.n_rb, q.n_cb = p.n_cb;
  q.items = p.items, q.per = p.per, q.cinp = p.cinp;
  // grid.y = the frame; a slab is [128][32 * 9 + 1], so one slab sum writes dw [128][32][3][3] as it lies
  conv2d_tile_wgrad<2, 5, SRC_PLAIN, SRC_CH_GROUP, 2><<<dim3((unsigned)p.n_slabs, kHistFrames), dim3(kBlock), p.lds, st>>>(q);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, nullptr, kCatC, kFrameC * 9, p.n_slabs, st);
  rc = check_launch(who);
  if (rc) return rc;
  float* bslabs = (float*)((char*)ws + bias_off);
  plane_sum_slabs_f32<<<dim3((unsigned)nb), dim3(kBlock), 0, st>>>(dy, dy_gate, bslabs, n, per, kFrameC, ho * wo);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(bslabs, nullptr, dbias, kFrameC, 0, nb, st);
  return check_launch(who);
}

}  // extern "C"
