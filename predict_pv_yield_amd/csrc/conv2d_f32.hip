// Conv2d 3x3, stride 1, no padding, in exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per product,
// f32 accumulation) for the satellite-image encoder of experiments/002_cnn_processes_single_sat_image_then_rnn.py
// (sat_conv1..3 at :93-101, the 17-channel input built at :140-162 and :180-208).
//
// All three passes are the implicit GEMMs of conv2d_tile_f32.h (conv2d_tile_fwd for forward and dgrad, conv2d_tile_wgrad)
// over a band of output rows of one image: a tile as wide as the output, one column band.  dgrad is the forward of dy
// zero-padded by 2 with mirrored, channel-swapped weights; its epilogue gates dx by the layer input (> 0) so it leaves as
// the lower layer's pre-activation gradient.  This file keeps what is its own: the band planner, the argument checks, and
// the first layer's source, which never materialises its input: its 12 satellite channels are read channels-last from
// sat_data and the 5 synthesised channels are computed while the band is staged (stage_in<SRC_SAT>).  The 32 -> 4 layer's
// weight gradient is the one pass these tiles do not fit; it takes the general Conv3d f32 kernel (conv3d_geom_1x3x3).
#include "conv2d_tile_f32.h"

namespace pv {
namespace {

constexpr int kSatChannels = 12;
constexpr int kCoordChannels = 17;   // 12 satellite + centre marker, geo x, geo y, pixel x, pixel y

// SRC_SAT here: sat[n][h][w][12] channels-last plus the five synthesised channels of experiments/002...py:140-162, 180-208
// (row r = the W axis, column c = the H axis); 0 beyond them.  The satellite channels are read in their native order (12
// consecutive floats per pixel), which is why this source stages itself rather than going through load_in.
template <>
__device__ void stage_in<SRC_SAT>(float* lds, const In& s, int n, int cinp, int r0, int rows, int c0, int cols) {
  const int cs = rows * cols;
  const int tot = cs * kSatChannels;
  for (int i = threadIdx.x; i < tot; i += kBlock) {
    const int ch = i % kSatChannels, pix = i / kSatChannels;
    const int col = pix % cols, r = pix / cols;
    const int ir = r0 + r, ic = c0 + col;
    float v = 0.0f;
    if (ir >= 0 && ir < s.h && ic >= 0 && ic < s.w) v = s.x[(((size_t)n * s.h + ir) * s.w + ic) * kSatChannels + ch];
    lds[ch * cs + r * cols + col] = v;
  }
  const int b = n / s.t_per_ex;
  const float* xc_b = s.xc + (size_t)b * s.w;
  const float* yc_b = s.yc + (size_t)b * s.h;
  const int tot2 = (cinp - kSatChannels) * cs;
  for (int i = threadIdx.x; i < tot2; i += kBlock) {
    const int col = i % cols, r = (i / cols) % rows, ch = kSatChannels + i / cs;
    const int ir = r0 + r, ic = c0 + col;
    float v = 0.0f;
    if (ir >= 0 && ir < s.h && ic >= 0 && ic < s.w)
      v = synth_channel(ch - kSatChannels, ir, ic, s.h / 2, s.w / 2, xc_b, yc_b);
    lds[ch * cs + r * cols + col] = v;
  }
}

In sat_in(const float* sat, const float* xc, const float* yc, int t_per_ex, int h, int w) {
  In s = {};
  s.x = sat, s.xc = xc, s.yc = yc, s.c_in = kCoordChannels, s.h = h, s.w = w, s.t_per_ex = t_per_ex;
  return s;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

constexpr size_t kMaxLds = kLdsFloats * sizeof(float);

// output rows per band: about 192 positions, bands of equal height, the staged input rows within kMaxLds
int band_rows(int h_out, int w_out, int cinp) {
  int rb = std::max(1, std::min(h_out, (192 + w_out - 1) / w_out));
  while (rb > 1 && (size_t)cinp * (rb + 2) * (w_out + 2) * sizeof(float) > kMaxLds) --rb;
  const int nb = (h_out + rb - 1) / rb;
  return (h_out + nb - 1) / nb;
}

// a band is a tile as wide as the output; cinp = the channels whose staged rows bound the band's height
void plan_bands(Fwd& a, int cinp) {
  a.tr = band_rows(a.h_out, a.w_out, cinp), a.tc = a.w_out;
  a.n_rb = (a.h_out + a.tr - 1) / a.tr, a.n_cb = 1;
}

WgPlan wgrad_plan(int n, int c_in, int c_out, int h_in, int w_in) {
  WgPlan p = {};
  p.h_out = h_in - 2, p.w_out = w_in - 2;
  p.cinp = (c_in + 3) & ~3;
  p.mt = 2;   // c_out = 32 (4 output channels take the general kernel: conv3d_geom_1x3x3)
  p.tr = band_rows(p.h_out, p.w_out, p.cinp);
  while (p.tr > 1 && wg_lds_floats(p.cinp, p.mt, p.tr, p.w_out) * sizeof(float) > kMaxLds) --p.tr;
  p.tc = p.w_out, p.n_rb = (p.h_out + p.tr - 1) / p.tr, p.n_cb = 1;
  // workspace: n_slabs <= 512 partials of c_out x (9 c_in + 1) floats, at most 512 x 32 x 289 x 4 B = 18.9 MB
  slab_split(p, n, c_in, c_out);
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
  Fwd a = conv_fwd_args(w, bias, y, kCoordChannels, c_out, h_in, w_in, 1);
  a.in = sat_in(sat, x_coords, y_coords, t_per_example, h_in, w_in);
  plan_bands(a, 20);
  return launch_fwd<20, 2, SRC_SAT, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                      int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  Fwd a = conv_fwd_args(w, bias, y, c_in, c_out, h_in, w_in, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  plan_bands(a, 32);
  // 4 output channels: one 16-row tile (12 rows idle) -- the layer is 6 % of the forward's products
  if (c_out > 16) return launch_fwd<32, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
  return launch_fwd<32, 1, SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                           int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  // the forward of dy [n][c_out][h_in - 2][w_in - 2] padded by 2, weights mirrored with the channel roles swapped
  Fwd a = full_fwd_args(w, nullptr, dx, c_in, h_in - 2, w_in - 2, 0);
  a.in = plain_in(dy, dy_gate, c_out, h_in - 2, w_in - 2);
  a.out_gate = x_gate;
  plan_bands(a, 32);
  if (c_out > 16) return launch_fwd<32, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
  return launch_fwd<4, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                         size_t* bytes) {
  const char* who = "pv_conv2d_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, c_in == kCoordChannels);
  if (rc) return rc;
  if (c_out <= 16) {
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    return pv_conv3d_general_bwd_weight_workspace_bytes(&g, bytes);
  }
  *bytes = wgrad_plan(n, c_in, c_out, h_in, w_in).ws;
  return PV_OK;
}

int pv_conv2d_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                             int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                             void* stream) {
  const char* who = "pv_conv2d_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_dims(who, n, c_in, c_out, h_in, w_in, false);
  if (rc) return rc;
  // The weight gradient of a 32 -> 4 layer (sat_conv3) is 0.95 GFLOP over the same 32-channel input bands as the 32 -> 32
  // layer's: the 16-row output-channel tile would idle 12 of its rows and re-stage a 32-channel band per 4 output channels,
  // so those calls take pv_conv3d_general_bwd_weight_f32 as a 1x3x3 conv with T = 1 (the same NCHW memory, dw [4][32][1][3]
  // [3] = [4][32][3][3]; deterministic: slab partials summed in slab order).
  if (c_out <= 16) {
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    size_t need = 0;
    rc = pv_conv3d_general_bwd_weight_workspace_bytes(&g, &need);
    if (rc) return rc;
    rc = check_workspace(who, ws, ws_bytes, need);
    if (rc) return rc;
    return pv_conv3d_general_bwd_weight_f32(x, dy, dy_gate, dw, dbias, &g, ws, ws_bytes, stream);
  }
  // column tiles: ceil((32 * 9 + 1) / 16) = 19 over 4 waves
  return launch_wgrad<2, 5, SRC_PLAIN, SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                                  plain_in(dy, dy_gate, c_out, h_in - 2, w_in - 2), 0,
                                                  wgrad_plan(n, c_in, c_out, h_in, w_in), dw, dbias, false, ws, ws_bytes,
                                                  as_stream(stream));
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
  // column tiles: ceil((17 * 9 + 1) / 16) = 10 over 4 waves
  return launch_wgrad<2, 3, SRC_SAT, SRC_PLAIN>(who, sat_in(sat, x_coords, y_coords, t_per_example, h_in, w_in),
                                                plain_in(dy, nullptr, c_out, h_in - 2, w_in - 2), 0,
                                                wgrad_plan(n, kCoordChannels, c_out, h_in, w_in), dw, dbias, false, ws,
                                                ws_bytes, as_stream(stream));
}

}  // extern "C"
