// The two layers of notebooks/05_more_image_inputs.ipynb (the LitAutoEncoder cell, raw lines 1348-1408: STRIDE = 1, GROUPS = 1,
// CHANNELS = 32) that no other notebook has, in exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per
// product, f32 accumulation), as instances of the two implicit GEMMs of conv2d_tile_f32.h with the tiles of
// conv2d_ae_plan_f32.h.  Planes up to 128 wide.  The layers between them are pv_conv2d_ae_*, pv_convt2d_ae_* and
// pv_convt2d_head_*.
//
// First layer, nn.Conv2d(4, 32, 3): x_cat = cat(input_images, T0_IMAGES, optical_flow.squeeze()) is never stored.  SRC_INPUTS4
// reads the flow prediction [n][h][w], the t0 image [n][h][w] and the flow field [n][2][h][w] in place while a tile is staged
// (channels 0, 1 and 2 - 3).  Forward: CINP = 4, MT = 2, one 16 x 16 x 4 K step per tap.  Weight gradient: 4 * 9 + 1 = 37
// columns in three 16-column tiles, one per wave (MT, NTW) = (2, 1), re-reading the three tensors as the forward does.  The
// inputs are data, so there is no data gradient.
//
// Horizon layer, nn.ConvTranspose2d(33, 32, 3): the 33rd input channel is forecast_horizon[n] over the embedding's extent
// (SRC_HORIZON of conv2d_horizon_f32.h: synthesised while staging, 0 in the padding).  Forward: the family's data-gradient
// form at pad 2 over 36 padded channels in one K pass (weights [33][32][3][3] read through their strides, mirrored).  Weight
// gradient: D[co][(ci, tap')] over the positions of dy against the 33-channel input zero-padded by 2, the shared slab sum
// writing dW[ci][co][8 - tap']; row 32 is sum_n horizon[n] sum_pos dy[n][co][pos + tap] and the ones column is the bias
// gradient.  The data gradient of the 32 real channels is pv_convt2d_ae_bwd_data_f32 on the first 32 rows of the weight
// (contiguous), as pv_convt2d_s2_horizon_fwd_f32 arranges it at stride 2.
//
// Weight gradients: fixed slabs, each block writing its partial sums to its own workspace slab, added in slab order (no
// atomics, identical bits run to run).
#include "conv2d_ae_plan_f32.h"
#include "conv2d_horizon_f32.h"

namespace pv {
namespace {

// flow prediction, t0 image, then the two planes of the flow field
template <>
__device__ __forceinline__ float load_in<SRC_INPUTS4>(const In& s, int n, int ch, int r, int col) {
  const size_t pix = (size_t)r * s.w + col, plane = (size_t)s.h * s.w;
  if (ch == 0) return s.x[n * plane + pix];
  if (ch == 1) return s.xc[n * plane + pix];
  return ((const float*)s.flow)[((size_t)n * 2 + (ch - 2)) * plane + pix];
}

constexpr int kMaxWidth = 128;
constexpr int kInputsC = 4, kChannels = 32;   // x_cat's channels; CHANNELS

In inputs4_in(const float* flow_pred, const float* t0, const float* flow_field, int h, int w) {
  In s = {};
  s.x = flow_pred, s.xc = t0, s.flow = flow_field, s.c_in = kInputsC, s.h = h, s.w = w;
  return s;
}

int check_inputs(const char* who, int n, int h, int w) {
  int rc = check_conv_dims(who, n, kInputsC, kChannels, h, w);
  if (rc) return rc;
  PV_REQUIRE(w <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w, kMaxWidth);
  return PV_OK;
}

// (h, w) = the extent of the embedding, the layer's input
int check_horizon(const char* who, int n, int h, int w) {
  PV_REQUIRE(n > 0 && h > 0 && w > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(w + 2 <= kMaxWidth, PV_ESIZE, "%s: output width %d beyond %d", who, w + 2, kMaxWidth);
  PV_REQUIRE((long long)n * (kChannels + 1) * (h + 2) * (w + 2) < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_ae_inputs_fwd_f32(const float* flow_pred, const float* t0, const float* flow_field, const float* w,
                                const float* bias, float* y, int32_t n, int32_t h, int32_t w_img, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_ae_inputs_fwd_f32";
  PV_REQUIRE(flow_pred && t0 && flow_field && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_inputs(who, n, h, w_img);
  if (rc) return rc;
  Fwd a = conv_fwd_args(w, bias, y, kInputsC, kChannels, h, w_img, relu);
  a.in = inputs4_in(flow_pred, t0, flow_field, h, w_img);
  return run_fwd<4, 2, SRC_INPUTS4, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_inputs_bwd_weight_workspace_bytes(int32_t n, int32_t h, int32_t w_img, size_t* bytes) {
  const char* who = "pv_conv2d_ae_inputs_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_inputs(who, n, h, w_img);
  if (rc) return rc;
  *bytes = wg_plan(n, kInputsC, kChannels, h - 2, w_img - 2).ws;
  return PV_OK;
}

int pv_conv2d_ae_inputs_bwd_weight_f32(const float* flow_pred, const float* t0, const float* flow_field, const float* dy,
                                       const float* dy_gate, float* dw, float* dbias, int32_t n, int32_t h, int32_t w_img,
                                       void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_ae_inputs_bwd_weight_f32";
  PV_REQUIRE(flow_pred && t0 && flow_field && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_inputs(who, n, h, w_img);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, kInputsC, kChannels, h - 2, w_img - 2);
  // 37 columns = 3 column tiles, one per wave: the (MT, NTW) = (2, 1) tile, which no layer of run_wgrad's other callers has
  return launch_wgrad<2, 1, SRC_INPUTS4, SRC_PLAIN>(who, inputs4_in(flow_pred, t0, flow_field, h, w_img),
                                                    plain_in(dy, dy_gate, kChannels, h - 2, w_img - 2), 0, p, dw, dbias, false,
                                                    ws, ws_bytes, as_stream(stream));
}

int pv_convt2d_ae_horizon_fwd_f32(const float* x, const float* horizon, const float* w, const float* bias, float* y, int32_t n,
                                  int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_ae_horizon_fwd_f32";
  PV_REQUIRE(x && horizon && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, h_in, w_in);
  if (rc) return rc;
  Fwd a = full_fwd_args(w, bias, y, kChannels, h_in, w_in, relu);
  a.in = horizon_in(x, horizon, kChannels, h_in, w_in);
  return run_fwd<36, 2, SRC_HORIZON, false>(who, a, n, as_stream(stream));
}

int pv_convt2d_ae_horizon_bwd_weight_workspace_bytes(int32_t n, int32_t h_in, int32_t w_in, size_t* bytes) {
  const char* who = "pv_convt2d_ae_horizon_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, h_in, w_in);
  if (rc) return rc;
  *bytes = wg_plan(n, kChannels + 1, kChannels, h_in + 2, w_in + 2).ws;
  return PV_OK;
}

int pv_convt2d_ae_horizon_bwd_weight_f32(const float* x, const float* horizon, const float* dy, const float* dy_gate, float* dw,
                                         float* dbias, int32_t n, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                         void* stream) {
  const char* who = "pv_convt2d_ae_horizon_bwd_weight_f32";
  PV_REQUIRE(x && horizon && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_horizon(who, n, h_in, w_in);
  if (rc) return rc;
  // 33 * 9 + 1 = 298 columns = 19 column tiles, 5 per wave: the (2, 5) tile of the 32 -> 32 layers (the channel counts are
  // fixed, so run_wgrad's dispatch over the other tiles is not instantiated for this source kind)
  const WgPlan p = wg_plan(n, kChannels + 1, kChannels, h_in + 2, w_in + 2);
  return launch_wgrad<2, 5, SRC_HORIZON, SRC_PLAIN>(who, horizon_in(x, horizon, kChannels, h_in, w_in),
                                                    plain_in(dy, dy_gate, kChannels, h_in + 2, w_in + 2), 2, p, dw, dbias, true,
                                                    ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
