// The 2-D encoder / decoder of notebooks/16_maxpool.ipynb (the LitAutoEncoder cell, raw lines 13737-13830) in exact f32 on
// the matrix cores (v_mfma_f32_16x16x4_f32: one rounding per product, f32 accumulation): Conv2d 3x3 valid 6 -> 16 -> 32 ->
// 32 -> 32 with MaxPool2d(3) fused into the fourth layer, ConvTranspose2d 3x3 (stride 1, no padding) 32 -> 32 -> 16 -> 16 ->
// 1, and the cropped, normalised MSE.  Planes are up to 128 wide.
//
// Every convolution pass is one of the two implicit GEMMs of conv2d_tile_f32.h over a tile of tr x tc output positions of
// one image staged in LDS:
//   forward-like  D[m][pos]  = sum_{tap, c} A[m][(tap, c)] * X[c][pos + tap]     A = weights, held in VGPRs
//   wgrad-like    D[m][col]  = sum_{pos} G[m][pos] * X[c][pos + tap]             col = (c, tap), plus a ones column
// Conv2d forward is the first with pad 0; its data gradient is the first over dy zero-padded by 2 with mirrored,
// channel-swapped weights.  ConvTranspose2d forward IS that data-gradient form (weights [c_in][c_out][3][3] read through
// their strides, mirrored), its data gradient is the plain valid form with unmirrored weights, and its weight gradient is
// the second form over the positions of dy against x zero-padded by 2: D[co][(ci, tap')] with dW[ci][co][8 - tap'] =
// D[co][(ci, tap')], so the ones column is the bias gradient as for Conv2d; the shared slab sum writes the transposed layout.
// The 16 -> 1 layer shares these kernels (one 16-row tile with 15 rows idle: 0.08 % of the step's products).  Large
// launches of the passes that lost to pv_conv3d_general_*_f32 when timed run there (general_route below): the plain Conv2d
// data and weight gradients, the 32 -> 32 forward, and the pooled layer's forward (+ a pool kernel) and weight gradient (+
// an expansion kernel).
//
// Tiles.  A 128-wide band of 32 channels is 16.6 KB per row, so a tile is at most 64 columns wide and as many rows as keep
// the staged halo tile within 64 KB (two blocks per CU): 5 rows x 64 columns at 32 channels, 8 x 64 at 16.  The weight
// gradient also stages the tile's G rows, so its tiles are chosen by the smallest halo overhead that fits.
// First layer: history [B][4][S][S] and the flow prediction [B][S][S] are read in place as int16 or f32 counts, normalised
// ((v - 93.23458) / 115.34247: subtract, then a true f32 divide) while staged; the horizon plane is synthesised
// (load_in<SRC_COUNTS> of conv2d_counts_f32.h, shared with conv2d_s2_f32.hip).  Pooling follows conv2d_pool_f32.hip
// through the shared pool3_relu / pool3_expand: the forward
// pools the pre-activations of a tile of whole windows, applies ReLU to the maxima, and writes one code byte per pooled
// output (0..8 = first maximum, row-major; 255 = maximum <= 0, no gradient); backward passes expand the pooled gradient
// through the codes while staging.  Weight gradients: fixed slabs, each block writing its partial sums to its own
// workspace slab, added in slab order (no atomics, identical bits run to run).
//
// notebooks/11_just_conv_and_conv_over_time.ipynb (the LitAutoEncoder cell, raw lines 1407-1416 and 1428-1447) adds two
// layers to this file.  Its first layer, Conv2d 2 -> 16 on each history frame with the forecast-horizon stripe as the second
// channel, is the counts layer's tile pair over SRC_STRIPE: image frames b + f reads plane f of history [b] in place and the
// stripe plane of example b is synthesised while the tile is staged (Stripe / load_in of conv2d_stripe_f32.h), so neither the
// [frames n][2][h][w] input nor the plane is stored.  Its padded layer, Conv2d 32 -> 32 padding 2, is the ConvTranspose2d 32
// -> 32 passes of this file with the weight index switched (Fwd's w_sm / w_sc / flip; the slab sum untransposed): forward =
// the padded form with [c_out][c_in] read as it lies, data gradient = the valid form with the mirrored, channel-swapped
// weight, weight gradient = D[co][(ci, tap)] over the positions of dy against x zero-padded by 2.  No weight copy is made.
#include "conv2d_ae_plan_f32.h"
#include "conv2d_counts_f32.h"
#include "conv2d_stripe_f32.h"

namespace pv {
namespace {

constexpr int kMaxWidth = 128, kCrop = 8, kMinSide = 11;
constexpr int kFrameStripeC = 16, kPaddedC = 32;   // notebook 11: CHANNELS // 2 of its first layer, CHANNELS of its padded one

// SRC_STRIPE under the tile kernels (c_in = 2): x = history [n][n_frames][h][w], flow = the int32 stripe starts [n], t_total =
// the stripe's width.  Image i = n_frames b + f: channel 0 is plane i of history (a one-frame history indexed by the image),
// channel 1 the stripe plane of example b.
template <>
__device__ __forceinline__ float load_in<SRC_STRIPE>(const In& s, int img, int ch, int r, int col) {
  const Stripe sp = {(const int32_t*)s.flow, s.t_total, 1};
  return load_in<SRC_STRIPE>(s, sp, ch == 0 ? img : img / s.n_frames, ch, r, col);
}

// Windowed, normalised MSE (16_maxpool.ipynb, _training_or_validation_step: the window starts at (8, 8); 15_int16.ipynb: at
// (0, 0)): block b takes example b; d = y_hat - (target[row0 + r][col0 + c] - mean) / std, dy_hat = 2 d / count, partial[b]
// = sum d^2 (tree sum in LDS: fixed order); then one block adds the partials in index order.
__global__ __launch_bounds__(kBlock) void mse_window_norm_partial(const float* __restrict__ y_hat, const void* target,
                                                                 int t_i16, int oh, int ow, int th, int tw, int row0,
                                                                 int col0, float inv_count, float* __restrict__ dy_hat,
                                                                 float* __restrict__ partials) {
  __shared__ float part[kBlock];
  const int b = blockIdx.x, tot = oh * ow;
  float s = 0.0f;
  for (int i = threadIdx.x; i < tot; i += kBlock) {
    const int r = i / ow, c = i - r * ow;
    const float t = count_at(target, t_i16, ((size_t)b * th + row0 + r) * tw + col0 + c);
    const float d = y_hat[(size_t)b * tot + i] - t;
    if (dy_hat) dy_hat[(size_t)b * tot + i] = 2.0f * d * inv_count;
    s += d * d;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[b] = part[0];
}

__global__ __launch_bounds__(kBlock) void mse_window_norm_final(const float* __restrict__ partials, int n, float inv_count,
                                                             float* __restrict__ loss) {
  __shared__ float part[kBlock];
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += kBlock) s += partials[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] * inv_count;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

enum Kind { KIND_CONV, KIND_POOL, KIND_CONVT };

int check_ae(const char* who, int n, int c_in, int c_out, int h_in, int w_in, Kind kind) {
  if (kind == KIND_CONVT) {
    // any input extent >= 1 x 1 (the 11-pixel image leaves one pooled value per channel)
    PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
    PV_REQUIRE(w_in + 2 <= kMaxWidth, PV_ESIZE, "%s: output width %d beyond %d", who, w_in + 2, kMaxWidth);
    PV_REQUIRE((long long)n * std::max(c_in, c_out) * (h_in + 2) * (w_in + 2) < (1LL << 31), PV_ESIZE,
               "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
    PV_REQUIRE((c_in == 32 && (c_out == 32 || c_out == 16)) || (c_in == 16 && (c_out == 16 || c_out == 1)), PV_ESIZE,
               "%s: unsupported channel counts c_in=%d c_out=%d (32 -> 32, 32 -> 16, 16 -> 16 or 16 -> 1)", who, c_in, c_out);
    return PV_OK;
  }
  int rc = check_conv_dims(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(w_in <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w_in, kMaxWidth);
  if (kind == KIND_POOL) {
    PV_REQUIRE(c_in == 32 && c_out == 32, PV_ESIZE, "%s: unsupported channel counts c_in=%d c_out=%d (32 -> 32)", who, c_in,
               c_out);
    PV_REQUIRE(h_in >= 5 && w_in >= 5, PV_ESIZE, "%s: spatial extent %d x %d gives no whole 3x3 pool window", who, h_in,
               w_in);
  } else {
    PV_REQUIRE((c_in == 16 || c_in == 32) && c_out == 32, PV_ESIZE,
               "%s: unsupported channel counts c_in=%d c_out=%d (16 -> 32 or 32 -> 32)", who, c_in, c_out);
  }
  return PV_OK;
}

int check_counts(const char* who, int n, int h, int w, int c_out) {
  int rc = check_conv_dims(who, n, 6, c_out, h, w);
  if (rc) return rc;
  PV_REQUIRE(c_out == 16, PV_ESIZE, "%s: unsupported channel count c_out=%d (the counts layer has 16)", who, c_out);
  PV_REQUIRE(w <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w, kMaxWidth);
  PV_REQUIRE(h >= kMinSide && w >= kMinSide, PV_ESIZE,
             "%s: spatial extent %d x %d gives no whole 3x3 pool window after four 3x3 convolutions", who, h, w);
  return PV_OK;
}

In frame_stripe_in(const float* history, const int32_t* stripe_start, int frames, int stripe_width, int h, int w) {
  In s = {};
  s.x = history, s.flow = stripe_start, s.t_total = stripe_width, s.n_frames = frames, s.c_in = 2, s.h = h, s.w = w;
  return s;
}

// (h, w) = the extent of a history frame
int check_frame_stripe(const char* who, int n, int frames, int h, int w, int c_out, int stripe_width) {
  PV_REQUIRE(n > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(frames >= 1 && frames <= kMaxHist, PV_ESIZE, "%s: unsupported frame count %d (1..%d)", who, frames, kMaxHist);
  PV_REQUIRE(c_out == kFrameStripeC, PV_ESIZE, "%s: unsupported channel count c_out=%d (%d)", who, c_out, kFrameStripeC);
  PV_REQUIRE(stripe_width >= 0, PV_EINVAL, "%s: negative stripe width", who);
  PV_REQUIRE(h >= 3 && w >= 3, PV_ESIZE, "%s: spatial extent %d x %d smaller than the 3x3 kernel", who, h, w);
  PV_REQUIRE(w <= kMaxWidth, PV_ESIZE, "%s: width %d beyond %d", who, w, kMaxWidth);
  PV_REQUIRE((long long)n * frames * kFrameStripeC * h * w < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

// (h_in, w_in) = the extent of x, the padded layer's input; the output is (h_in + 2) x (w_in + 2)
int check_p2(const char* who, int n, int c_in, int c_out, int h_in, int w_in) {
  PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(c_in == kPaddedC && c_out == kPaddedC, PV_ESIZE, "%s: unsupported channel counts c_in=%d c_out=%d (32 -> 32)",
             who, c_in, c_out);
  PV_REQUIRE(w_in + 2 <= kMaxWidth, PV_ESIZE, "%s: output width %d beyond %d", who, w_in + 2, kMaxWidth);
  PV_REQUIRE((long long)n * kPaddedC * (h_in + 2) * (w_in + 2) < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

// Routing by size.  Timed at B = 64, S = 128 (tools/time_nb16.py; profiles/nb16/NOTES.md keeps the rows of the two runs
// made before each routing), this file's kernels lost to pv_conv3d_general_*_f32 on the same tensors as 1x3x3 convs with T
// = 1 in: the data gradients of the 16 -> 32 / 32 -> 32 layers (0.39 / 0.57 against 0.26 / 0.45 ms), their weight gradients
// (0.44 / 0.60 against 0.24 / 0.26 ms), the 32 -> 32 forward (0.516 against 0.503 ms), the pooled layer's forward (0.60
// against 0.36 ms without the pool) and its weight gradient (0.53 against 0.24 ms on a materialised pre-pool gradient).  Those
// launches take the general kernel from kGeneralPositions output positions up; the pooled layer adds pool3_relu_codes_f32
// after the forward and pool3_expand_f32 before the weight gradient (0.37 and 0.31 ms with them:
// profiles/nb16/time_nb16_B64.json).  The threshold itself is a provisional choice, not a measured crossover: only that one
// size has been timed, and 32768 output positions puts it (1.0 M positions per launch) far above, the reduced test shapes
// below.  Same NCHW memory, same gates, slab partials summed in slab order.
constexpr long long kGeneralPositions = 32768;

bool general_route(int n, int h_in, int w_in) { return (long long)n * (h_in - 2) * (w_in - 2) >= kGeneralPositions; }

// The pooled layer on the general route: pv_conv3d_general_fwd_f32 writes the pre-activations z (bias included) to the
// workspace, then one thread per pooled output puts its whole window through pool3_relu -- what conv2d_tile_fwd<.., POOL>
// does in its epilogue.
__global__ __launch_bounds__(kBlock) void pool3_relu_codes_f32(const float* __restrict__ z, float* __restrict__ y,
                                                              uint8_t* __restrict__ codes, int planes, int h, int w, int ph,
                                                              int pw) {
  const long long total = (long long)planes * ph * pw;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
    const int pc = (int)(e % pw), pr = (int)((e / pw) % ph);
    const long long plane = e / ((long long)pw * ph);
    const float* win = z + (plane * h + pr * 3) * w + pc * 3;
    y[e] = pool3_relu([&](int k) { return win[(k / 3) * w + k % 3]; }, codes[e]);
  }
}

// ... and its weight gradient: the pre-pool gradient [planes][h][w] written out once (the pooled gradient at the window
// position its code names, 0 elsewhere and beyond the whole windows), then pv_conv3d_general_bwd_weight_f32 on it.
__global__ __launch_bounds__(kBlock) void pool3_expand_f32(const float* __restrict__ dyp, const uint8_t* __restrict__ codes,
                                                          float* __restrict__ dz, int planes, int h, int w, int ph, int pw) {
  const long long total = (long long)planes * h * w;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
    const int c = (int)(e % w), r = (int)((e / w) % h);
    const long long plane = e / ((long long)w * h);
    dz[e] = pool3_expand(dyp + plane * ph * pw, codes + plane * ph * pw, ph, pw, r, c);
  }
}

// bytes of a [n][c][h_in - 2][w_in - 2] f32 scratch tensor, rounded up so that what follows it stays 256-byte aligned
size_t pre_pool_bytes(int n, int c, int h_in, int w_in) {
  return (((size_t)n * c * (h_in - 2) * (w_in - 2) * sizeof(float)) + 255) & ~(size_t)255;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_ae_counts_fwd_f32(const void* history, int32_t history_is_i16, const void* flow_pred, int32_t flow_is_i16,
                                const float* horizon, const float* w, const float* bias, float* y, int32_t n, int32_t h,
                                int32_t w_img, int32_t c_out, void* stream) {
  const char* who = "pv_conv2d_ae_counts_fwd_f32";
  PV_REQUIRE(history && flow_pred && horizon && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_counts(who, n, h, w_img, c_out);
  if (rc) return rc;
  Fwd a = conv_fwd_args(w, bias, y, 6, c_out, h, w_img, 1);
  a.in = counts_in(history, history_is_i16, flow_pred, flow_is_i16, horizon, h, w_img);
  return run_fwd<8, 1, SRC_COUNTS, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                         int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_ae_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  if (c_in == 32 && general_route(n, h_in, w_in)) {   // 32 -> 32 only: the 16 -> 32 forward is faster here (0.23 / 0.24 ms)
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    return pv_conv3d_general_fwd_f32(x, w, bias, y, &g, relu ? 1 : 0, stream);
  }
  Fwd a = conv_fwd_args(w, bias, y, c_in, c_out, h_in, w_in, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  if (c_in == 16) return run_fwd<16, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
  return run_fwd<32, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_pool_fwd_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                          size_t* bytes) {
  const char* who = "pv_conv2d_ae_pool_fwd_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_POOL);
  if (rc) return rc;
  *bytes = general_route(n, h_in, w_in) ? pre_pool_bytes(n, c_out, h_in, w_in) : 0;
  return PV_OK;
}

int pv_conv2d_ae_pool_fwd_f32(const float* x, const float* w, const float* bias, float* y, uint8_t* codes, int32_t n,
                              int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                              void* stream) {
  const char* who = "pv_conv2d_ae_pool_fwd_f32";
  PV_REQUIRE(x && w && bias && y && codes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_POOL);
  if (rc) return rc;
  if (general_route(n, h_in, w_in)) {
    rc = check_workspace(who, ws, ws_bytes, pre_pool_bytes(n, c_out, h_in, w_in));
    if (rc) return rc;
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    rc = pv_conv3d_general_fwd_f32(x, w, bias, (float*)ws, &g, 0, stream);
    if (rc) return rc;
    const int ph = (h_in - 2) / 3, pw = (w_in - 2) / 3;
    pool3_relu_codes_f32<<<dim3(stream_grid((size_t)n * c_out * ph * pw, kBlock)), dim3(kBlock), 0, as_stream(stream)>>>(
        (const float*)ws, y, codes, n * c_out, h_in - 2, w_in - 2, ph, pw);
    return check_launch(who);
  }
  Fwd a = conv_fwd_args(w, bias, y, c_in, c_out, h_in, w_in, 1);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  a.codes = codes;
  return run_fwd<32, 2, SRC_PLAIN, true>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                              int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_ae_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  if (general_route(n, h_in, w_in)) {
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    return pv_conv3d_general_bwd_data_f32(dy, dy_gate, w, dx, x_gate, &g, stream);
  }
  Fwd a = full_fwd_args(w, nullptr, dx, c_in, h_in - 2, w_in - 2, 0);
  a.in = plain_in(dy, dy_gate, c_out, h_in - 2, w_in - 2);
  a.out_gate = x_gate;
  if (c_in == 16) return run_fwd<32, 1, SRC_PLAIN, false>(who, a, n, as_stream(stream));
  return run_fwd<32, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_pool_bwd_data_f32(const float* dy_pooled, const uint8_t* codes, const float* w, float* dx,
                                   const float* x_gate, int32_t n, int32_t c_in, int32_t c_out, int32_t h_in,
                                   int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_ae_pool_bwd_data_f32";
  PV_REQUIRE(dy_pooled && codes && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_POOL);
  if (rc) return rc;
  Fwd a = full_fwd_args(w, nullptr, dx, c_in, h_in - 2, w_in - 2, 0);
  a.in = pooled_in(dy_pooled, codes, c_out, h_in - 2, w_in - 2);
  a.out_gate = x_gate;
  return run_fwd<32, 2, SRC_POOLED, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                            int32_t pooled, size_t* bytes) {
  const char* who = "pv_conv2d_ae_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = c_in == 6 ? check_counts(who, n, h_in, w_in, c_out)
                     : check_ae(who, n, c_in, c_out, h_in, w_in, pooled ? KIND_POOL : KIND_CONV);
  if (rc) return rc;
  if (c_in != 6 && general_route(n, h_in, w_in)) {
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    rc = pv_conv3d_general_bwd_weight_workspace_bytes(&g, bytes);
    if (rc == PV_OK && pooled) *bytes += pre_pool_bytes(n, c_out, h_in, w_in);   // the expanded gradient comes first
    return rc;
  }
  const int ho = pooled ? (h_in - 2) / 3 * 3 : h_in - 2, wo = pooled ? (w_in - 2) / 3 * 3 : w_in - 2;
  *bytes = wg_plan(n, c_in, c_out, ho, wo).ws;
  return PV_OK;
}

int pv_conv2d_ae_counts_bwd_weight_f32(const void* history, int32_t history_is_i16, const void* flow_pred,
                                       int32_t flow_is_i16, const float* horizon, const float* dy, float* dw, float* dbias,
                                       int32_t n, int32_t h, int32_t w_img, int32_t c_out, void* ws, size_t ws_bytes,
                                       void* stream) {
  const char* who = "pv_conv2d_ae_counts_bwd_weight_f32";
  PV_REQUIRE(history && flow_pred && horizon && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_counts(who, n, h, w_img, c_out);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, 6, c_out, h - 2, w_img - 2);
  return run_wgrad<SRC_COUNTS, SRC_PLAIN>(who, counts_in(history, history_is_i16, flow_pred, flow_is_i16, horizon, h, w_img),
                                          plain_in(dy, nullptr, c_out, h - 2, w_img - 2), 0, p, dw, dbias, false, ws,
                                          ws_bytes, as_stream(stream));
}

int pv_conv2d_ae_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                                int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                void* stream) {
  const char* who = "pv_conv2d_ae_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONV);
  if (rc) return rc;
  if (general_route(n, h_in, w_in)) {
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    size_t need = 0;
    rc = pv_conv3d_general_bwd_weight_workspace_bytes(&g, &need);
    if (rc) return rc;
    rc = check_workspace(who, ws, ws_bytes, need);
    if (rc) return rc;
    return pv_conv3d_general_bwd_weight_f32(x, dy, dy_gate, dw, dbias, &g, ws, ws_bytes, stream);
  }
  const WgPlan p = wg_plan(n, c_in, c_out, h_in - 2, w_in - 2);
  return run_wgrad<SRC_PLAIN, SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                         plain_in(dy, dy_gate, c_out, h_in - 2, w_in - 2), 0, p, dw, dbias, false, ws,
                                         ws_bytes, as_stream(stream));
}

int pv_conv2d_ae_pool_bwd_weight_f32(const float* x, const float* dy_pooled, const uint8_t* codes, float* dw, float* dbias,
                                     int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                     size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_ae_pool_bwd_weight_f32";
  PV_REQUIRE(x && dy_pooled && codes && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_POOL);
  if (rc) return rc;
  if (general_route(n, h_in, w_in)) {
    const pv_conv3d_geom g = conv3d_geom_1x3x3(n, c_in, c_out, h_in, w_in);
    const size_t dz_bytes = pre_pool_bytes(n, c_out, h_in, w_in);
    size_t need = 0;
    rc = pv_conv3d_general_bwd_weight_workspace_bytes(&g, &need);
    if (rc) return rc;
    rc = check_workspace(who, ws, ws_bytes, dz_bytes + need);
    if (rc) return rc;
    float* dz = (float*)ws;
    const size_t elems = (size_t)n * c_out * (h_in - 2) * (w_in - 2);
    pool3_expand_f32<<<dim3(stream_grid(elems, kBlock)), dim3(kBlock), 0, as_stream(stream)>>>(
        dy_pooled, codes, dz, n * c_out, h_in - 2, w_in - 2, (h_in - 2) / 3, (w_in - 2) / 3);
    rc = check_launch(who);
    if (rc) return rc;
    return pv_conv3d_general_bwd_weight_f32(x, dz, nullptr, dw, dbias, &g, (char*)ws + dz_bytes, ws_bytes - dz_bytes, stream);
  }
  const WgPlan p = wg_plan(n, c_in, c_out, (h_in - 2) / 3 * 3, (w_in - 2) / 3 * 3);
  return run_wgrad<SRC_PLAIN, SRC_POOLED>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                          pooled_in(dy_pooled, codes, c_out, h_in - 2, w_in - 2), 0, p, dw, dbias, false,
                                          ws, ws_bytes, as_stream(stream));
}

int pv_convt2d_ae_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                          int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_ae_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  Fwd a = full_fwd_args(w, bias, y, c_out, h_in, w_in, relu);
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  hipStream_t st = as_stream(stream);
  if (c_in == 32 && c_out == 32) return run_fwd<32, 2, SRC_PLAIN, false>(who, a, n, st);
  if (c_in == 32) return run_fwd<32, 1, SRC_PLAIN, false>(who, a, n, st);
  return run_fwd<16, 1, SRC_PLAIN, false>(who, a, n, st);
}

int pv_convt2d_ae_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                               int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_convt2d_ae_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  // a valid conv of dy [n][c_out][h + 2][w + 2] with the unmirrored weights, [c_in][c_out][3][3] read as [m][c]
  Fwd a = conv_fwd_args(w, nullptr, dx, c_out, c_in, h_in + 2, w_in + 2, 0);
  a.in = plain_in(dy, dy_gate, c_out, h_in + 2, w_in + 2);
  a.out_gate = x_gate;
  hipStream_t st = as_stream(stream);
  if (c_in == 32 && c_out == 32) return run_fwd<32, 2, SRC_PLAIN, false>(who, a, n, st);
  if (c_in == 32) return run_fwd<16, 2, SRC_PLAIN, false>(who, a, n, st);
  if (c_out == 16) return run_fwd<16, 1, SRC_PLAIN, false>(who, a, n, st);
  return run_fwd<4, 1, SRC_PLAIN, false>(who, a, n, st);
}

int pv_convt2d_ae_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                             size_t* bytes) {
  const char* who = "pv_convt2d_ae_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  *bytes = wg_plan(n, c_in, c_out, h_in + 2, w_in + 2).ws;
  return PV_OK;
}

int pv_convt2d_ae_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                                 int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                 void* stream) {
  const char* who = "pv_convt2d_ae_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_ae(who, n, c_in, c_out, h_in, w_in, KIND_CONVT);
  if (rc) return rc;
  const WgPlan p = wg_plan(n, c_in, c_out, h_in + 2, w_in + 2);
  return run_wgrad<SRC_PLAIN, SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                         plain_in(dy, dy_gate, c_out, h_in + 2, w_in + 2), 2, p, dw, dbias, true, ws,
                                         ws_bytes, as_stream(stream));
}

int pv_conv2d_ae_frame_stripe_fwd_f32(const float* history, const int32_t* stripe_start, const float* w, const float* bias,
                                      float* y, int32_t n, int32_t frames, int32_t h, int32_t w_img, int32_t c_out,
                                      int32_t stripe_width, void* stream) {
  const char* who = "pv_conv2d_ae_frame_stripe_fwd_f32";
  PV_REQUIRE(history && stripe_start && w && bias && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frame_stripe(who, n, frames, h, w_img, c_out, stripe_width);
  if (rc) return rc;
  Fwd a = conv_fwd_args(w, bias, y, 2, c_out, h, w_img, 1);
  a.in = frame_stripe_in(history, stripe_start, frames, stripe_width, h, w_img);
  return run_fwd<4, 1, SRC_STRIPE, false>(who, a, n * frames, as_stream(stream));
}

int pv_conv2d_ae_frame_stripe_bwd_weight_workspace_bytes(int32_t n, int32_t frames, int32_t h, int32_t w_img, size_t* bytes) {
  const char* who = "pv_conv2d_ae_frame_stripe_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frame_stripe(who, n, frames, h, w_img, kFrameStripeC, 0);
  if (rc) return rc;
  *bytes = wg_plan(n * frames, 2, kFrameStripeC, h - 2, w_img - 2).ws;
  return PV_OK;
}

int pv_conv2d_ae_frame_stripe_bwd_weight_f32(const float* history, const int32_t* stripe_start, const float* dy, float* dw,
                                             float* dbias, int32_t n, int32_t frames, int32_t h, int32_t w_img, int32_t c_out,
                                             int32_t stripe_width, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_conv2d_ae_frame_stripe_bwd_weight_f32";
  PV_REQUIRE(history && stripe_start && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_frame_stripe(who, n, frames, h, w_img, c_out, stripe_width);
  if (rc) return rc;
  // 9 * 2 + 1 = 19 columns: two column tiles, one per wave, against one 16-row tile
  const WgPlan p = wg_plan(n * frames, 2, kFrameStripeC, h - 2, w_img - 2);
  return launch_wgrad<1, 1, SRC_STRIPE, SRC_PLAIN>(who, frame_stripe_in(history, stripe_start, frames, stripe_width, h, w_img),
                                                   plain_in(dy, nullptr, kFrameStripeC, h - 2, w_img - 2), 0, p, dw, dbias,
                                                   false, ws, ws_bytes, as_stream(stream));
}

int pv_conv2d_ae_p2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                            int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_conv2d_ae_p2_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_p2(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  // pv_convt2d_ae_fwd_f32's padded form with the weight [c_out][c_in][3][3] read as it lies: [m][c], unmirrored
  Fwd a = full_fwd_args(w, bias, y, c_out, h_in, w_in, relu);
  a.w_sm = c_in * 9, a.w_sc = 9, a.flip = 0;
  a.in = plain_in(x, nullptr, c_in, h_in, w_in);
  return run_fwd<32, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_p2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                 int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_conv2d_ae_p2_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  int rc = check_p2(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  // pv_convt2d_ae_bwd_data_f32's valid conv of dy [n][c_out][h + 2][w + 2], the weight [c_out][c_in][3][3] read as [c][m],
  // mirrored
  Fwd a = conv_fwd_args(w, nullptr, dx, c_out, c_in, h_in + 2, w_in + 2, 0);
  a.w_sm = 9, a.w_sc = c_in * 9, a.flip = 1;
  a.in = plain_in(dy, dy_gate, c_out, h_in + 2, w_in + 2);
  a.out_gate = x_gate;
  return run_fwd<32, 2, SRC_PLAIN, false>(who, a, n, as_stream(stream));
}

int pv_conv2d_ae_p2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                               size_t* bytes) {
  const char* who = "pv_conv2d_ae_p2_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_p2(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  *bytes = wg_plan(n, c_in, c_out, h_in + 2, w_in + 2).ws;
  return PV_OK;
}

int pv_conv2d_ae_p2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias, int32_t n,
                                   int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws, size_t ws_bytes,
                                   void* stream) {
  const char* who = "pv_conv2d_ae_p2_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  int rc = check_p2(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  // pv_convt2d_ae_bwd_weight_f32's sum with the slab sum untransposed: dw[co][ci][tap] = D[co][(ci, tap)]
  const WgPlan p = wg_plan(n, c_in, c_out, h_in + 2, w_in + 2);
  return run_wgrad<SRC_PLAIN, SRC_PLAIN>(who, plain_in(x, nullptr, c_in, h_in, w_in),
                                         plain_in(dy, dy_gate, c_out, h_in + 2, w_in + 2), 2, p, dw, dbias, false, ws,
                                         ws_bytes, as_stream(stream));
}

int pv_mse_window_norm_f32(const float* y_hat, const void* target, int32_t target_is_i16, int32_t n, int32_t out_h,
                           int32_t out_w, int32_t target_h, int32_t target_w, int32_t row0, int32_t col0, float* loss,
                           float* dy_hat, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "pv_mse_window_norm_f32";
  PV_REQUIRE(y_hat && target && loss, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(n > 0 && out_h > 0 && out_w > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(row0 >= 0 && col0 >= 0 && row0 + out_h <= target_h && col0 + out_w <= target_w, PV_ESIZE,
             "%s: the %d x %d window at (%d, %d) leaves the %d x %d target", who, out_h, out_w, row0, col0, target_h,
             target_w);
  PV_REQUIRE((long long)n * target_h * target_w < (1LL << 31), PV_ESIZE, "%s: tensor beyond 2^31 elements", who);
  int rc = check_workspace(who, ws, ws_bytes, (size_t)n * sizeof(float));
  if (rc) return rc;
  const float inv_count = (float)(1.0 / ((double)n * out_h * out_w));
  hipStream_t st = as_stream(stream);
  mse_window_norm_partial<<<dim3((unsigned)n), dim3(kBlock), 0, st>>>(y_hat, target, target_is_i16, out_h, out_w, target_h,
                                                                     target_w, row0, col0, inv_count, dy_hat, (float*)ws);
  rc = check_launch(who);
  if (rc) return rc;
  mse_window_norm_final<<<dim3(1), dim3(kBlock), 0, st>>>((const float*)ws, n, inv_count, loss);
  return check_launch(who);
}

int pv_mse_crop_norm_f32(const float* y_hat, const void* target, int32_t target_is_i16, int32_t n, int32_t out_h,
                         int32_t out_w, int32_t target_h, int32_t target_w, float* loss, float* dy_hat, void* ws,
                         size_t ws_bytes, void* stream) {
  const char* who = "pv_mse_crop_norm_f32";
  PV_REQUIRE(y_hat && target && loss, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(n > 0 && out_h > 0 && out_w > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(target_h - 2 * kCrop == out_h && target_w - 2 * kCrop == out_w, PV_ESIZE,
             "%s: target side %d x %d does not match the output %d x %d plus the %d-pixel crop on each side", who, target_h,
             target_w, out_h, out_w, kCrop);
  return pv_mse_window_norm_f32(y_hat, target, target_is_i16, n, out_h, out_w, target_h, target_w, kCrop, kCrop, loss,
                                dy_hat, ws, ws_bytes, stream);
}

}  // extern "C"
