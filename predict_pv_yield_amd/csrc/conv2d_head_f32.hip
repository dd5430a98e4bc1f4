// The one-output-channel 3x3 last layers of the wide frame predictors (notebooks 09, 10 and 12) in exact f32.  One output
// channel would use 1/16 of a matrix tile and the layers are bandwidth-bound, so this is plain vector code with every sum in
// a fixed order:
//   pv_conv2d_head_s2_*    Conv2d, stride 2, padding 2 (notebook 10): x [n][c_in][h][w] -> y [n][1][ho][wo], ho = (h + 1) / 2 + 1
//   pv_conv2d_head_s2p1_*  Conv2d, stride 2, padding 1 (notebook 12, whose last Conv3d on depth 2 is exactly this on the free
//                          views x [n][2 c][h][w] and w [1][2 c][3][3]): ho = (h - 1) / 2 + 1
//   pv_convt2d_head_*      ConvTranspose2d, stride 1 (notebook 09): y [n][1][h + 2][w + 2]
// The two strided heads are one set of three kernels at PAD = 2 and 1: output (oh, ow) reads rows 2 oh - PAD + kh, columns
// 2 ow - PAD + kw.  The transposed head has its own tap rule (output (oh, ow) reads x (oh - kh, ow - kw) with weight
// w[ci][0][kh][kw]) and bias-gradient rule, so it keeps its three kernels; it shares the forward's body over a tap functor
// (head_forward) and the reduction of the weight gradient (head_reduce_store).  Any c_in.
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int kHeadDxPerBlock = 4 * kBlock;              // data gradient: elements of a plane per block
constexpr int kHeadBand = 16, kHeadMaxSlabs = 128;       // weight gradient: rows per item, slabs at most
constexpr int kHeadMaxW = 128;                           // widest input plane of the transposed head

// A forward, one output per thread: tap(oh, ow, t, ir, ic) names the input row and column that tap t of output (oh, ow) of
// the ho x wo plane reads (outside the image: 0).  The 9 taps of a channel are one fma chain, the channels go round-robin
// into four partial sums added in a fixed order, then the bias.
template <class Tap>
__device__ __forceinline__ void head_forward(const float* __restrict__ x, const float* __restrict__ w,
                                             const float* __restrict__ bias, float* __restrict__ y, int total, int c_in,
                                             int h, int wi, int ho, int wo, int relu, Tap tap) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int ow = idx % wo, oh = (idx / wo) % ho, b = idx / (wo * ho);
  int off[9];
  bool ok[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    int ir, ic;
    tap(oh, ow, t, ir, ic);
    ok[t] = ir >= 0 && ir < h && ic >= 0 && ic < wi;
    off[t] = ok[t] ? ir * wi + ic : 0;
  }
  const size_t plane = (size_t)h * wi;
  const float* xb = x + (size_t)b * c_in * plane;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int ci = 0; ci < c_in; ++ci) {
    const float* xp = xb + ci * plane;
    const float* wp = w + ci * 9;
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) s = fmaf(wp[t], ok[t] ? xp[off[t]] : 0.0f, s);
    acc[ci & 3] += s;
  }
  float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + (bias ? bias[0] : 0.0f);
  if (relu) v = v > 0.0f ? v : 0.0f;
  y[idx] = v;
}

// The tail of a weight gradient: the block adds its threads' ten sums (nine taps and the bias) in a fixed tree, lanes by
// shuffle and then the four waves in order, and writes them to its slab row [c_in * 9 + 1]: the taps of channel ci, and
// from channel 0 the last column, the bias gradient.
__device__ __forceinline__ void head_reduce_store(const float (&a)[10], float* __restrict__ slabs, int slab, int ci,
                                                  int c_in) {
  __shared__ float part[kBlock / 64][10];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    float v = a[t];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if (lane == 0) part[wave][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int t = threadIdx.x;
    const float v = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    const int ncols = c_in * 9 + 1;
    if (t < 9) slabs[(size_t)slab * ncols + ci * 9 + t] = v;
    else if (ci == 0) slabs[(size_t)slab * ncols + ncols - 1] = v;
  }
}

// ---- the strided heads: 3x3, stride 2, padding PAD -------------------------------------------------------------------------

// forward
template <int PAD>
__global__ __launch_bounds__(kBlock) void head_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ y, int total,
                                                   int c_in, int h, int wi, int ho, int wo, int relu) {
  head_forward(x, w, bias, y, total, c_in, h, wi, ho, wo, relu,
               [](int oh, int ow, int t, int& ir, int& ic) { ir = 2 * oh - PAD + t / 3, ic = 2 * ow - PAD + t % 3; });
}

// data gradient: every dx element is written once, from the at most four taps of its parity class.  Block = (1024 elements
// of a plane, input channel, image): the channel's nine weights are uniform over the block, one division per element.  (At
// PAD = 2 no tap row or column is negative.)
template <int PAD>
__global__ __launch_bounds__(kBlock) void head_bwd_data(const float* __restrict__ dy, const float* __restrict__ w,
                                                        float* __restrict__ dx, const float* __restrict__ x_gate,
                                                        int c_in, int h, int wi, int ho, int wo) {
  const int ci = blockIdx.y, b = blockIdx.z, plane = h * wi;
  const float* dyb = dy + (size_t)b * ho * wo;
  const float* wp = w + ci * 9;
  const size_t base = ((size_t)b * c_in + ci) * plane;
  const int p1 = min(plane, (int)(blockIdx.x + 1) * kHeadDxPerBlock);
  for (int p = blockIdx.x * kHeadDxPerBlock + threadIdx.x; p < p1; p += kBlock) {
    const int r = p / wi, c = p - r * wi;
    float s = 0.0f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int tr = r + PAD - kh;
      if ((PAD < 2 && tr < 0) || (tr & 1) || (tr >> 1) >= ho) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tc = c + PAD - kw;
        if ((PAD < 2 && tc < 0) || (tc & 1) || (tc >> 1) >= wo) continue;
        s = fmaf(wp[kh * 3 + kw], dyb[(tr >> 1) * wo + (tc >> 1)], s);
      }
    }
    if (x_gate && !(x_gate[base + p] > 0.0f)) s = 0.0f;
    dx[base + p] = s;
  }
}

// weight / bias gradient.  Block = (input channel, slab of (image, band of 16 output rows) items); every thread sums its
// positions' nine products (and dy itself), then head_reduce_store.
template <int PAD>
__global__ __launch_bounds__(kBlock) void head_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                     float* __restrict__ slabs, int c_in, int h, int wi, int ho, int wo,
                                                     int n_rb, int items, int per) {
  const int ci = blockIdx.x, slab = blockIdx.y;
  float a[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) a[t] = 0.0f;
  const int it0 = slab * per, it1 = min(it0 + per, items);
  for (int it = it0; it < it1; ++it) {
    const int rb = it % n_rb, b = it / n_rb;
    const int oh0 = rb * kHeadBand, rows = min(kHeadBand, ho - oh0);
    const float* xp = x + ((size_t)b * c_in + ci) * h * wi;
    const float* dyb = dy + (size_t)b * ho * wo;
    for (int p = threadIdx.x; p < rows * wo; p += kBlock) {
      const int oh = oh0 + p / wo, ow = p % wo;
      const float g = dyb[oh * wo + ow];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ir = 2 * oh - PAD + t / 3, ic = 2 * ow - PAD + t % 3;
        const float v = (ir >= 0 && ir < h && ic >= 0 && ic < wi) ? xp[ir * wi + ic] : 0.0f;
        a[t] = fmaf(g, v, a[t]);
      }
      a[9] += g;
    }
  }
  head_reduce_store(a, slabs, slab, ci, c_in);
}

// ---- the ConvTranspose2d head: 3x3, stride 1 ---------------------------------------------------------------------------------

// forward
__global__ __launch_bounds__(kBlock) void headt_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ y, int total,
                                                    int c_in, int h, int wi, int relu) {
  head_forward(x, w, bias, y, total, c_in, h, wi, h + 2, wi + 2, relu,
               [](int oh, int ow, int t, int& ir, int& ic) { ir = oh - t / 3, ic = ow - t % 3; });
}

// data gradient: dx[ci][i][j] = sum_tap w[ci][tap] dy[i + kh][j + kw], every tap inside dy.  Block = (1024 elements of a
// plane, input channel, image): the channel's nine weights are uniform over the block
__global__ __launch_bounds__(kBlock) void headt_bwd_data(const float* __restrict__ dy, const float* __restrict__ w,
                                                         float* __restrict__ dx, const float* __restrict__ x_gate,
                                                         int c_in, int h, int wi) {
  const int ci = blockIdx.y, b = blockIdx.z, plane = h * wi, wo = wi + 2;
  const float* dyb = dy + (size_t)b * (h + 2) * wo;
  const float* wp = w + ci * 9;
  const size_t base = ((size_t)b * c_in + ci) * plane;
  const int p1 = min(plane, (int)(blockIdx.x + 1) * kHeadDxPerBlock);
  for (int p = blockIdx.x * kHeadDxPerBlock + threadIdx.x; p < p1; p += kBlock) {
    const int r = p / wi, c = p - r * wi;
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) s = fmaf(wp[t], dyb[(r + t / 3) * wo + c + t % 3], s);
    if (x_gate && !(x_gate[base + p] > 0.0f)) s = 0.0f;
    dx[base + p] = s;
  }
}

// weight / bias gradient.  Block = (input channel, slab of (image, band of 16 input rows) items); every thread sums its
// positions' nine products, then head_reduce_store.  The bias gradient runs over dy's own positions: channel 0's blocks add
// the band's dy rows (the last band also the two rows below it).
__global__ __launch_bounds__(kBlock) void headt_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ slabs, int c_in, int h, int wi, int n_rb,
                                                      int items, int per) {
  const int ci = blockIdx.x, slab = blockIdx.y, wo = wi + 2;
  float a[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) a[t] = 0.0f;
  const int it0 = slab * per, it1 = min(it0 + per, items);
  for (int it = it0; it < it1; ++it) {
    const int rb = it % n_rb, b = it / n_rb;
    const int i0 = rb * kHeadBand, rows = min(kHeadBand, h - i0);
    const float* xp = x + ((size_t)b * c_in + ci) * h * wi;
    const float* dyb = dy + (size_t)b * (h + 2) * wo;
    for (int p = threadIdx.x; p < rows * wi; p += kBlock) {
      const int i = i0 + p / wi, j = p % wi;
      const float v = xp[i * wi + j];
#pragma unroll
      for (int t = 0; t < 9; ++t) a[t] = fmaf(v, dyb[(i + t / 3) * wo + j + t % 3], a[t]);
    }
    if (ci == 0) {
      const int drows = rows + (rb == n_rb - 1 ? 2 : 0);
      for (int p = threadIdx.x; p < drows * wo; p += kBlock) a[9] += dyb[i0 * wo + p];
    }
  }
  head_reduce_store(a, slabs, slab, ci, c_in);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// a strided head: every tensor within 32-bit indexing
int check_head(const char* who, int n, int c_in, int c_out, int h_in, int w_in) {
  PV_REQUIRE(n > 0 && c_in > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(c_out == 1, PV_ESIZE, "%s: unsupported channel count c_out=%d (1)", who, c_out);
  PV_REQUIRE((long long)n * c_in * h_in * w_in < (1LL << 31), PV_ESIZE, "%s: tensor beyond 2^31 elements (32-bit indexing)",
             who);
  return PV_OK;
}

// the transposed head: output (h + 2) x (w + 2) at most kHeadMaxW + 2 wide, every tensor within 32-bit indexing
int check_headt(const char* who, int n, int c_in, int c_out, int h_in, int w_in) {
  PV_REQUIRE(n > 0 && c_in > 0 && h_in > 0 && w_in > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(c_out == 1, PV_ESIZE, "%s: unsupported channel count c_out=%d (1)", who, c_out);
  PV_REQUIRE(w_in <= kHeadMaxW, PV_ESIZE, "%s: width %d beyond %d", who, w_in, kHeadMaxW);
  PV_REQUIRE((long long)n * c_in * h_in * w_in < (1LL << 31) && (long long)n * (h_in + 2) * (w_in + 2) < (1LL << 31),
             PV_ESIZE, "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

// output side of a strided head at padding PAD
template <int PAD>
inline int head_out(int side) { return (side + 2 * PAD - 3) / 2 + 1; }

// the weight gradient's items (image, band of 16 of the `rows` rows the sum runs over) dealt to at most 128 fixed slabs
struct HeadPlan {
  int n_rb, items, per, n_slabs;
  size_t ws;
};

HeadPlan head_plan(int n, int c_in, int rows) {
  HeadPlan p;
  p.n_rb = (rows + kHeadBand - 1) / kHeadBand;
  p.items = n * p.n_rb;
  const int want = std::min(p.items, kHeadMaxSlabs);
  p.per = (p.items + want - 1) / want;
  p.n_slabs = (p.items + p.per - 1) / p.per;
  p.ws = (size_t)p.n_slabs * (c_in * 9 + 1) * sizeof(float);
  return p;
}

template <int PAD>
int run_head_fwd(const char* who, const float* x, const float* w, const float* bias, float* y, int n, int c_in, int c_out,
                 int h_in, int w_in, int relu, void* stream) {
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  const int ho = head_out<PAD>(h_in), wo = head_out<PAD>(w_in), total = n * ho * wo;
  head_fwd<PAD><<<dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream)>>>(
      x, w, bias, y, total, c_in, h_in, w_in, ho, wo, relu ? 1 : 0);
  return check_launch(who);
}

template <int PAD>
int run_head_bwd_data(const char* who, const float* dy, const float* dy_gate, const float* w, float* dx,
                      const float* x_gate, int n, int c_in, int c_out, int h_in, int w_in, void* stream) {
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(!dy_gate, PV_EINVAL, "%s: the head has no ReLU, so it takes no dy_gate", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(c_in <= 65535 && n <= 65535, PV_ESIZE, "%s: more than 65535 channels or images (grid axes)", who);
  head_bwd_data<PAD><<<dim3((unsigned)((h_in * w_in + kHeadDxPerBlock - 1) / kHeadDxPerBlock), (unsigned)c_in, (unsigned)n),
                       dim3(kBlock), 0, as_stream(stream)>>>(dy, w, dx, x_gate, c_in, h_in, w_in, head_out<PAD>(h_in),
                                                             head_out<PAD>(w_in));
  return check_launch(who);
}

template <int PAD>
int run_head_ws_bytes(const char* who, int n, int c_in, int c_out, int h_in, int w_in, size_t* bytes) {
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  *bytes = head_plan(n, c_in, head_out<PAD>(h_in)).ws;
  return PV_OK;
}

template <int PAD>
int run_head_bwd_weight(const char* who, const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                        int n, int c_in, int c_out, int h_in, int w_in, void* ws, size_t ws_bytes, void* stream) {
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(!dy_gate, PV_EINVAL, "%s: the head has no ReLU, so it takes no dy_gate", who);
  int rc = check_head(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  const int ho = head_out<PAD>(h_in), wo = head_out<PAD>(w_in);
  const HeadPlan p = head_plan(n, c_in, ho);
  rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  head_wgrad<PAD><<<dim3((unsigned)c_in, (unsigned)p.n_slabs), dim3(kBlock), 0, st>>>(x, dy, (float*)ws, c_in, h_in, w_in, ho,
                                                                                        wo, p.n_rb, p.items, p.per);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, dbias, 1, c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv2d_head_s2_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                              int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  return run_head_fwd<2>("pv_conv2d_head_s2_fwd_f32", x, w, bias, y, n, c_in, c_out, h_in, w_in, relu, stream);
}

int pv_conv2d_head_s2_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                   int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  return run_head_bwd_data<2>("pv_conv2d_head_s2_bwd_data_f32", dy, dy_gate, w, dx, x_gate, n, c_in, c_out, h_in, w_in,
                              stream);
}

int pv_conv2d_head_s2_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                 size_t* bytes) {
  return run_head_ws_bytes<2>("pv_conv2d_head_s2_bwd_weight_workspace_bytes", n, c_in, c_out, h_in, w_in, bytes);
}

int pv_conv2d_head_s2_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                     int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                     size_t ws_bytes, void* stream) {
  return run_head_bwd_weight<2>("pv_conv2d_head_s2_bwd_weight_f32", x, dy, dy_gate, dw, dbias, n, c_in, c_out, h_in, w_in,
                                ws, ws_bytes, stream);
}

int pv_conv2d_head_s2p1_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                                int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  return run_head_fwd<1>("pv_conv2d_head_s2p1_fwd_f32", x, w, bias, y, n, c_in, c_out, h_in, w_in, relu, stream);
}

int pv_conv2d_head_s2p1_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                     int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  return run_head_bwd_data<1>("pv_conv2d_head_s2p1_bwd_data_f32", dy, dy_gate, w, dx, x_gate, n, c_in, c_out, h_in, w_in,
                              stream);
}

int pv_conv2d_head_s2p1_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                                   size_t* bytes) {
  return run_head_ws_bytes<1>("pv_conv2d_head_s2p1_bwd_weight_workspace_bytes", n, c_in, c_out, h_in, w_in, bytes);
}

int pv_conv2d_head_s2p1_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                       int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                       size_t ws_bytes, void* stream) {
  return run_head_bwd_weight<1>("pv_conv2d_head_s2p1_bwd_weight_f32", x, dy, dy_gate, dw, dbias, n, c_in, c_out, h_in, w_in,
                                ws, ws_bytes, stream);
}

int pv_convt2d_head_fwd_f32(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c_in,
                            int32_t c_out, int32_t h_in, int32_t w_in, int32_t relu, void* stream) {
  const char* who = "pv_convt2d_head_fwd_f32";
  PV_REQUIRE(x && w && y, PV_EINVAL, "%s: null pointer", who);
  int rc = check_headt(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  const int total = n * (h_in + 2) * (w_in + 2);
  headt_fwd<<<dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream)>>>(
      x, w, bias, y, total, c_in, h_in, w_in, relu ? 1 : 0);
  return check_launch(who);
}

int pv_convt2d_head_bwd_data_f32(const float* dy, const float* dy_gate, const float* w, float* dx, const float* x_gate,
                                 int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* stream) {
  const char* who = "pv_convt2d_head_bwd_data_f32";
  PV_REQUIRE(dy && w && dx, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(!dy_gate, PV_EINVAL, "%s: the head has no ReLU, so it takes no dy_gate", who);
  int rc = check_headt(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(c_in <= 65535 && n <= 65535, PV_ESIZE, "%s: more than 65535 channels or images (grid axes)", who);
  headt_bwd_data<<<dim3((unsigned)((h_in * w_in + kHeadDxPerBlock - 1) / kHeadDxPerBlock), (unsigned)c_in, (unsigned)n),
                   dim3(kBlock), 0, as_stream(stream)>>>(dy, w, dx, x_gate, c_in, h_in, w_in);
  return check_launch(who);
}

int pv_convt2d_head_bwd_weight_workspace_bytes(int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in,
                                               size_t* bytes) {
  const char* who = "pv_convt2d_head_bwd_weight_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  int rc = check_headt(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  *bytes = head_plan(n, c_in, h_in).ws;
  return PV_OK;
}

int pv_convt2d_head_bwd_weight_f32(const float* x, const float* dy, const float* dy_gate, float* dw, float* dbias,
                                   int32_t n, int32_t c_in, int32_t c_out, int32_t h_in, int32_t w_in, void* ws,
                                   size_t ws_bytes, void* stream) {
  const char* who = "pv_convt2d_head_bwd_weight_f32";
  PV_REQUIRE(x && dy && dw && dbias, PV_EINVAL, "%s: null pointer", who);
  PV_REQUIRE(!dy_gate, PV_EINVAL, "%s: the head has no ReLU, so it takes no dy_gate", who);
  int rc = check_headt(who, n, c_in, c_out, h_in, w_in);
  if (rc) return rc;
  PV_REQUIRE(c_in <= 65535, PV_ESIZE, "%s: more than 65535 channels (grid axis)", who);
  const HeadPlan p = head_plan(n, c_in, h_in);
  rc = check_workspace(who, ws, ws_bytes, p.ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  headt_wgrad<<<dim3((unsigned)c_in, (unsigned)p.n_slabs), dim3(kBlock), 0, st>>>(x, dy, (float*)ws, c_in, h_in, w_in, p.n_rb,
                                                                                 p.items, p.per);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(ws, dw, dbias, 1, c_in * 9, p.n_slabs, st);
  return check_launch(who);
}

}  // extern "C"
