// The convolution over time of notebooks/11_just_conv_and_conv_over_time.ipynb (the LitAutoEncoder cell, self.temporal_conv,
// raw lines 1418-1426 and 1446-1451): nn.Conv2d 1 -> 16 (1, 2), ReLU, Conv2d 16 -> 16 (1, 2), ReLU, Conv2d 16 -> 1 (1, 2) over
// the [B, 1, P, 4] "image" whose row p holds pixel p of the per-frame conv stack's four outputs.  Each pixel is a network
// of its own, 4 -> 16 x 3 -> 16 x 2 -> 1 with 609 shared parameters and about 1.2 k multiply-adds, so one thread takes one
// pixel and keeps every intermediate in registers: the notebook's [B, 16, P, 3] and [B, 16, P, 2] tensors, its view and its
// concatenation are never stored.
//
// Layout.  u is the stack's output as it lies, [frames B][1][s'][s'] = [B][4][P]: pixel p of example b reads u[(4 b + f) P +
// p], f = 0..3, coalesced per frame; y and dy are [B][P]; du has u's layout.  The parameters are wave-uniform: every index into
// them is a compile-time constant of the unrolled loops, so they arrive through scalar loads and feed the FMAs as scalar
// operands (no LDS traffic and no vector register per weight).  Exact f32, one rounding per fused multiply-add, fixed order.
//
// Backward, one launch plus the ordered slab sums: a thread recomputes its pixel's two hidden layers, gates by the recomputed
// values, writes du, and the block reduces the parameter gradients over its pixels in LDS.  The 16 x 32 gradient of the
// middle layer is an outer product per pixel: the block stages (gated gradient [2][16], first hidden layer [3][16]) per pixel
// and thread (c, ci) sums its two taps over the staged pixels; the 97 small sums (first and last layer, the biases) go the same
// way from a second staging of (dy h2, gated first-layer gradient, u, dy).  A record is 85 floats, an odd stride, so the 64
// lanes' writes fall on 64 banks; the reduction reads are broadcasts of at most 16 consecutive words.  128 pixels are staged
// at a time (43.5 KB), the block's 256 in two halves.  A block owns a fixed run of 256-pixel chunks and writes its partial
// sums to its own workspace slab; conv2d_slab_sum_f32 adds the slabs in slab order: no atomics, identical bits run to run.
// As compiled the forward is 80 vector registers with every weight a scalar operand; the backward is 208, no scratch, and
// moves about 1000 scalar registers through vector lanes (v_writelane / v_readlane) around its two passes over the middle
// layer's weight, which costs issue slots and is not yet understood.
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int kTimeFrames = 4, kTimeC = 16;        // N_HIST_IMAGES, CHANNELS // 2
constexpr int kTimeSlabs = 512;                    // at most this many blocks, each with its slab
constexpr int kStagePix = 128, kRec = 85;          // pixels staged at a time; floats per staged pixel (odd)
constexpr int kW2Cols = 2 * kTimeC;                // a row of the middle layer's weight: [ci][k]
constexpr int kSlabFloats = kTimeC * (kW2Cols + 1) + kTimeC * 3 + (kW2Cols + 1);      // 528 + 48 + 33 = 609

// the two hidden layers of one pixel from its four frame values; the forward and the backward's recomputation share the
// order of every sum, so the backward's gates are the forward's
__device__ __forceinline__ void hidden_layers(const float (&u)[kTimeFrames], const float* __restrict__ w1,
                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                              const float* __restrict__ b2, float (&h1)[kTimeC][3], float (&h2)[kTimeC][2]) {
#pragma unroll
  for (int c = 0; c < kTimeC; ++c) {
    const float wa = w1[2 * c], wb = w1[2 * c + 1], bc = b1[c];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const float z = fmaf(wb, u[t + 1], fmaf(wa, u[t], bc));
      h1[c][t] = fmaxf(z, 0.0f);
    }
  }
#pragma unroll
  for (int c = 0; c < kTimeC; ++c) {
    float z0 = b2[c], z1 = z0;
#pragma unroll
    for (int ci = 0; ci < kTimeC; ++ci) {
      const float wa = w2[(c * kTimeC + ci) * 2], wb = w2[(c * kTimeC + ci) * 2 + 1];
      z0 = fmaf(wb, h1[ci][1], fmaf(wa, h1[ci][0], z0));
      z1 = fmaf(wb, h1[ci][2], fmaf(wa, h1[ci][1], z1));
    }
    h2[c][0] = fmaxf(z0, 0.0f);
    h2[c][1] = fmaxf(z1, 0.0f);
  }
}

__global__ __launch_bounds__(kBlock) void conv_time_fwd(const float* __restrict__ u, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, const float* __restrict__ w3,
                                                        const float* __restrict__ b3, float* __restrict__ y, int p_per_ex,
                                                        int total) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= total) return;
  const int b = q / p_per_ex, p = q - b * p_per_ex;
  const float* ub = u + (size_t)b * kTimeFrames * p_per_ex + p;
  float uv[kTimeFrames];
#pragma unroll
  for (int f = 0; f < kTimeFrames; ++f) uv[f] = ub[(size_t)f * p_per_ex];
  float h1[kTimeC][3], h2[kTimeC][2];
  hidden_layers(uv, w1, b1, w2, b2, h1, h2);
  float z = b3[0];
#pragma unroll
  for (int c = 0; c < kTimeC; ++c) z = fmaf(w3[2 * c + 1], h2[c][1], fmaf(w3[2 * c], h2[c][0], z));
  y[q] = z;
}

// slabs: three regions, each [n_slabs][rows][cols + 1] as conv2d_slab_sum_f32 reads them: the middle layer [16][32 + 1] (the
// last column its bias), the first layer [16][2 + 1], the last layer [1][32 + 1]
__global__ __launch_bounds__(kBlock) void conv_time_bwd(const float* __restrict__ u, const float* __restrict__ dy,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2,
                                                        const float* __restrict__ w3, float* __restrict__ du,
                                                        float* __restrict__ slabs, int p_per_ex, int total, int chunks, int per,
                                                        int n_slabs, int gate_du) {
  __shared__ float st[kStagePix * kRec];
  const int tid = threadIdx.x;
  const int rc = tid >> 4, rci = tid & 15;        // phase 1: this thread's row c and input channel ci of the middle layer
  float acc_w2[2] = {0.0f, 0.0f}, acc_b2 = 0.0f, acc_small = 0.0f;

  const int it1 = min((int)(blockIdx.x + 1) * per, chunks);
  for (int it = blockIdx.x * per; it < it1; ++it) {
    // The parameters are loop-invariant, and the first hidden layer's gradient reads the middle layer's weight a second time.
    // Left alone, the compiler issues each of the 609 scalar loads once, ahead of the loop, and holds the values (286
    // registers and scratch).  An offset of 0 that it cannot see through keeps the loads where they are used, and the
    // pointers keep their __restrict__, so the loads stay scalar.
    int z_fwd = 0, z_bwd = 0;
    asm volatile("" : "+s"(z_fwd), "+s"(z_bwd));
    const float *w1f = w1 + z_fwd, *b1f = b1 + z_fwd, *w2f = w2 + z_fwd, *b2f = b2 + z_fwd, *w3f = w3 + z_fwd;
    const float *w1b = w1 + z_bwd, *w2b = w2 + z_bwd;
    const int q = it * kBlock + tid;
    const bool valid = q < total;
    const int qq = valid ? q : 0;
    const int b = qq / p_per_ex, p = qq - b * p_per_ex;
    const size_t uoff = (size_t)b * kTimeFrames * p_per_ex + p;
    // a pixel beyond the end takes g = 0 and u = 0: every product below that reaches a parameter gradient has a factor g
    const float g = valid ? dy[qq] : 0.0f;
    float uv[kTimeFrames];
#pragma unroll
    for (int f = 0; f < kTimeFrames; ++f) uv[f] = valid ? u[uoff + (size_t)f * p_per_ex] : 0.0f;
    float h1[kTimeC][3], h2[kTimeC][2], dz2[kTimeC][2];
    hidden_layers(uv, w1f, b1f, w2f, b2f, h1, h2);
#pragma unroll
    for (int c = 0; c < kTimeC; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) dz2[c][t] = h2[c][t] > 0.0f ? g * w3f[2 * c + t] : 0.0f;

    // phase 1: dw2[c][ci][k] += sum_t dz2[c][t] h1[ci][t + k], db2[c] += dz2[c][0] + dz2[c][1]
    for (int half = 0; half < kBlock / kStagePix; ++half) {
      __syncthreads();   // the previous reduction's reads are done
      if (tid / kStagePix == half) {
        float* rec = st + (tid % kStagePix) * kRec;
#pragma unroll
        for (int c = 0; c < kTimeC; ++c) {
          rec[c] = dz2[c][0], rec[kTimeC + c] = dz2[c][1];
          rec[32 + c] = h1[c][0], rec[48 + c] = h1[c][1], rec[64 + c] = h1[c][2];
        }
      }
      __syncthreads();
#pragma unroll 2
      for (int pix = 0; pix < kStagePix; ++pix) {
        const float* rec = st + pix * kRec;
        const float d0 = rec[rc], d1 = rec[kTimeC + rc];
        const float a0 = rec[32 + rci], a1 = rec[48 + rci], a2 = rec[64 + rci];
        acc_w2[0] = fmaf(d1, a1, fmaf(d0, a0, acc_w2[0]));
        acc_w2[1] = fmaf(d1, a2, fmaf(d0, a1, acc_w2[1]));
        acc_b2 = (acc_b2 + d0) + d1;
      }
    }

    // the first hidden layer's gated gradient, then in place of h1: dz1[ci][s] = [h1 > 0] sum_c sum_{t + k = s} dz2[c][t] w2[c]
    // [ci][k]; c outermost, so the weight is read in the order it lies, as the forward reads it
    float dh[kTimeC][3];
#pragma unroll
    for (int ci = 0; ci < kTimeC; ++ci) dh[ci][0] = dh[ci][1] = dh[ci][2] = 0.0f;
#pragma unroll
    for (int c = 0; c < kTimeC; ++c) {
#pragma unroll
      for (int ci = 0; ci < kTimeC; ++ci) {
        const float wa = w2b[(c * kTimeC + ci) * 2], wb = w2b[(c * kTimeC + ci) * 2 + 1];
        dh[ci][0] = fmaf(wa, dz2[c][0], dh[ci][0]);
        dh[ci][1] = fmaf(wa, dz2[c][1], fmaf(wb, dz2[c][0], dh[ci][1]));
        dh[ci][2] = fmaf(wb, dz2[c][1], dh[ci][2]);
      }
    }
#pragma unroll
    for (int ci = 0; ci < kTimeC; ++ci)
#pragma unroll
      for (int s = 0; s < 3; ++s) h1[ci][s] = h1[ci][s] > 0.0f ? dh[ci][s] : 0.0f;
    // du[f] = sum_ci sum_{s + k = f} dz1[ci][s] w1[ci][k], zeroed where u <= 0 if u is a ReLU's output (gate_du)
    float d[kTimeFrames] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ci = 0; ci < kTimeC; ++ci) {
      const float wa = w1b[2 * ci], wb = w1b[2 * ci + 1];
      d[0] = fmaf(wa, h1[ci][0], d[0]);
      d[1] = fmaf(wa, h1[ci][1], fmaf(wb, h1[ci][0], d[1]));
      d[2] = fmaf(wa, h1[ci][2], fmaf(wb, h1[ci][1], d[2]));
      d[3] = fmaf(wb, h1[ci][2], d[3]);
    }
    if (valid) {
#pragma unroll
      for (int f = 0; f < kTimeFrames; ++f) du[uoff + (size_t)f * p_per_ex] = (gate_du && !(uv[f] > 0.0f)) ? 0.0f : d[f];
    }

    // phase 2: dw3[c][t] += g h2[c][t], db3 += g, dw1[ci][k] += sum_s dz1[ci][s] u[s + k], db1[ci] += sum_s dz1[ci][s]
    for (int half = 0; half < kBlock / kStagePix; ++half) {
      __syncthreads();
      if (tid / kStagePix == half) {
        float* rec = st + (tid % kStagePix) * kRec;
#pragma unroll
        for (int c = 0; c < kTimeC; ++c) {
          rec[c] = g * h2[c][0], rec[kTimeC + c] = g * h2[c][1];
          rec[32 + c] = h1[c][0], rec[48 + c] = h1[c][1], rec[64 + c] = h1[c][2];
        }
#pragma unroll
        for (int f = 0; f < kTimeFrames; ++f) rec[80 + f] = uv[f];
        rec[84] = g;
      }
      __syncthreads();
      if (tid < 32) {                              // dw3, flat index 2 c + t
        const int off = (tid & 1) * kTimeC + (tid >> 1);
#pragma unroll 4
        for (int pix = 0; pix < kStagePix; ++pix) acc_small += st[pix * kRec + off];
      } else if (tid == 32) {                      // db3
#pragma unroll 4
        for (int pix = 0; pix < kStagePix; ++pix) acc_small += st[pix * kRec + 84];
      } else if (tid < 65) {                       // dw1, flat index 2 ci + k
        const int ci = (tid - 33) >> 1, k = (tid - 33) & 1;
#pragma unroll 4
        for (int pix = 0; pix < kStagePix; ++pix) {
          const float* rec = st + pix * kRec;
          acc_small = fmaf(rec[64 + ci], rec[82 + k], fmaf(rec[48 + ci], rec[81 + k], fmaf(rec[32 + ci], rec[80 + k], acc_small)));
        }
      } else if (tid < 81) {                       // db1
        const int ci = tid - 65;
#pragma unroll 4
        for (int pix = 0; pix < kStagePix; ++pix) {
          const float* rec = st + pix * kRec;
          acc_small += (rec[32 + ci] + rec[48 + ci]) + rec[64 + ci];
        }
      }
    }
  }

  // this block's slab of each region
  float* s2 = slabs + (size_t)blockIdx.x * (kTimeC * (kW2Cols + 1));
  float* s1 = slabs + (size_t)n_slabs * (kTimeC * (kW2Cols + 1)) + (size_t)blockIdx.x * (kTimeC * 3);
  float* s3 = slabs + (size_t)n_slabs * (kTimeC * (kW2Cols + 1) + kTimeC * 3) + (size_t)blockIdx.x * (kW2Cols + 1);
  s2[rc * (kW2Cols + 1) + 2 * rci] = acc_w2[0];
  s2[rc * (kW2Cols + 1) + 2 * rci + 1] = acc_w2[1];
  if (rci == 0) s2[rc * (kW2Cols + 1) + kW2Cols] = acc_b2;
  if (tid < 32) s3[tid] = acc_small;
  else if (tid == 32) s3[kW2Cols] = acc_small;
  else if (tid < 65) s1[((tid - 33) >> 1) * 3 + ((tid - 33) & 1)] = acc_small;
  else if (tid < 81) s1[(tid - 65) * 3 + 2] = acc_small;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

struct TimePlan {
  int total, chunks, per, n_slabs;
  size_t ws;
};

// n examples of p pixels: 256-pixel chunks cut into at most kTimeSlabs runs of `per` chunks, one block and one slab each
int time_plan(const char* who, int n, int frames, int c_mid, int p, TimePlan& t) {
  PV_REQUIRE(n > 0 && p > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(frames == kTimeFrames && c_mid == kTimeC, PV_ESIZE,
             "%s: unsupported channel counts frames=%d c_mid=%d (%d frames, %d channels)", who, frames, c_mid, kTimeFrames,
             kTimeC);
  PV_REQUIRE((long long)n * kTimeFrames * p < (1LL << 31) - kBlock, PV_ESIZE, "%s: tensor beyond 2^31 elements (32-bit indexing)",
             who);
  t.total = n * p;
  t.chunks = (t.total + kBlock - 1) / kBlock;
  const int want = std::min(t.chunks, kTimeSlabs);
  t.per = (t.chunks + want - 1) / want;
  t.n_slabs = (t.chunks + t.per - 1) / t.per;
  t.ws = (size_t)t.n_slabs * kSlabFloats * sizeof(float);
  return PV_OK;
}

}  // namespace
}  // namespace pv

using namespace pv;

extern "C" {

int pv_conv_time_fwd_f32(const float* u, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                         const float* b3, float* y, int32_t n, int32_t frames, int32_t c_mid, int32_t p, void* stream) {
  const char* who = "pv_conv_time_fwd_f32";
  PV_REQUIRE(u && w1 && b1 && w2 && b2 && w3 && b3 && y, PV_EINVAL, "%s: null pointer", who);
  TimePlan t;
  int rc = time_plan(who, n, frames, c_mid, p, t);
  if (rc) return rc;
  conv_time_fwd<<<dim3((unsigned)t.chunks), dim3(kBlock), 0, as_stream(stream)>>>(u, w1, b1, w2, b2, w3, b3, y, p, t.total);
  return check_launch(who);
}

int pv_conv_time_bwd_workspace_bytes(int32_t n, int32_t frames, int32_t c_mid, int32_t p, size_t* bytes) {
  const char* who = "pv_conv_time_bwd_workspace_bytes";
  PV_REQUIRE(bytes, PV_EINVAL, "%s: null pointer", who);
  TimePlan t;
  int rc = time_plan(who, n, frames, c_mid, p, t);
  if (rc) return rc;
  *bytes = t.ws;
  return PV_OK;
}

int pv_conv_time_bwd_f32(const float* u, const float* dy, const float* w1, const float* b1, const float* w2, const float* b2,
                         const float* w3, float* du, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3,
                         int32_t n, int32_t frames, int32_t c_mid, int32_t p, int32_t u_is_relu_output, void* ws, size_t ws_bytes,
                         void* stream) {
  const char* who = "pv_conv_time_bwd_f32";
  PV_REQUIRE(u && dy && w1 && b1 && w2 && b2 && w3 && du && dw1 && db1 && dw2 && db2 && dw3 && db3, PV_EINVAL,
             "%s: null pointer", who);
  TimePlan t;
  int rc = time_plan(who, n, frames, c_mid, p, t);
  if (rc) return rc;
  rc = check_workspace(who, ws, ws_bytes, t.ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  float* slabs = (float*)ws;
  conv_time_bwd<<<dim3((unsigned)t.n_slabs), dim3(kBlock), 0, st>>>(u, dy, w1, b1, w2, b2, w3, du, slabs, p, t.total, t.chunks,
                                                                   t.per, t.n_slabs, u_is_relu_output ? 1 : 0);
  rc = check_launch(who);
  if (rc) return rc;
  const float* r1 = slabs + (size_t)t.n_slabs * (kTimeC * (kW2Cols + 1));
  const float* r3 = r1 + (size_t)t.n_slabs * (kTimeC * 3);
  launch_slab_sum(slabs, dw2, db2, kTimeC, kW2Cols, t.n_slabs, st);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(r1, dw1, db1, kTimeC, 2, t.n_slabs, st);
  rc = check_launch(who);
  if (rc) return rc;
  launch_slab_sum(r3, dw3, db3, 1, kW2Cols, t.n_slabs, st);
  return check_launch(who);
}

}  // extern "C"
