// What the stride-2 members of the VGPR-weight tile family share on top of conv2d_tile_f32.h: conv2d_s2_f32.hip (notebooks
// 14 / 15, 2-D) and conv3d_s2_f32.hip (notebook 08, the depth-2 Conv3d and the horizon ConvTranspose2d).  The weight
// gradient's tile plan and the ConvTranspose2d bias gradient (plane sums in slabs) are stated once here.
#pragma once
#include "conv2d_tile_f32.h"

namespace pv {
namespace {

inline int conv_out(int s) { return (s - 3) / 2 + 1; }

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The ConvTranspose2d bias gradient's slabs: block s adds dy (zeroed where the gate <= 0) over the planes of its images,
// channel by channel: strided partial sums per thread, then a tree sum in LDS (fixed order).  slabs [n_slabs][c][1].
__global__ __launch_bounds__(kBlock) void plane_sum_slabs_f32(const float* __restrict__ dy, const float* __restrict__ gate,
                                                             float* __restrict__ slabs, int n, int per, int c, int plane) {
  __shared__ float part[kBlock];
  const int n0 = blockIdx.x * per, n1 = min(n0 + per, n);
  for (int ch = 0; ch < c; ++ch) {
    float s = 0.0f;
    for (int img = n0; img < n1; ++img) {
      const size_t base = ((size_t)img * c + ch) * plane;
      for (int i = threadIdx.x; i < plane; i += kBlock) {
        const float v = dy[base + i];
        s += (gate && !(gate[base + i] > 0.0f)) ? 0.0f : v;
      }
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int k = kBlock / 2; k > 0; k >>= 1) {
      if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
      __syncthreads();
    }
    if (threadIdx.x == 0) slabs[(size_t)blockIdx.x * c + ch] = part[0];
    __syncthreads();
  }
}

// the bias slabs of a ConvTranspose2d weight gradient: one per group of `per` images, at most kMaxSlabs
inline void bias_slabs(int n, int& n_slabs, int& per) {
  const int want = std::min(n, kMaxSlabs);
  per = (n + want - 1) / want;
  n_slabs = (n + per - 1) / per;
}

// C: (h_out, w_out) = the positions the sum runs over, rows = the D rows, c = the sliding operand's channels.  Among column
// splits, the largest tile that fits 64 KB and 384 positions with the smallest staged area per position.
inline WgPlan wg_plan_s2(int n, int c, int rows, int h_out, int w_out) {
  WgPlan p = {};
  p.h_out = h_out, p.w_out = w_out, p.cinp = (c + 3) & ~3, p.mt = (rows + 15) / 16;
  double best = 1e30;
  const int cb0 = (w_out + 63) / 64;
  for (int n_cb = cb0; n_cb <= cb0 + 3 && n_cb <= w_out; ++n_cb) {
    const int tc = (w_out + n_cb - 1) / n_cb;
    int tr = 0;
    while (tr < h_out && (tr + 1) * tc <= 384 && wg_lds_floats(p.cinp, p.mt, tr + 1, tc, 2) <= (size_t)kLdsFloats) ++tr;
    if (tr == 0) continue;
    const int n_rb = (h_out + tr - 1) / tr;
    tr = (h_out + n_rb - 1) / n_rb;
    const double cost = (double)(2 * tr + 1) * (2 * tc + 1) / ((double)tr * tc);
    if (cost < best) best = cost, p.tr = tr, p.tc = tc, p.n_rb = n_rb, p.n_cb = (w_out + tc - 1) / tc;
  }
  if (p.tr == 0) p.tr = 1, p.tc = std::min(w_out, 8), p.n_rb = h_out, p.n_cb = (w_out + p.tc - 1) / p.tc;
  slab_split(p, n, c, rows, 2);
  return p;
}

}  // namespace
}  // namespace pv
