// What the three exact-f32 Conv2d 3x3 files share: conv2d_f32.hip (experiments/002, 17 / 32 -> 32 / 4 channels),
// conv2d_pool_f32.hip (experiments/001, 144 channels with fused MaxPool2d(3)) and conv2d_ae_f32.hip (notebooks/16_maxpool:
// Conv2d / ConvTranspose2d up to 128 wide).  Their main loops stay in their own files; this header holds the ordered slab
// sum of their weight gradients (also in the ConvTranspose2d layout), the five synthesised input channels of the two
// experiments and the argument checks all repeat.
#pragma once
#include "pv_common.h"

namespace pv {
namespace {

constexpr int kBlock = 256;   // 4 waves

typedef __attribute__((ext_vector_type(4))) float acc4;

// dw[co][j] = sum_s slabs[s][co][j] (j < k9), dbias[co] = sum_s slabs[s][co][k9] in a fixed order: block = 32 elements x 8
// slab groups; group g adds slabs g, g + 8, ... into four interleaved partial sums (independent loads in flight), then
// the four and the 8 groups' results are added in index order.  dw or db may be null (that part is not written).
// TRANSPOSED: j = ci * 9 + tap' is stored as dw[ci][co][8 - tap'] (a ConvTranspose2d's [c_in][c_out][3][3] layout).
constexpr int kSumElems = 32, kSumGroups = kBlock / kSumElems;
template <bool TRANSPOSED>
__global__ __launch_bounds__(kBlock) void conv2d_slab_sum_f32(const float* __restrict__ slabs, float* __restrict__ dw,
                                                              float* __restrict__ db, int c_out, int k9, int n_slabs) {
  __shared__ float part[kSumGroups][kSumElems];
  const int ncols = k9 + 1, total = c_out * ncols;
  const int le = threadIdx.x % kSumElems, g = threadIdx.x / kSumElems;
  const int e = blockIdx.x * kSumElems + le;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (e < total) {
    int i = g;
    for (; i + 3 * kSumGroups < n_slabs; i += 4 * kSumGroups)
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += slabs[(size_t)(i + u * kSumGroups) * total + e];
    for (; i < n_slabs; i += kSumGroups) s[0] += slabs[(size_t)i * total + e];
  }
  part[g][le] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (g != 0 || e >= total) return;
  float t = part[0][le];
#pragma unroll
  for (int j = 1; j < kSumGroups; ++j) t += part[j][le];
  const int co = e / ncols, j = e - co * ncols;
  if (j < k9) {
    if (!dw) return;
    if (TRANSPOSED) dw[((j / 9) * c_out + co) * 9 + 8 - j % 9] = t;
    else dw[co * k9 + j] = t;
  } else if (db) {
    db[co] = t;
  }
}

// launch of the slab sum over a [c_out][k9 + 1] gradient
inline void launch_slab_sum(const void* ws, float* dw, float* db, int c_out, int k9, int n_slabs, hipStream_t st,
                            bool transposed = false) {
  const int total = c_out * (k9 + 1);
  const dim3 grid((unsigned)((total + kSumElems - 1) / kSumElems)), block(kBlock);
  if (transposed) conv2d_slab_sum_f32<true><<<grid, block, 0, st>>>((const float*)ws, dw, db, c_out, k9, n_slabs);
  else conv2d_slab_sum_f32<false><<<grid, block, 0, st>>>((const float*)ws, dw, db, c_out, k9, n_slabs);
}

// The five synthesised channels of both experiments (k = 0..4: centre marker, geo x, geo y, pixel x, pixel y) at input row
// r, column c; xc_b / yc_b are the example's geo coordinates along columns / rows.
__device__ __forceinline__ float synth_channel(int k, int r, int c, int centre_r, int centre_c, const float* xc_b,
                                               const float* yc_b) {
  switch (k) {
    case 0:   // centre marker: 1 on rows [centre_r - 2, centre_r + 2) and columns [centre_c - 2, centre_c + 2)
      return (r >= centre_r - 2 && r < centre_r + 2 && c >= centre_c - 2 && c < centre_c + 2) ? 1.0f : 0.0f;
    case 1: return __fdiv_rn(xc_b[c] - 309000.0f, 316387.42073603f);   // (x - SAT_X_MEAN) / SAT_X_STD in f32
    case 2: return __fdiv_rn(yc_b[r] - 519000.0f, 406454.17945938f);   // (y - SAT_Y_MEAN) / SAT_Y_STD in f32
    case 3: return __fdiv_rn((float)(c - 64), 37.0f);                  // (arange(S) - 64) / 37 along the last axis
    case 4: return __fdiv_rn((float)(r - 64), 37.0f);                  // ... and along rows
    default: return 0.0f;                                               // channels padded to a multiple of 4
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// positive extents, a 3x3 kernel that fits, every tensor of the conv within 32-bit indexing
inline int check_conv_dims(const char* who, int n, int c_in, int c_out, int h_in, int w_in) {
  PV_REQUIRE(n > 0 && c_in > 0 && c_out > 0, PV_EINVAL, "%s: non-positive dimension", who);
  PV_REQUIRE(h_in >= 3 && w_in >= 3, PV_ESIZE, "%s: spatial extent %d x %d smaller than the 3x3 kernel", who, h_in, w_in);
  PV_REQUIRE((long long)n * std::max(c_in, c_out) * h_in * w_in < (1LL << 31), PV_ESIZE,
             "%s: tensor beyond 2^31 elements (32-bit indexing)", who);
  return PV_OK;
}

inline int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  PV_REQUIRE(ws && ws_bytes >= need, PV_EINVAL, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, need);
  return PV_OK;
}

}  // namespace
}  // namespace pv
