// The raw-counts first layer of notebooks 15 and 16 (normalise_images_in_model, then the horizon plane), stated once for
// conv2d_ae_f32.hip (stride 1) and conv2d_s2_f32.hip (stride 2): history [n][4][h][w] and the flow prediction [n][h][w] are
// read in place as int16 or f32 counts and normalised ((v - 93.23458) / 115.34247: subtract, then a true f32 divide) while
// they are staged; the horizon is a sixth, constant plane.  The same load serves the normalised MSE targets.
#pragma once
#include "conv2d_tile_f32.h"

namespace pv {
namespace {

constexpr float kCountMean = 93.23458f, kCountStd = 115.34247f;   // normalise_images_in_model

__device__ __forceinline__ float count_at(const void* p, int is_i16, size_t off) {
  const float v = is_i16 ? (float)((const int16_t*)p)[off] : ((const float*)p)[off];
  return __fdiv_rn(v - kCountMean, kCountStd);
}

// SRC_COUNTS: the four history frames and the flow prediction normalised in place, then the horizon plane
template <>
__device__ __forceinline__ float load_in<SRC_COUNTS>(const In& s, int n, int ch, int r, int col) {
  if (ch < 4) return count_at(s.x, s.x_i16, (((size_t)n * 4 + ch) * s.h + r) * s.w + col);
  if (ch == 4) return count_at(s.flow, s.flow_i16, ((size_t)n * s.h + r) * s.w + col);
  return s.horizon[n];
}

// ---- host side ---------------------------------------------------------------------------------------------------------

inline In counts_in(const void* hist, int hist_i16, const void* flow, int flow_i16, const float* horizon, int h, int w) {
  In s = {};
  s.x = (const float*)hist, s.x_i16 = hist_i16, s.flow = flow, s.flow_i16 = flow_i16, s.horizon = horizon;
  s.c_in = 6, s.h = h, s.w = w;
  return s;
}

}  // namespace
}  // namespace pv
