// The forecast horizon as a constant last input channel of a ConvTranspose2d (SRC_HORIZON), stated once for conv3d_s2_f32.hip
// (notebook 08: ConvTranspose2d 33 -> 32 at stride 2) and conv2d_inputs_f32.hip (notebook 05: the same layer at stride 1).
// The channel is synthesised while a tile is staged: horizon[n] inside the source extent, 0 in the halo (stage_in's bounds).
#pragma once
#include "conv2d_tile_f32.h"

namespace pv {
namespace {

// the real channels, then the horizon plane
template <>
__device__ __forceinline__ float load_in<SRC_HORIZON>(const In& s, int n, int ch, int r, int col) {
  if (ch == s.c_in - 1) return s.horizon[n];
  return s.x[(((size_t)n * (s.c_in - 1) + ch) * s.h + r) * s.w + col];
}

// ---- host side ---------------------------------------------------------------------------------------------------------

inline In horizon_in(const float* x, const float* horizon, int c_real, int h, int w) {
  In s = {};
  s.x = x, s.horizon = horizon, s.c_in = c_real + 1, s.h = h, s.w = w;
  return s;
}

}  // namespace
}  // namespace pv
