// The forecast-horizon stripe input of notebooks 09 and 10 (10_just_conv.ipynb:1398-1409, 09_horizon_represented_as_a_stripe
// .ipynb:1382-1395): history [n][n_hist][h][w] plus one plane that is 1 on columns start <= c < start + width and 0
// elsewhere.  The plane is synthesised while a kernel stages its input and never stored.  Shared by conv2d_wide_f32.hip
// (stride 1) and conv2d_wide_s2_f32.hip (stride 2): the source kind, its load, its descriptor and the argument check of the
// two first layers.  The tiles those files share are in conv_wide_f32.h.
#pragma once
#include "conv2d_f32_common.h"

namespace pv {
namespace {

constexpr int SRC_STRIPE = SRC_COUNTS + 1;   // history [n][n_hist][h][w] + the stripe channel
constexpr int kMaxHist = 7;

struct Stripe {
  const int32_t* start;    // [n] first column of the stripe (may lie outside the image)
  int width, n_hist;
};

// input channel ch (< c_in) of image n at (r, c) inside the image
template <int SRC>
__device__ __forceinline__ float load_in(const In& s, const Stripe& sp, int n, int ch, int r, int c) {
  if (SRC == SRC_STRIPE) {
    if (ch < sp.n_hist) return s.x[(((size_t)n * sp.n_hist + ch) * s.h + r) * s.w + c];
    const int st = sp.start[n];
    return (c >= st && c - st < sp.width) ? 1.0f : 0.0f;
  }
  return load_plain(s, n, ch, r, c);
}

inline In stripe_in(const float* history, int n_hist, int h, int w) {
  In s = {};
  s.x = history, s.c_in = n_hist + 1, s.h = h, s.w = w;
  return s;
}

// what a stripe first layer checks before its file's own extents check
inline int check_stripe_args(const char* who, int n_hist, int c_out, int stripe_width) {
  PV_REQUIRE(n_hist >= 1 && n_hist <= kMaxHist, PV_ESIZE, "%s: unsupported channel count: %d history frames (1..%d)", who,
             n_hist, kMaxHist);
  PV_REQUIRE(c_out == 64, PV_ESIZE, "%s: unsupported channel count c_out=%d (64)", who, c_out);
  PV_REQUIRE(stripe_width >= 0, PV_EINVAL, "%s: negative stripe width", who);
  return PV_OK;
}

}  // namespace
}  // namespace pv
