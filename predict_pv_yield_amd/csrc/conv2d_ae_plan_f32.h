// The stride-1 tile planners and launch helpers of the VGPR-weight tile family at planes up to 128 wide, on top of
// conv2d_tile_f32.h: conv2d_ae_f32.hip (notebooks/16_maxpool) and conv2d_inputs_f32.hip (notebooks/05_more_image_inputs)
// plan their forward-like tiles and their weight gradients' tiles and slabs here, so a layer of one file and a layer of the
// other with the same extents run the same tiles.
#pragma once
#include "conv2d_tile_f32.h"

namespace pv {
namespace {

// forward-like tiles: at most 64 columns, bands of equal width; rows: the staged halo tile within 64 KB, about 512
// positions, bands of equal height.  POOL: one row of whole windows, at most 20 windows (the pre-activations share the LDS).
inline void fwd_tiles(Fwd& a, int cinp, bool pool) {
  if (pool) {
    const int pw = a.w_out / 3;
    a.n_cb = (pw + 19) / 20;
    const int tw = (pw + a.n_cb - 1) / a.n_cb;
    a.tc = 3 * tw, a.n_cb = (pw + tw - 1) / tw;
    a.tr = 3, a.n_rb = a.h_out / 3;
    a.h_out = a.n_rb * 3, a.w_out = pw * 3;   // floor pooling: the last rows / columns are not computed
    return;
  }
  a.n_cb = (a.w_out + 63) / 64;
  a.tc = (a.w_out + a.n_cb - 1) / a.n_cb;
  const int fit = kLdsFloats / (cinp * (a.tc + 2)) - 2;
  a.tr = std::max(1, std::min(std::min(a.h_out, fit), (512 + a.tc - 1) / a.tc));
  a.n_rb = (a.h_out + a.tr - 1) / a.tr;
  a.tr = (a.h_out + a.n_rb - 1) / a.n_rb;
}

template <int CINP, int MT, int SRC, bool POOL>
int run_fwd(const char* who, Fwd a, int n, hipStream_t st) {
  fwd_tiles(a, CINP, POOL);
  return launch_fwd<CINP, MT, SRC, POOL>(who, a, n, st);
}

// (h_out, w_out) = the positions the sum runs over; rows = the D rows (c_out), c = the sliding operand's channels.  Among
// column splits of at most 64, the tile with the smallest halo overhead that fits 64 KB and 384 positions.
inline WgPlan wg_plan(int n, int c, int rows, int h_out, int w_out) {
  WgPlan p = {};
  p.h_out = h_out, p.w_out = w_out, p.cinp = (c + 3) & ~3, p.mt = (rows + 15) / 16;
  double best = 1e30;
  const int cb0 = (w_out + 63) / 64;
  for (int n_cb = cb0; n_cb <= cb0 + 3 && n_cb <= w_out; ++n_cb) {
    const int tc = (w_out + n_cb - 1) / n_cb;
    int tr = 0;
    while (tr < h_out && (tr + 1) * tc <= 384 && wg_lds_floats(p.cinp, p.mt, tr + 1, tc) <= (size_t)kLdsFloats) ++tr;
    if (tr == 0) continue;
    const int n_rb = (h_out + tr - 1) / tr;
    tr = (h_out + n_rb - 1) / n_rb;
    const double cost = (double)(tr + 2) * (tc + 2) / ((double)tr * tc);
    if (cost < best) best = cost, p.tr = tr, p.tc = tc, p.n_rb = n_rb, p.n_cb = (w_out + tc - 1) / tc;
  }
  if (p.tr == 0) p.tr = 1, p.tc = std::min(w_out, 16), p.n_rb = h_out, p.n_cb = (w_out + p.tc - 1) / p.tc;
  slab_split(p, n, c, rows);
  return p;
}

template <int XSRC, int GSRC>
int run_wgrad(const char* who, const In& in, const In& g, int pad, const WgPlan& p, float* dw, float* db, bool transposed,
              void* ws, size_t ws_bytes, hipStream_t st) {
  // column tiles ceil((9 c + 1) / 16) over 4 waves: 4 (c = 6), 10 (c = 16), 19 (c = 32)
  const int ntw = ((in.c_in * 9 + 1 + 15) / 16 + 3) / 4;
#define PV_WG(MT, NTW) \
  if (p.mt == MT && ntw == NTW) \
  return launch_wgrad<MT, NTW, XSRC, GSRC>(who, in, g, pad, p, dw, db, transposed, ws, ws_bytes, st)
  PV_WG(2, 5);
  PV_WG(2, 3);
  PV_WG(1, 5);
  PV_WG(1, 3);
  PV_WG(1, 1);
#undef PV_WG
  return fail(PV_ESIZE, "%s: no weight-gradient tile for %d rows x %d channels", who, g.c_in, in.c_in);
}

}  // namespace
}  // namespace pv
