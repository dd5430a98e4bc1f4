// What the stride-2 members of the VGPR-weight tile family share on top of conv2d_tile_f32.h: conv2d_s2_f32.hip (notebooks
// 14 / 15, 2-D), conv3d_s2_f32.hip (notebook 08, the depth-2 Conv3d and the horizon ConvTranspose2d) and conv2d_frames_f32.hip
// (notebook 07, the per-frame first layer and the 128 -> 32 ConvTranspose2d).  Stated once here: the weight gradient's tile
// plan, the ConvTranspose2d bias gradient (plane sums in slabs), the gather form's tile planner, both forms' Fwd, and the
// parity-class scatter in K passes with its tile planner.
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

// A (strided gather): at most 64 output columns per band (input tile up to 129 wide), bands of equal width; rows: the staged
// (2 tr + 1) x (2 tc + 1) tile within 64 KB, about 512 positions, bands of equal height.  w_out <= 63 leaves at least one row
// at 32 channels.
inline void gather_tiles(Fwd& a, int cinp) {
  a.n_cb = (a.w_out + 63) / 64;
  a.tc = (a.w_out + a.n_cb - 1) / a.n_cb;
  const int fit = (kLdsFloats / (cinp * (2 * a.tc + 1)) - 1) / 2;
  a.tr = std::max(1, std::min(std::min(a.h_out, fit), (512 + a.tc - 1) / a.tc));
  a.n_rb = (a.h_out + a.tr - 1) / a.tr;
  a.tr = (a.h_out + a.n_rb - 1) / a.n_rb;
}

template <int CINP, int MT, int SRC>
int run_gather(const char* who, Fwd a, int n, hipStream_t st) {
  gather_tiles(a, CINP);
  return launch_fwd<CINP, MT, SRC, false, 2>(who, a, n, st);
}

// the gather form's Fwd: out [m_out] over the conv_out grid of a [c] x h_src x w_src source, weights stored [m_out][c][3][3]
inline Fwd gather_args(const float* w, const float* bias, float* y, int c, int m_out, int h_src, int w_src, int relu) {
  Fwd a = conv_fwd_args(w, bias, y, c, m_out, h_src, w_src, relu);
  a.h_out = conv_out(h_src), a.w_out = conv_out(w_src);
  return a;
}

// the scatter form's Fwd: out [m_out][h_out][w_out] from src; weights stored [c][m_out][3][3], taps as they stand
inline Fwd scatter_args(const float* w, const float* bias, float* y, int m_out, int h_out, int w_out, int relu) {
  Fwd a = {};
  a.w = w, a.bias = bias, a.y = y, a.m_out = m_out, a.h_out = h_out, a.w_out = w_out;
  a.w_sm = 9, a.w_sc = m_out * 9, a.flip = 0, a.relu = relu ? 1 : 0;
  return a;
}

// ---- B (parity-class scatter) in K passes: a wave keeps the accumulators of its (class, tile) slots across the passes.  Used
// by conv3d_s2_f32.hip (one pass per depth tap) and conv2d_frames_f32.hip (one pass per frame's channel group). ----
constexpr int kClassTiles = 2;   // 16-position tiles of one parity class per wave (128 class positions per block)

// one output element of image i = (b, z) of y [n][m_out][dst_d][h_out][w_out]: bias, ReLU, output gate (dst_d = 1: NCHW)
__device__ __forceinline__ void store_out_depth(const Fwd& a, int img, int dst_d, int m, int r, int c, float acc) {
  const int b = img / dst_d, z = img - b * dst_d;
  const size_t off = ((((size_t)b * a.m_out + m) * dst_d + z) * a.h_out + r) * a.w_out + c;
  float v = acc + (a.bias ? a.bias[m] : 0.0f);
  if (a.relu) v = v > 0.0f ? v : 0.0f;
  if (a.out_gate && !(a.out_gate[off] > 0.0f)) v = 0.0f;
  a.y[off] = v;
}

// One parity class (PR, PC) of the block: its 16-position tiles continue the numbering of the classes before it and are
// dealt to the waves in turn, as in conv2d_s2_f32.hip; a wave's tiles of the class are its slots 0 .. kClassTiles - 1.  STORE
// = false: one pass's products are added into the slots; STORE = true: the slots are written out.
template <int CP, int MT, int PR, int PC, bool STORE>
__device__ __forceinline__ void scatter_class3(const Fwd& a, const float* lds, const float (&wa)[MT][9][CP / 4], int img,
                                               int dst_d, int a0, int b0, int cs, int sw, int& first_tile,
                                               acc4 (&acc)[kClassTiles][MT]) {
  constexpr int KS = CP / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // class positions inside the block: 2 a + PR < h_out, 2 b + PC < w_out
  const int rows = max(0, min(a.tr, (a.h_out - PR + 1) / 2 - a0)), cols = max(0, min(a.tc, (a.w_out - PC + 1) / 2 - b0));
  const int npos = rows * cols, tiles = (npos + 15) / 16;
  const int start = (wave - first_tile) & 3;
  first_tile += tiles;
#pragma unroll
  for (int ti = 0; ti < kClassTiles; ++ti) {
    const int t = start + 4 * ti;
    if (t >= tiles) continue;
    const int p = t * 16 + (lane & 15);
    const bool valid = p < npos;
    const int pp = valid ? p : 0;
    const int la = pp / cols, lb = pp - la * cols;
    if constexpr (STORE) {
      if (!valid) continue;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt * 16 + (lane >> 4) * 4 + i;
          if (m < a.m_out) store_out_depth(a, img, dst_d, m, 2 * (a0 + la) + PR, 2 * (b0 + lb) + PC, acc[ti][mt][i]);
        }
    } else {
      const float* src = lds + (lane >> 4) * cs + (la + 1) * sw + lb + 1;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        if ((kh & 1) != PR) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          if ((kw & 1) != PC) continue;
          const float* st = src - (kh >> 1) * sw - (kw >> 1);   // source (a - kh / 2, b - kw / 2)
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const float bv = st[s * 4 * cs];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              acc[ti][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][kh * 3 + kw][s], bv, acc[ti][mt], 0, 0, 0);
          }
        }
      }
    }
  }
}

template <int CP, int MT, bool STORE>
__device__ __forceinline__ void scatter_classes3(const Fwd& a, const float* lds, const float (&wa)[MT][9][CP / 4], int img,
                                                 int dst_d, int a0, int b0, int cs, int sw,
                                                 acc4 (&acc)[4][kClassTiles][MT]) {
  int first_tile = 0;
  scatter_class3<CP, MT, 0, 0, STORE>(a, lds, wa, img, dst_d, a0, b0, cs, sw, first_tile, acc[0]);
  scatter_class3<CP, MT, 0, 1, STORE>(a, lds, wa, img, dst_d, a0, b0, cs, sw, first_tile, acc[1]);
  scatter_class3<CP, MT, 1, 0, STORE>(a, lds, wa, img, dst_d, a0, b0, cs, sw, first_tile, acc[2]);
  scatter_class3<CP, MT, 1, 1, STORE>(a, lds, wa, img, dst_d, a0, b0, cs, sw, first_tile, acc[3]);
}

// ... its tiles: at most 64 output columns = 32 class columns per band; rows: the staged (tr + 1) x (tc + 1) tile of cp
// channels within 64 KB and at most 64 kClassTiles class positions.  Returns the tile's LDS bytes.
inline int scatter_slot_tiles(const char* who, Fwd& a, int cp, size_t& lds) {
  const int ga = (a.h_out + 1) / 2, gb = (a.w_out + 1) / 2;   // class grid of the even rows / columns (the larger one)
  a.n_cb = (a.w_out + 63) / 64;
  a.tc = (gb + a.n_cb - 1) / a.n_cb;
  a.n_cb = (gb + a.tc - 1) / a.tc;
  const int fit = kLdsFloats / (cp * (a.tc + 1)) - 1;
  a.tr = std::max(1, std::min(std::min(ga, fit), 64 * kClassTiles / a.tc));
  a.n_rb = (ga + a.tr - 1) / a.tr;
  a.tr = (ga + a.n_rb - 1) / a.n_rb;
  lds = (size_t)cp * (a.tr + 1) * (a.tc + 1) * sizeof(float);
  PV_REQUIRE(lds <= kLdsFloats * sizeof(float) && a.tr * a.tc <= 64 * kClassTiles, PV_ESIZE,
             "%s: no tile of %d x %d within the LDS budget", who, a.tr, a.tc);
  return PV_OK;
}

}  // namespace
}  // namespace pv
