// What the four exact-f32 Conv2d 3x3 files share: conv2d_f32.hip (experiments/002, 17 / 32 -> 32 / 4 channels),
// conv2d_pool_f32.hip (experiments/001, 144 channels with fused MaxPool2d(3)), conv2d_ae_f32.hip (notebooks/16_maxpool:
// Conv2d / ConvTranspose2d up to 128 wide) and conv2d_s2_f32.hip (notebooks 14 / 15: the same at stride 2).  This header holds the ordered slab sum of their weight gradients (also in the
// ConvTranspose2d layout), the MaxPool2d(3) + ReLU window rule and its backward, the descriptor of what a pass reads (In) with
// its plain and pooled-gradient loads, the five synthesised input channels of the two experiments and the argument checks
// they all repeat.  The 144-channel main loops (weights in LDS, K streamed in chunks) stay in their file; the files whose
// weights fit the VGPRs share theirs in conv2d_tile_f32.h.  The 64 / 128-channel families (conv2d_wide_f32.hip,
// conv2d_wide_s2_f32.hip, conv3d_wide_f32.hip) and their one-output-channel heads (conv2d_head_f32.hip) use the slab sum, In
// and the checks of this header too; their tiles are in conv_wide_f32.h.
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
// DEPTH2: one depth tap of a [c_out][c_in][2][3][3] weight (dw points at the tap's first element): j = ci * 9 + tap is
// stored as dw[co * 2 k9 + ci * 18 + tap] (instantiated by conv3d_s2_f32.hip alone).
constexpr int kSumElems = 32, kSumGroups = kBlock / kSumElems;
template <bool TRANSPOSED, bool DEPTH2 = false>
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
    else if (DEPTH2) dw[co * 2 * k9 + (j / 9) * 18 + j % 9] = t;
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

// MaxPool2d(3) fused with ReLU, one rule for every site.  pool3_relu: at(k) = the pre-activation at window position k =
// 0..8 (row-major); the first maximum wins and NaN propagates (torch CPU); returns relu(max) and the code byte kept per
// pooled output: the winning position, or kDead where the maximum is <= 0 (the window passes no gradient).
constexpr uint8_t kDead = 255;

template <class At>
__device__ __forceinline__ float pool3_relu(At at, uint8_t& code) {
  float best = -__builtin_inff();
  int k_best = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float v = at(k);
    if (v > best || __builtin_isnan(v)) best = v, k_best = k;
  }
  const bool live = best > 0.0f || __builtin_isnan(best);
  code = live ? (uint8_t)k_best : kDead;
  return live ? best : 0.0f;
}

// ... and its backward: element (r, c) of the pre-pool gradient of one plane from the plane's pooled gradient dyp[ph][pw]
// and codes: the pooled gradient where the window's code names (r % 3, c % 3), else (and beyond the whole windows) 0.
__device__ __forceinline__ float pool3_expand(const float* dyp, const uint8_t* codes, int ph, int pw, int r, int c) {
  const int pr = r / 3, pc = c / 3;
  if (pr >= ph || pc >= pw) return 0.0f;
  const int off = pr * pw + pc;
  return (int)codes[off] == (r - pr * 3) * 3 + (c - pc * 3) ? dyp[off] : 0.0f;
}

// What a pass reads, by source kind.  Each file's first layer synthesises its input while staging (its own load_in /
// stage_in arm); the other two kinds are the same everywhere.
enum Src { SRC_PLAIN, SRC_POOLED, SRC_SAT, SRC_COUNTS, SRC_DEPTH, SRC_HORIZON, SRC_FRAME_HORIZON, SRC_CH_GROUP, SRC_FRAME_SHARED,
           SRC_INPUTS4 };

struct In {
  // SRC_PLAIN: x[n][c_in][h][w], zeroed where gate <= 0 (gate may be null)
  // SRC_POOLED: the pre-pool gradient of a pooled layer, [n][c_in][h][w] = pool3_expand of x = dyp[n][c_in][ph][pw]
  // SRC_SAT: satellite frames behind x plus centre marker, geo x, geo y, pixel x, pixel y: experiments/001 reads sat[b]
  //          [t_total][h][w] frames 0..n_frames-1, experiments/002 sat[n][h][w][12] with n / t_per_ex the coords' example
  // SRC_COUNTS: x = history [n][4][h][w], flow [n][h][w] (int16 where *_i16, else f32 counts), horizon [n]: 6 channels
  // SRC_DEPTH: x[b][c_in][t_total][h][w] read one depth slice at a time: the pass's image index is (b, z) = (i / n_frames,
  //            i % n_frames) and channel ch is the plane (ch, z + t_per_ex); zeroed where gate <= 0 (gate may be null)
  // SRC_HORIZON: x[n][c_in - 1][h][w], then horizon[n] as a constant last channel
  // SRC_FRAME_HORIZON: x = history [b][n_frames][h][w]: the pass's image i = n_frames b + f is plane i of x (channel 0), then
  //                    horizon[i / n_frames] as a constant second channel (c_in = 2)
  // SRC_CH_GROUP: the c_in channels [t_per_ex, t_per_ex + c_in) of x[n][t_total][h][w]; zeroed where gate <= 0 (may be null)
  // SRC_FRAME_SHARED: x[b][c_in][h][w] read by the n_frames images i = n_frames b + f of an example alike; gate as SRC_PLAIN
  // SRC_INPUTS4: four channels from three tensors read in place (c_in = 4): channel 0 = x, the flow prediction [n][h][w];
  //              channel 1 = xc, the t0 image [n][h][w]; channels 2, 3 = flow, the f32 flow field [n][2][h][w] (x then y)
  const float* x;
  const float* gate;
  const uint8_t* codes;    // SRC_POOLED: [n][c_in][ph][pw]
  const float* xc;         // SRC_SAT: [b][w] geo x (varies along the last axis); SRC_INPUTS4: the t0 image [n][h][w]
  const float* yc;         // SRC_SAT: [b][h] geo y (varies along rows)
  const void* flow;
  const float* horizon;
  int c_in, h, w, ph, pw, t_total, n_frames, t_per_ex, x_i16, flow_i16;
};

__device__ __forceinline__ float load_plain(const In& s, int n, int ch, int r, int c) {
  const size_t off = (((size_t)n * s.c_in + ch) * s.h + r) * s.w + c;
  const float v = s.x[off];
  return (s.gate && !(s.gate[off] > 0.0f)) ? 0.0f : v;
}

__device__ __forceinline__ float load_pooled(const In& s, int n, int ch, int r, int c) {
  const size_t plane = ((size_t)n * s.c_in + ch) * s.ph * s.pw;
  return pool3_expand(s.x + plane, s.codes + plane, s.ph, s.pw, r, c);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

inline In plain_in(const float* x, const float* gate, int c, int h, int w) {
  In s = {};
  s.x = x, s.gate = gate, s.c_in = c, s.h = h, s.w = w;
  return s;
}

inline In pooled_in(const float* dyp, const uint8_t* codes, int c, int h, int w) {
  In s = {};
  s.x = dyp, s.codes = codes, s.c_in = c, s.h = h, s.w = w, s.ph = h / 3, s.pw = w / 3;
  return s;
}

// the same NCHW conv as a 1x3x3 Conv3d with T = 1, for the launches that take pv_conv3d_general_*_f32
inline pv_conv3d_geom conv3d_geom_1x3x3(int n, int c_in, int c_out, int h_in, int w_in) {
  pv_conv3d_geom g = {};
  g.batch = n, g.c_in = c_in, g.c_out = c_out, g.t_in = 1, g.h_in = h_in, g.w_in = w_in;
  g.k_t = 1, g.k_h = 3, g.k_w = 3, g.stride_t = 1, g.stride_h = 1, g.stride_w = 1;
  return g;
}

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
