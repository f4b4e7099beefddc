// Shared pieces of the GATv2 attention kernels (wg_gatv2.hip, wg_gatv2_edge.hip): the shape limits, the sum over a head's lanes,
// the lanes-per-head dispatch, the argument blocks and what follows a row's walk in the forward kernel.  Both files walk a row the
// same way — one wave per row, lane = one float4 of the H C <= 256 wide row, edges in groups of four.
#pragma once
#include "wg_transformer_parts.hpp"

namespace wgamd {

constexpr int kGatv2MaxHC   = 256;    // one float4 of the row per lane
constexpr int kGatv2BwdRows = 16;     // destination rows per tile of the destination-major backward (4 per wave)

// the sum of v over the lanes of head hd; LPH = lanes per head when that is a power of two (butterflies inside the head's lanes:
// the idle lanes behind the row form groups of their own, H LPH being a multiple of LPH), 0 = any C / 4 (H masked wave sums)
template <int LPH>
__device__ __forceinline__ float head_sum(float v, int hd, int H)
{
  if constexpr (LPH > 0) {
#pragma unroll
    for (int o = LPH / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  } else {
    float mine = 0.f;
    for (int h = 0; h < H; ++h) {
      const float s = wave_sum(hd == h ? v : 0.f);
      if (hd == h) mine = s;
    }
    return mine;
  }
}

// launch(std::integral_constant<int, LPH>{}) for C channels per head
template <typename Launch>
void with_head_lanes(int C, Launch&& launch)
{
  switch (C / 4) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    case 16: launch(std::integral_constant<int, 16>{}); break;
    case 32: launch(std::integral_constant<int, 32>{}); break;
    case 64: launch(std::integral_constant<int, 64>{}); break;
    default: launch(std::integral_constant<int, 0>{}); break;
  }
}

struct gatv2_args {
  const int* row_ptr;
  const int* col;             // rows of xl
  int64_t n_rows;
  const float* xl;            // [n_src, ldxl]
  int64_t ldxl;
  const float* xr;            // XR[i] = xr[xr_rows ? xr_rows[i] : i]
  int64_t ldxr;
  const int64_t* xr_rows;
  const float* att;           // [H C]
  int H, C;
  float slope;
  const float* bias;          // [H C], or [C] with mean; nullable
  int relu, mean;
  float* out;                 // [n_rows, ldo]: H C wide, C with mean
  int64_t ldo;
  float* alpha;               // [E, H] or null
  float* agg;                 // [n_rows, H C] or null
};

struct gatv2_bwd_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* xl;
  int64_t ldxl;
  const float* xr;
  int64_t ldxr;
  const int64_t* xr_rows;
  const float* att;
  int H, C;
  float slope;
  const float* alpha;         // [E, H]
  const float* g;             // [n_rows, ldg] = dL/d agg
  int64_t ldg;
  const float* agg;           // [n_rows, H C]
  float* dxr;                 // [n_rows, H C]
  float* de;                  // [E, H]
  float* datt_part;           // [n_blocks, H C]
};

struct gatv2_src_args {
  const int* row_ptr_t;
  const int* col_t;           // destination row of every transposed entry
  const int* perm;            // its CSR edge
  int64_t n_src;
  const float* xl;
  int64_t ldxl;
  const float* xr;
  int64_t ldxr;
  const int64_t* xr_rows;
  const float* att;
  int H, C;
  float slope;
  const float* alpha;
  const float* de;
  const float* g;
  int64_t ldg;
  float* gx;                  // [n_src, ldgx]
  int64_t ldgx;
  int accumulate;
};

// What follows the walk of row i (edges [s, t)) in the forward kernels: acc / l / m = the lane's accumulator and its head's
// softmax sum and maximum.  Writes agg, the output row (bias, ReLU, the head mean of concat=False) and turns the row's logits in
// alpha into alpha.  Every lane of the wave takes part.
__device__ __forceinline__ void gatv2_row_finish(const gatv2_args& a, int64_t i, int lane, bool on, int H, int lph, int HC, int s,
                                                 int t, f32x4 acc, float l, float m)
{
  const float inv = l > 0.f ? 1.f / l : 0.f;      // (no edges: acc = 0 and inv = 0 — the aggregate is exactly zero)
  const f32x4 o = acc * inv;
  if (a.agg && on) reinterpret_cast<f32x4*>(a.agg + i * HC)[lane] = o;
  if (!a.mean) {
    if (on) {
      f32x4 y = o;
      if (a.bias) y += reinterpret_cast<const f32x4*>(a.bias)[lane];
      if (a.relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fmaxf(y[k], 0.f);
      }
      reinterpret_cast<f32x4*>(a.out + i * a.ldo)[lane] = y;
    }
  } else {
    // the head mean: lane q < C / 4 adds the H lanes that hold its columns, in head order (every lane takes part in the reads)
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    const int q = lane % lph;
    for (int h = 0; h < H; ++h) {
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] += __shfl(o[k], h * lph + q, 64);
    }
    if (lane < lph) {
      y *= 1.f / (float)H;
      if (a.bias) y += reinterpret_cast<const f32x4*>(a.bias)[lane];
      if (a.relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fmaxf(y[k], 0.f);
      }
      reinterpret_cast<f32x4*>(a.out + i * a.ldo)[lane] = y;
    }
  }
  if (a.alpha && s < t) {
    __threadfence_block();                        // the logits this wave wrote, read back by other lanes
    float* base = a.alpha + (int64_t)s * H;
    const int n = (t - s) * H;
    for (int b = 0; b < n; b += 64) {             // (a uniform trip count: every lane is a source of the two reads)
      const int idx = b + lane;
      const int src = (idx % H) * lph;            // the first lane of the entry's head
      const float mh = __shfl(m, src, 64), lh = __shfl(inv, src, 64);
      if (idx < n) base[idx] = expf(base[idx] - mh) * lh;
    }
  }
}

inline void gatv2_require_shape(int H, int C)
{
  if (!wgamd_gatv2_supported(H, C))
    throw logic_error(fmt("unsupported shape: H=%d (1 .. %d), C=%d (a multiple of 4), H C <= %d", H, kMaxH, C, kGatv2MaxHC));
}

}  // namespace wgamd
