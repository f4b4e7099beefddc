// What the GIN-family layer kernels share (wg_gin.hip, wg_gine.hip): the argument block, the self row of a destination, the zero
// padding of an aggregate row in LDS tile A, and phases 2 and 3 — tile A times W1^T with b1 and ReLU -> LDS tile B (the hidden
// activation, and hidden_out), tile B times W2^T with b2 and the output ReLU -> global memory; with a null W2 phase 2 writes to
// global memory and the kernel ends (the one-product form).  tile_times_wt: wg_layer_parts.hpp.
#pragma once
#include "wg_layer_parts.hpp"

namespace wgamd {

constexpr int kGinUnroll = 8;   // edges of a row in flight

struct gin_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* x;
  int64_t ldx;
  int F;
  const void* src_ids;
  const int64_t* self_rows;   // nullable; input row of destination i itself, < 0 = none
  const float* x_dst;         // nullable; when set the self row of destination i is x_dst[i] (self_rows is not read)
  int64_t ldx_dst;
  const float* eps;           // nullable (0): ONE float on the device
  const float* w1;            // [H, ldw1] row-major
  int64_t ldw1;
  int H;
  const float* b1;
  int relu1;
  const float* w2;            // nullable: [N, ldw2] row-major
  int64_t ldw2;
  int N;
  const float* b2;
  int relu2;
  float* out;                 // [n_rows, N], or [n_rows, H] when w2 is null
  int64_t ldo;
  float* agg_out;             // nullable
  int64_t ld_agg;
  float* hidden_out;          // nullable
  int64_t ld_hidden;
  int F16, SD;                // tile A: F rounded up to 16, floats per row
  int H16, SH;                // tile B
  float* partials;            // STATS: [tiles of the layer][2][H], this launch's tiles from tile0 on
  int* counts;                // STATS: [tiles of the layer]
  int64_t tile0;
};

// the self row of destination i as float4 chunks, or null
template <int KIND>
__device__ __forceinline__ const f32x4* self_row(const gin_args& a, int64_t i)
{
  if (a.x_dst) return reinterpret_cast<const f32x4*>(a.x_dst + i * a.ldx_dst);
  if (a.self_rows == nullptr) return nullptr;
  const int64_t self = a.self_rows[i];
  return self >= 0 ? reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, self)) : nullptr;
}

// one float4 of an aggregate row into LDS tile A, zeros behind F up to F16 (lane c of a group of LG lanes, row r of the tile)
template <int LG>
__device__ __forceinline__ void store_agg_chunk(float* tile, const gin_args& a, int r, int c, f32x4 v)
{
  const int C4 = a.F / 4, C16 = a.F16 / 4;
  if (c < C16) reinterpret_cast<f32x4*>(tile + r * a.SD)[c] = c < C4 ? v : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int cc = c + LG; cc < C16; cc += LG) reinterpret_cast<f32x4*>(tile + r * a.SD)[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// phases 2 and 3 over the finished tile A (behind the barrier that ends phase 1)
__device__ __forceinline__ void gin_tile_products(const gin_args& a, float* tile, int64_t row0)
{
  const int tid = threadIdx.x;
  // ---- phase 2: [16 x F16] tile A @ W1^T ----
  if (a.w2 == nullptr) {
    tile_times_wt(tile, a.SD, a.F, a.F16, a.w1, a.ldw1, a.H, a.b1, a.relu1, a.out, a.ldo, row0, a.n_rows);
    return;
  }
  float* hid = tile + kTileRows * a.SD;     // tile B: all 16 rows are computed (rows past n_rows hold act1(b1): never written out)
  for (int idx = tid; idx < kTileRows * (a.H16 - a.H); idx += kThreads) {
    const int r = idx / (a.H16 - a.H), n = a.H + idx % (a.H16 - a.H);
    hid[r * a.SH + n] = 0.f;
  }
  tile_times_wt(tile, a.SD, a.F, a.F16, a.w1, a.ldw1, a.H, a.b1, a.relu1, hid, a.SH, 0, kTileRows);
  __syncthreads();
  if (a.hidden_out) {
    const int H4 = a.H / 4;                 // (H % 4 == 0 with a second product: W2's rows are read as float4)
    for (int idx = tid; idx < kTileRows * H4; idx += kThreads) {
      const int r = idx / H4, q = idx % H4;
      if (row0 + r < a.n_rows)
        reinterpret_cast<f32x4*>(a.hidden_out + (row0 + r) * a.ld_hidden)[q] = reinterpret_cast<const f32x4*>(hid + r * a.SH)[q];
    }
  }

  // ---- phase 3: [16 x H16] tile B @ W2^T ----
  tile_times_wt(hid, a.SH, a.H, a.H16, a.w2, a.ldw2, a.N, a.b2, a.relu2, a.out, a.ldo, row0, a.n_rows);
}

// what every launch of the family fills first
inline gin_args make_gin_args(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
                              const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps)
{
  gin_args a{};
  a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F, a.src_ids = src_ids;
  a.self_rows = self_rows, a.x_dst = x_dst, a.ldx_dst = ldx_dst, a.eps = eps;
  return a;
}

// the lane group of a row F floats wide: launch(std::integral_constant<int, LG>{}) with LG >= F / 4 of 4, 8, 16, 32, 64
template <typename Launch>
void with_lane_group(int F, Launch&& launch)
{
  const int c4 = F / 4;
  if (c4 <= 4) launch(std::integral_constant<int, 4>{});
  else if (c4 <= 8) launch(std::integral_constant<int, 8>{});
  else if (c4 <= 16) launch(std::integral_constant<int, 16>{});
  else if (c4 <= 32) launch(std::integral_constant<int, 32>{});
  else launch(std::integral_constant<int, 64>{});
}

}  // namespace wgamd
