// Shared pieces of the one-kernel layers over a sampled hop (wg_gcn.hip, wg_rgcn.hip, wg_transformer.hip, wg_sage_hetero.hip,
// wg_transformer_hetero.hip, wg_gin.hip): an input row read through the layer's node list, the kind of that list, the launch for
// the kind found at run time, the 16-B row test, the dynamic-LDS launch of a layer kernel, the zeroing of the tile's k padding
// and the copy of a finished tile to kept rows, the frame of a heterogeneous launch (row_of, hetero_frame and its host check,
// the relations' row_ptr windows), and phase 2 of every layer kernel — the [16 x K16] LDS tile times wt^T on the exact fp32
// matrix pipe (v_mfma_f32_16x16x4_f32), bias and ReLU fused.
#pragma once
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "wg_common.hpp"
#include "wgamd_ext.h"

namespace wgamd {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kTileRows = 16;   // destination rows per workgroup of a layer kernel: one 16-row MFMA tile
constexpr int kThreads  = 256;  // 4 waves

// id kinds: 0 = x is indexed by the row itself, 1 = int32 node list, 2 = int64 node list, 3 = int64 BYTE offsets from x
template <int KIND>
__device__ __forceinline__ const float* x_row(const float* x, int64_t ldx, const void* ids, int64_t r)
{
  if constexpr (KIND == 0) return x + r * ldx;
  else if constexpr (KIND == 1) return x + (int64_t) static_cast<const int32_t*>(ids)[r] * ldx;
  else if constexpr (KIND == 2) return x + static_cast<const int64_t*>(ids)[r] * ldx;
  else return reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + static_cast<const int64_t*>(ids)[r]);
}

inline int ids_kind(const void* src_ids, wholememory_dtype_t dt)
{
  if (src_ids == nullptr) return 0;
  if (dt == WHOLEMEMORY_DT_INT) return 1;
  if (dt == WHOLEMEMORY_DT_INT64) return 2;
  if (dt == WGAMD_IDS_BYTE_OFFSETS) return 3;
  throw invalid_input("src_ids must be INT, INT64 or WGAMD_IDS_BYTE_OFFSETS");
}

// launch(std::integral_constant<int, KIND>{}) for the kind of ids_kind
template <typename Launch>
void with_kind(int kind, Launch&& launch)
{
  switch (kind) {
    case 0: launch(std::integral_constant<int, 0>{}); break;
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    default: launch(std::integral_constant<int, 3>{}); break;
  }
}

// rows of ld floats from p can be read as float4: p 16-B aligned, ld a multiple of 4 (ld = 0: rows at byte offsets, p alone)
inline bool aligned_rows(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

// A layer kernel over a.n_rows destination rows: one workgroup per 16-row tile, a.SD floats of dynamic LDS per tile row
// (16 x (1024 + 4) floats = 65.8 KB at the largest K: above the 64 KB default)
template <typename Args>
void launch_tiles(void (*kern)(Args), const Args& a, hipStream_t st)
{
  const dim3 grid((unsigned)((a.n_rows + kTileRows - 1) / kTileRows));
  const size_t lds = (size_t)kTileRows * a.SD * 4;
  WG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, kThreads, lds, st>>>(a);
}

// the tile's k padding [K, K16) is zero (all threads of the workgroup)
__device__ __forceinline__ void zero_tile_padding(float* tile, int SD, int K, int K16)
{
  const int pad4 = (K16 - K) / 4;
  for (int p = threadIdx.x; p < kTileRows * pad4; p += kThreads)
    reinterpret_cast<f32x4*>(tile + (p / pad4) * SD + K)[p % pad4] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// rows_here x K of the finished tile to kept[row0 + r, :], rows ld apart: the operand of the product, for the backward
__device__ __forceinline__ void keep_tile_rows(const float* tile, int SD, int K, int rows_here, float* kept, int64_t ld, int64_t row0)
{
  const int K4 = K / 4;
  for (int p = threadIdx.x; p < rows_here * K4; p += kThreads)
    reinterpret_cast<f32x4*>(kept + (row0 + p / K4) * ld)[p % K4] = reinterpret_cast<const f32x4*>(tile + (p / K4) * SD)[p % K4];
}

// (mean, M2 = sum of squared distances from that mean) of `rows` values `stride` floats apart, two passes (never E[v^2] -
// mean^2): one column of a row tile, in LDS or in global memory — a batch-norm partial (wg_gin.hip, wg_batch_norm.hip)
__device__ __forceinline__ void column_mean_m2(const float* p, int64_t stride, int rows, float& mean, float& m2)
{
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += p[r * stride];
  mean = rows > 0 ? s / (float)rows : 0.f;
  m2 = 0.f;
  for (int r = 0; r < rows; ++r) {
    const float d = p[r * stride] - mean;
    m2 = __builtin_fmaf(d, d, m2);
  }
}

// ---- the frame of a heterogeneous layer launch (wg_sage_hetero.hip, wg_transformer_hetero.hip): n_rel relations' blocks side by
// side in the tile, then the root block; one stacked weight; the running sum of an earlier launch and the row placement ----

// a row read through a node list whose kind is known at run time only (0 = by row, 1 = int32, 2 = int64)
__device__ __forceinline__ const float* row_of(const float* x, int64_t ldx, const void* ids, int kind, int64_t r)
{
  if (kind == 1) r = static_cast<const int32_t*>(ids)[r];
  else if (kind == 2) r = static_cast<const int64_t*>(ids)[r];
  return x + r * ldx;
}

// what the two kernels' argument blocks share; each derives from it and adds its rel[] array
struct hetero_frame {
  int n_rel;
  int64_t n_rows;
  const float* x_dst;         // the root block: null = none
  int64_t ldx_dst;
  int F_dst;
  const int64_t* dst_rows;    // row of destination i in x_dst's numbering (null: i)
  const void* dst_ids;
  int dst_kind;
  int root_col0;
  const float* wt;
  int64_t ldw;
  int N;
  const float* bias;
  int relu;
  const float* acc_in;
  int64_t ld_acc;
  const int64_t* out_rows;
  float* out;
  int64_t ldo;
  float* kept;                // _train: the tile's rows (C of the SAGE layer, A of the transformer layer)
  int64_t ld_kept;
  int K, K16, SD;
};

// Fills the frame of a launch whose relation blocks are k_rel floats wide together, checking the root block, the leading
// dimensions and the kept rows; kept_error is what a bad kept-rows buffer throws.
inline void fill_hetero_frame(hetero_frame& a, int n_rel, int64_t n_rows, int k_rel, const float* x_dst, int64_t ldx_dst, int F_dst,
                              const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind, const float* wt, int64_t ldw, int N,
                              const float* bias, bool relu, const float* acc_in, int64_t ld_acc, const int64_t* out_rows, float* out,
                              int64_t ldo, float* kept, int64_t ld_kept, const char* kept_error)
{
  int at = k_rel;
  a.n_rel = n_rel, a.n_rows = n_rows;
  if (x_dst) {
    WG_REQUIRE_INPUT(F_dst > 0 && ldx_dst >= F_dst, "leading dimension too small");
    WG_REQUIRE_INPUT(dst_ids_kind >= 0 && dst_ids_kind <= 2 && (dst_ids_kind == 0) == (dst_ids == nullptr), "bad node list kind");
    if (!aligned_rows(x_dst, ldx_dst)) throw logic_error("x_dst rows must be 16-B aligned");
    a.x_dst = x_dst, a.ldx_dst = ldx_dst, a.F_dst = F_dst, a.dst_rows = dst_rows, a.dst_ids = dst_ids, a.dst_kind = dst_ids_kind;
    a.root_col0 = at;
    at += F_dst;
  }
  a.wt = wt, a.ldw = ldw, a.N = N, a.bias = bias, a.relu = relu ? 1 : 0;
  a.acc_in = acc_in, a.ld_acc = ld_acc, a.out_rows = out_rows, a.out = out, a.ldo = ldo, a.kept = kept, a.ld_kept = ld_kept;
  a.K   = at;
  a.K16 = (a.K + 15) / 16 * 16;
  a.SD  = a.K16 + 4;      // rows 4 banks apart: the 16 rows of a fragment read spread over the 64 banks
  WG_REQUIRE_INPUT(ldw >= a.K && ldo >= N && (acc_in == nullptr || ld_acc >= N), "leading dimension too small");
  if (!aligned_rows(wt, ldw)) throw logic_error("wt rows must be 16-B aligned");
  if (kept != nullptr && (ld_kept < a.K || !aligned_rows(kept, ld_kept))) throw logic_error(kept_error);
}

// every relation's row_ptr window of the tile into LDS: rp[r][t] = row_ptr_r[row0 + min(t, rows_here)]
template <typename Rel, int NR>
__device__ __forceinline__ void load_row_windows(int (&rp)[NR][kTileRows + 1], const Rel* rel, int n_rel, int64_t row0, int rows_here)
{
  const int tid = threadIdx.x;
  if (tid < n_rel * (kTileRows + 1)) {
    const int r = tid / (kTileRows + 1), t = tid % (kTileRows + 1);
    rp[r][t] = rel[r].row_ptr[row0 + std::min(t, rows_here)];
  }
}

// Phase 2: out[row0 + r, n] = act(sum_k tile[r, k] wt[n, k] + bias[n]) for r < 16 (rows below n_rows), n < N, k < K16.  The
// tile's columns [K, K16) are zero and wt is read for k < K only.  Wave w owns the 16-column tiles w, w + 4, w + 8, w + 12; a
// lane reads one float4 of the tile (ds_read_b128) and one float4 of a wt row per 16 k — the four k of a float4 are four MFMA
// k-steps.  Rows SD floats apart in the tile.  acc_in (nullable, rows ld_acc apart): a running sum added before the activation;
// out_rows (nullable): row i is written to out[out_rows[i]].
__device__ __forceinline__ void tile_times_wt(const float* tile, int SD, int K, int K16, const float* wt, int64_t ldw, int N,
                                              const float* bias, int relu, float* out, int64_t ldo, int64_t row0, int64_t n_rows,
                                              const float* acc_in = nullptr, int64_t ld_acc = 0, const int64_t* out_rows = nullptr)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_ct = (N + 15) / 16;
  if (wave >= n_ct) return;
  const int m = lane & 15, g = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < K16; kb += 16) {
    const int k = kb + 4 * g;
    const f32x4 av = *reinterpret_cast<const f32x4*>(tile + m * SD + k);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ct = wave + 4 * q;
      if (ct < n_ct) {
        const int n = ct * 16 + m;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (n < N && k < K) bv = *reinterpret_cast<const f32x4*>(wt + (int64_t)n * ldw + k);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], bv[kk], acc[q], 0, 0, 0);
      }
    }
  }
  // C/D map of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = (wave + 4 * q) * 16 + m;
    if (wave + 4 * q >= n_ct || n >= N) continue;
    const float b = bias ? bias[n] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t i = row0 + 4 * g + reg;
      if (i < n_rows) {
        float y = acc[q][reg] + b;
        if (acc_in) y += acc_in[i * ld_acc + n];
        if (relu) y = fmaxf(y, 0.f);
        out[(out_rows ? out_rows[i] : i) * ldo + n] = y;
      }
    }
  }
}

}  // namespace wgamd
