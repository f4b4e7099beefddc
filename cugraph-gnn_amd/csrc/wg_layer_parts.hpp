// Shared pieces of the one-kernel layers over a sampled hop (wg_gcn.hip, wg_rgcn.hip, wg_transformer.hip, wg_sage_hetero.hip): an input row read
// through the layer's node list, the kind of that list, the launch for the kind found at run time, the 16-B row test, the
// dynamic-LDS launch of a layer kernel, and phase 2 of every layer kernel — the [16 x K16] LDS tile times wt^T on the exact
// fp32 matrix pipe (v_mfma_f32_16x16x4_f32), bias and ReLU fused.
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
