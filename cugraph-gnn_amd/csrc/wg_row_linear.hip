// RowLinear: a Linear over gathered rows with a row-wise epilogue, in ONE launch:
//     y   = X[rows] @ W^T + b                      X: a float32 / float16 / bfloat16 table read by row or through an id list
//     y   = relu(y)                                (relu)
//     z   = LayerNorm(y; gamma, beta, eps)         (norm 1: torch.nn.functional.layer_norm, biased variance)
//         = y / max(||y||_2, eps)                  (norm 2: torch.nn.functional.normalize(p=2, dim=-1))
//     out = z + add                                (add nullable)
// the input projection (`paper_norm(paper_lin(x))` over a 16-bit feature table), the skip term `lin1(x[rows])`, the tail
// (`normalize(lin2(x).relu()) + x_paper`) and the plain heads of the reference's models.
//
// Pieces:
//   * row_linear_kernel — the layer kernels' frame: one workgroup per 16-row tile, 4 waves, dynamic LDS.  Phase 1: the tile's
//     input rows -> LDS tile A, 16 B per lane of a float32 table, 8 B per lane of a 16-bit one converted exactly where it is
//     written to LDS (wg_x16.hpp); k padding zeroed; kept_x gets the rows (the operand of the weight gradient).  Phase 2:
//     tile_times_wt (wg_layer_parts.hpp) with the bias and ReLU — straight to global memory when nothing follows, else into LDS
//     tile B (as gin_layer_kernel's hidden tile).  Phase 3: 16 lanes per row hold the row of tile B in registers (up to four
//     float4 per lane): kept_y, a two-pass mean and variance (or the sum of squares), the affine, add, a float4 store.
//   * row_linear_bwd_kernel — dy from kept_y (post-ReLU, pre-norm) and grad_out: the statistics are recomputed in registers,
//     the norm's backward, then the ReLU mask.  With LayerNorm's affine gradients wanted every workgroup adds (g x^, g) over its
//     rows in registers, then over its 16 row groups through LDS in group order -> partials[workgroup][2][N].
//   * row_linear_affine_kernel adds the partial rows in workgroup order.  No atomics anywhere: the same bits on every run.
#include "wg_layer_parts.hpp"
#include "wg_x16.hpp"

namespace wgamd {
namespace {

constexpr int kRowLanes  = 16;     // lanes per row in phase 3 and in the backward: 16 rows per 256-thread pass
constexpr int kRowVecs   = 4;      // float4 per lane at most: N <= 256
constexpr int kBwdBlocks = 1024;   // workgroups of the backward at most: the partial rows the affine launch adds up
constexpr int kAgCols = 64, kAgLanes = 16;

struct rl_args {
  const void* x;              // [*, ldx] elements of XT
  int64_t ldx;
  const void* ids;            // nullable: row i of the problem is x[ids[i]]
  int64_t n_rows;
  int K;
  const float* wt;            // [N, ldw]
  int64_t ldw;
  int N;
  const float* bias;
  int relu, norm;             // norm: 0 none, 1 LayerNorm, 2 L2
  const float* gamma;
  const float* beta;
  float eps;
  const float* add;
  int64_t ld_add;
  float* out;
  int64_t ldo;
  float* kept_x;
  int64_t ld_kx;
  float* kept_y;
  int64_t ld_ky;
  int K16, SD;                // tile A: K rounded up to 16, floats per row
  int N16, SN;                // tile B
  int use_b;
};

struct rlb_args {
  const float* y;
  int64_t ldy;
  const float* g;
  int64_t ldg;
  int64_t n_rows;
  int N;
  int relu, norm;
  const float* gamma;
  float eps;
  float* dy;
  int64_t ld_dy;
  float* part;                // nullable: [blocks][2][N]
  int blocks;
};

template <int KIND>
__device__ __forceinline__ int64_t listed_row(const void* ids, int64_t r)
{
  if constexpr (KIND == 0) return r;
  else if constexpr (KIND == 1) return static_cast<const int32_t*>(ids)[r];
  else return static_cast<const int64_t*>(ids)[r];
}

__device__ __forceinline__ float lanes16_sum(float v)
{
#pragma unroll
  for (int m = kRowLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// a [N] vector's float4s of lane c (fill where the vector is absent or past its end)
template <int NV>
__device__ __forceinline__ void load_cols(const float* p, int c, int N4, float fill, f32x4 (&v)[NV])
{
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    v[k] = f32x4{fill, fill, fill, fill};
    if (p && c + k * kRowLanes < N4) v[k] = reinterpret_cast<const f32x4*>(p)[c + k * kRowLanes];
  }
}

template <int KIND, typename XT>
__global__ void __launch_bounds__(kThreads) row_linear_kernel(rl_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  using E = x16::row_elems<XT>;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);

  // ---- phase 1: the tile's input rows -> LDS tile A (rows past n_rows: zeros) ----
  const int K4 = a.K / 4;
  for (int p = tid; p < kTileRows * K4; p += kThreads) {
    const int r = p / K4, c = p % K4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows_here) {
      const XT* row = static_cast<const XT*>(a.x) + listed_row<KIND>(a.ids, row0 + r) * a.ldx;
      v = E::f32(reinterpret_cast<const typename E::raw_t*>(row)[c]);
    }
    reinterpret_cast<f32x4*>(tile + r * a.SD)[c] = v;
  }
  zero_tile_padding(tile, a.SD, a.K, a.K16);
  __syncthreads();
  if (a.kept_x) keep_tile_rows(tile, a.SD, a.K, rows_here, a.kept_x, a.ld_kx, row0);

  // ---- phase 2: [16 x K16] tile A @ W^T, bias, ReLU ----
  if (!a.use_b) {
    tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldw, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows);
    return;
  }
  float* hid = tile + kTileRows * a.SD;     // tile B: all 16 rows are computed (rows past n_rows hold act(bias): never written out)
  // (phase 3 reads columns below N only: tile B's padding columns [N, N16) need no zeroing, unlike a tile that is multiplied)
  tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldw, a.N, a.bias, a.relu, hid, a.SN, 0, kTileRows);
  __syncthreads();

  // ---- phase 3: the row-wise epilogue, 16 lanes per row ----
  const int r = tid / kRowLanes, c = tid % kRowLanes, N4 = a.N / 4;
  const int64_t i = row0 + r;
  const bool ok = r < rows_here;
  const float fn = (float)a.N;
  f32x4 v[kRowVecs];
#pragma unroll
  for (int k = 0; k < kRowVecs; ++k) {
    const int c4 = c + k * kRowLanes;
    v[k] = c4 < N4 ? reinterpret_cast<const f32x4*>(hid + r * a.SN)[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.kept_y && ok && c4 < N4) reinterpret_cast<f32x4*>(a.kept_y + i * a.ld_ky)[c4] = v[k];
  }
  if (a.norm == 1) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kRowVecs; ++k) s += sum4(v[k]);
    const float mean = lanes16_sum(s) / fn;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < kRowVecs; ++k) {
      v[k] = c + k * kRowLanes < N4 ? v[k] - mean : f32x4{0.f, 0.f, 0.f, 0.f};
      sq += sum4(v[k] * v[k]);
    }
    const float rstd = 1.f / sqrtf(lanes16_sum(sq) / fn + a.eps);
    f32x4 w[kRowVecs], b[kRowVecs];
    load_cols<kRowVecs>(a.gamma, c, N4, 1.f, w);
    load_cols<kRowVecs>(a.beta, c, N4, 0.f, b);
#pragma unroll
    for (int k = 0; k < kRowVecs; ++k) {
      v[k] *= rstd;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = __builtin_fmaf(v[k][e], w[k][e], b[k][e]);
    }
  } else if (a.norm == 2) {
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < kRowVecs; ++k) sq += sum4(v[k] * v[k]);
    const float d = fmaxf(sqrtf(lanes16_sum(sq)), a.eps);
#pragma unroll
    for (int k = 0; k < kRowVecs; ++k) v[k] = v[k] / d;
  }
  if (!ok) return;
#pragma unroll
  for (int k = 0; k < kRowVecs; ++k) {
    const int c4 = c + k * kRowLanes;
    if (c4 >= N4) continue;
    if (a.add) v[k] += reinterpret_cast<const f32x4*>(a.add + i * a.ld_add)[c4];
    reinterpret_cast<f32x4*>(a.out + i * a.ldo)[c4] = v[k];
  }
}

// NV: float4 per lane (1 up to N = 64, 2 up to 128, 4 up to 256)
template <int NV>
__global__ void __launch_bounds__(kThreads) row_linear_bwd_kernel(rlb_args a)
{
  extern __shared__ __attribute__((aligned(16))) float sums[];
  const int grp = threadIdx.x / kRowLanes, c = threadIdx.x % kRowLanes, N4 = a.N / 4;
  const int64_t tiles = (a.n_rows + kTileRows - 1) / kTileRows;
  const float fn = (float)a.N;
  const bool affine = a.norm == 1 && a.part != nullptr;
  f32x4 w[NV], dw[NV], db[NV];
  load_cols<NV>(a.norm == 1 ? a.gamma : nullptr, c, N4, 1.f, w);
#pragma unroll
  for (int k = 0; k < NV; ++k) dw[k] = db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t t = blockIdx.x; t < tiles; t += a.blocks) {
    const int64_t i = t * kTileRows + grp;
    const bool ok = i < a.n_rows;
    f32x4 y[NV], g[NV];
    bool pos[NV][4];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c4 = c + k * kRowLanes;
      y[k] = g[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok && c4 < N4) {
        if (a.relu || a.norm) y[k] = reinterpret_cast<const f32x4*>(a.y + i * a.ldy)[c4];
        g[k] = reinterpret_cast<const f32x4*>(a.g + i * a.ldg)[c4];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) pos[k][e] = !a.relu || y[k][e] > 0.f;
    }
    if (a.norm == 1) {
      // dy = rstd (w g - mean_c(w g) - x^ mean_c(w g x^))      (y holds x^ from here; g = 0 past the row's end)
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) s += sum4(y[k]);
      const float mean = lanes16_sum(s) / fn;
      float sq = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        y[k] = c + k * kRowLanes < N4 ? y[k] - mean : f32x4{0.f, 0.f, 0.f, 0.f};
        sq += sum4(y[k] * y[k]);
      }
      const float var = lanes16_sum(sq) / fn;
      const float rstd = ok ? 1.f / sqrtf(var + a.eps) : 0.f;      // (rows past the end add zeros to the sums, also with eps = 0)
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        y[k] *= rstd;
        dw[k] += g[k] * y[k], db[k] += g[k];
        g[k] *= w[k];
        s1 += sum4(g[k]), s2 += sum4(g[k] * y[k]);
      }
      const float m1 = lanes16_sum(s1) / fn, m2 = lanes16_sum(s2) / fn;
#pragma unroll
      for (int k = 0; k < NV; ++k) g[k] = (g[k] - m1 - y[k] * m2) * rstd;
    } else if (a.norm == 2) {
      // z = y / d, d = max(||y||, eps):  dy = g / d - y (g . y) / ||y||^3 where ||y|| >= eps, g / eps below it
      float sq = 0.f, gy = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) sq += sum4(y[k] * y[k]), gy += sum4(g[k] * y[k]);
      sq = lanes16_sum(sq), gy = lanes16_sum(gy);
      const float nrm = sqrtf(sq);
      if (nrm >= a.eps) {
        const float coef = gy / sq;
#pragma unroll
        for (int k = 0; k < NV; ++k) g[k] = (g[k] - y[k] * coef) / nrm;
      } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) g[k] = g[k] / a.eps;
      }
    }
    if (!ok) continue;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c4 = c + k * kRowLanes;
      if (c4 >= N4) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!pos[k][e]) g[k][e] = 0.f;
      reinterpret_cast<f32x4*>(a.dy + i * a.ld_dy)[c4] = g[k];
    }
  }
  if (!affine) return;
  // the row groups' sums through LDS, added in group order: partials[workgroup][0][:] = sum g x^, [1][:] = sum g
  const int N2 = 2 * a.N;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (c + k * kRowLanes < N4) {
      reinterpret_cast<f32x4*>(sums + grp * N2)[c + k * kRowLanes] = dw[k];
      reinterpret_cast<f32x4*>(sums + grp * N2 + a.N)[c + k * kRowLanes] = db[k];
    }
  __syncthreads();
  for (int j = threadIdx.x; j < N2; j += kThreads) {
    float acc = 0.f;
    for (int q = 0; q < kTileRows; ++q) acc += sums[q * N2 + j];
    a.part[(int64_t)blockIdx.x * N2 + j] = acc;
  }
}

// dgamma[c] = sum over the partial rows of part[b][0][c], dbeta[c] = ... part[b][1][c]: lane q of 16 adds rows q, q + 16, ...
// in order, then the 16 lane sums are added in lane order.  grid ceil(2 N / 64)
__global__ void __launch_bounds__(kAgCols* kAgLanes) row_linear_affine_kernel(const float* __restrict__ part, int blocks, int N,
                                                                             float* __restrict__ dgamma, float* __restrict__ dbeta)
{
  __shared__ float t[kAgLanes][kAgCols];
  const int N2 = 2 * N, col = threadIdx.x % kAgCols, q = threadIdx.x / kAgCols;
  const int j = blockIdx.x * kAgCols + col;
  float acc = 0.f;
  if (j < N2)
    for (int b = q; b < blocks; b += kAgLanes) acc += part[(int64_t)b * N2 + j];
  t[q][col] = acc;
  __syncthreads();
  if (q != 0 || j >= N2) return;
  acc = 0.f;
  for (int k = 0; k < kAgLanes; ++k) acc += t[k][col];
  if (j < N) {
    if (dgamma) dgamma[j] = acc;
  } else if (dbeta) {
    dbeta[j - N] = acc;
  }
}

template <int KIND, typename XT>
void launch_one(const rl_args& a, hipStream_t st)
{
  auto kern = row_linear_kernel<KIND, XT>;
  const dim3 grid((unsigned)((a.n_rows + kTileRows - 1) / kTileRows));
  const size_t lds = (size_t)kTileRows * (a.SD + (a.use_b ? a.SN : 0)) * 4;      // at most 16 x (1028 + 260) floats = 82 KB
  WG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, kThreads, lds, st>>>(a);
}

template <typename XT>
void launch_kind(const rl_args& a, int kind, hipStream_t st)
{
  if (kind == 0) launch_one<0, XT>(a, st);
  else if (kind == 1) launch_one<1, XT>(a, st);
  else launch_one<2, XT>(a, st);
}

inline bool vec_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline void require_shape(int K, int N)
{
  if (!wgamd_row_linear_supported(K, N))
    throw logic_error(fmt("unsupported shape: K=%d (multiple of 4, 4 .. 1024), N=%d (multiple of 4, 4 .. 256)", K, N));
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_row_linear_supported(int K, int N)
{
  return K % 4 == 0 && K >= 4 && K <= 1024 && N % 4 == 0 && N >= 4 && N <= 256;
}

extern "C" int64_t wgamd_row_linear_bwd_blocks(int64_t n_rows, int N)
{
  if (n_rows <= 0 || N < 4 || N > 256 || N % 4 != 0) return 0;
  return std::min<int64_t>((n_rows + wgamd::kTileRows - 1) / wgamd::kTileRows, wgamd::kBwdBlocks);
}

extern "C" wholememory_error_code_t wgamd_row_linear_f32(const void* x, wholememory_dtype_t x_dtype, int64_t ldx, const void* ids,
                                                         wholememory_dtype_t ids_dtype, int64_t n_rows, int K, const float* weight,
                                                         int64_t ldw, int N, const float* bias, int relu, int norm,
                                                         const float* gamma, const float* beta, float eps, const float* add,
                                                         int64_t ld_add, float* out, int64_t ldo, float* kept_x, int64_t ld_kx,
                                                         float* kept_y, int64_t ld_ky, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_row_linear_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    WG_REQUIRE_INPUT(norm >= WGAMD_ROW_LINEAR_NORM_NONE && norm <= WGAMD_ROW_LINEAR_NORM_L2 && eps >= 0.f, "norm must be 0, 1 or 2 and eps >= 0");
    const bool x32 = x_dtype == WHOLEMEMORY_DT_FLOAT;
    WG_REQUIRE_INPUT(x32 || x_dtype == WHOLEMEMORY_DT_HALF || x_dtype == WHOLEMEMORY_DT_BF16, "x must be FLOAT, HALF or BF16");
    WG_REQUIRE_INPUT(ids == nullptr || ids_dtype == WHOLEMEMORY_DT_INT || ids_dtype == WHOLEMEMORY_DT_INT64, "ids must be INT or INT64");
    require_shape(K, N);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(x && weight && out, "null pointer");
    WG_REQUIRE_INPUT(ldx >= K && ldw >= K && ldo >= N && (add == nullptr || ld_add >= N) && (kept_x == nullptr || ld_kx >= K) &&
                       (kept_y == nullptr || ld_ky >= N), "leading dimension too small");
    if ((reinterpret_cast<uintptr_t>(x) & (x32 ? 15 : 7)) || ldx % 4 != 0)
      throw logic_error("x rows must be 16-B aligned (float32) or 8-B aligned (16-bit)");
    if (!aligned_rows(weight, ldw) || !aligned_rows(out, ldo) || (add && !aligned_rows(add, ld_add)) ||
        (kept_x && !aligned_rows(kept_x, ld_kx)) || (kept_y && !aligned_rows(kept_y, ld_ky)) || !vec_ok(gamma) || !vec_ok(beta))
      throw logic_error("weight / out / add / kept rows, gamma and beta must be 16-B aligned (leading dimensions multiples of 4)");
    rl_args a{};
    a.x = x, a.ldx = ldx, a.ids = ids, a.n_rows = n_rows, a.K = K, a.wt = weight, a.ldw = ldw, a.N = N, a.bias = bias;
    a.relu = relu ? 1 : 0, a.norm = norm, a.gamma = norm == WGAMD_ROW_LINEAR_NORM_LAYER ? gamma : nullptr;
    a.beta = norm == WGAMD_ROW_LINEAR_NORM_LAYER ? beta : nullptr, a.eps = eps;
    a.add = add, a.ld_add = ld_add, a.out = out, a.ldo = ldo, a.kept_x = kept_x, a.ld_kx = ld_kx, a.kept_y = kept_y, a.ld_ky = ld_ky;
    a.K16 = (K + 15) / 16 * 16, a.SD = a.K16 + 4;      // rows 4 banks apart, as the GCN tile
    a.N16 = (N + 15) / 16 * 16, a.SN = a.N16 + 4;
    a.use_b = norm != WGAMD_ROW_LINEAR_NORM_NONE || add != nullptr || kept_y != nullptr;
    const int kind = ids == nullptr ? 0 : ids_dtype == WHOLEMEMORY_DT_INT ? 1 : 2;
    auto st = static_cast<hipStream_t>(stream);
    if (x32) launch_kind<float>(a, kind, st);
    else if (x_dtype == WHOLEMEMORY_DT_HALF) launch_kind<_Float16>(a, kind, st);
    else launch_kind<__bf16>(a, kind, st);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_row_linear_bwd_f32(const float* kept_y, int64_t ld_ky, const float* grad_out, int64_t ldg,
                                                             int64_t n_rows, int N, int relu, int norm, const float* gamma, float eps,
                                                             float* dy, int64_t ld_dy, float* partials, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_row_linear_bwd_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    WG_REQUIRE_INPUT(norm >= WGAMD_ROW_LINEAR_NORM_NONE && norm <= WGAMD_ROW_LINEAR_NORM_L2 && eps >= 0.f, "norm must be 0, 1 or 2 and eps >= 0");
    require_shape(4, N);
    if (n_rows == 0) return;
    const bool reads_y = relu || norm != WGAMD_ROW_LINEAR_NORM_NONE;
    WG_REQUIRE_INPUT(grad_out && dy && (kept_y || !reads_y), "null pointer");
    WG_REQUIRE_INPUT(ldg >= N && ld_dy >= N && (!reads_y || ld_ky >= N), "leading dimension too small");
    if (!aligned_rows(grad_out, ldg) || !aligned_rows(dy, ld_dy) || (reads_y && !aligned_rows(kept_y, ld_ky)) || !vec_ok(gamma) ||
        !vec_ok(partials))
      throw logic_error("kept_y / grad_out / dy rows, gamma and partials must be 16-B aligned (leading dimensions multiples of 4)");
    rlb_args a{};
    a.y = kept_y, a.ldy = ld_ky, a.g = grad_out, a.ldg = ldg, a.n_rows = n_rows, a.N = N, a.relu = relu ? 1 : 0, a.norm = norm;
    a.gamma = gamma, a.eps = eps, a.dy = dy, a.ld_dy = ld_dy;
    a.part = norm == WGAMD_ROW_LINEAR_NORM_LAYER ? partials : nullptr;
    a.blocks = (int)wgamd_row_linear_bwd_blocks(n_rows, N);
    const size_t lds = a.part ? (size_t)kTileRows * 2 * N * sizeof(float) : 0;      // 32 KB at N = 256
    auto st = static_cast<hipStream_t>(stream);
    if (N <= 64) row_linear_bwd_kernel<1><<<(unsigned)a.blocks, kThreads, lds, st>>>(a);
    else if (N <= 128) row_linear_bwd_kernel<2><<<(unsigned)a.blocks, kThreads, lds, st>>>(a);
    else row_linear_bwd_kernel<4><<<(unsigned)a.blocks, kThreads, lds, st>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_row_linear_affine_grad_f32(const float* partials, int64_t n_rows, int N, float* dgamma,
                                                                     float* dbeta, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_row_linear_affine_grad_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    require_shape(4, N);
    if (dgamma == nullptr && dbeta == nullptr) return;
    const int blocks = (int)wgamd_row_linear_bwd_blocks(n_rows, N);      // no partial rows: zeros
    WG_REQUIRE_INPUT(blocks == 0 || partials != nullptr, "null partials");
    row_linear_affine_kernel<<<(unsigned)((2 * N + kAgCols - 1) / kAgCols), kAgCols * kAgLanes, 0, static_cast<hipStream_t>(stream)>>>(
      partials, blocks, N, dgamma, dbeta);
    WG_HIP_CHECK(hipGetLastError());
  });
}
