// GIN layer (torch_geometric.nn.GINConv, flow source_to_target) over a sampled hop, with the MLP of the GIN paper:
//     agg[i, :] = sum_{e = (j -> i)} X[j]  +  (1 + eps) X_self[i]                (every edge summed: loops and duplicates too)
//     out[i, :] = act2( act1(agg[i] @ W1^T + b1) @ W2^T + b2 )
// X[r] = x[src_ids[r]] when the rows are read through a node list; X_self[i] = x_dst[i] when a destination table is passed,
// X[self_rows[i]] otherwise (self_rows[i] < 0, or neither array: no self term).  The model of the reference's cugraph-pyg
// example dist_gin_sg.py (GINConv(MLP([in, hidden, hidden])) layers, then global_add_pool).
//
// Pieces:
//   * gin_layer_kernel — the whole layer, one launch per hop: 16-row tiles, 4 waves, two LDS tiles.  Phase 1 as
//     gcn_layer_kernel's (lane groups of LG >= F / 4 lanes, a row's edges 8 at a time, sums in CSR order) -> LDS tile A (and
//     agg_out).  Phase 2: tile A times W1^T (tile_times_wt, wg_layer_parts.hpp) with b1 and ReLU -> LDS tile B, the hidden
//     activation (and hidden_out).  Phase 3: tile B times W2^T with b2 and the output ReLU -> global memory.  With a null W2
//     phase 2 writes to global memory and the kernel ends: the one-product form, also what runs the input gradient over the
//     hop's transpose (W1^T as the weight).  STATS (a compile-time variant of the one-product form, the training forward of the
//     batch-norm route, wg_batch_norm.hip): phase 2 writes z = agg W1^T + b1 to LDS tile B, stores the rows to z_out, and one
//     thread per column writes the tile's (mean, M2) over its valid rows to partials[tile0 + tile][2][H], the row count to
//     counts[tile0 + tile].
//   * gin_aggregate_kernel — agg alone for any F (shapes outside the layer kernel's domain, or an nn that does not start with
//     a Linear).
//   * segment_sum_kernel — global_add_pool over a sorted batch vector given as segment offsets: one wave per (segment,
//     64-feature block), rows added in order (no atomics: the same bits from run to run), an empty segment gives zeros.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kUnroll = 8;

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

// The aggregate of destination row i, features [4 c, 4 c + 4) (c < F / 4)
template <int KIND>
__device__ __forceinline__ f32x4 aggregate_chunk(const gin_args& a, int64_t i, int c, bool active, float self_coef)
{
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int e = s; e < t; e += kUnroll) {
    int j[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) j[u] = e + u < t ? a.col[e + u] : -1;
    f32x4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j[u] >= 0 && active) v[u] = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j[u]))[c];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) acc += v[u];
  }
  const f32x4* self = self_row<KIND>(a, i);
  if (self && active) acc += self_coef * self[c];
  return acc;
}

template <int KIND, int LG, bool STATS>
__global__ void __launch_bounds__(kThreads) gin_layer_kernel(gin_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const float self_coef = 1.f + (a.eps ? *a.eps : 0.f);

  // ---- phase 1: the aggregate rows of the tile -> LDS tile A (and agg_out) ----
  constexpr int kGroups = kThreads / LG;
  const int grp = tid / LG, c = tid % LG;
  const int C4 = a.F / 4, C16 = a.F16 / 4;
  for (int r = grp; r < kTileRows; r += kGroups) {
    const int64_t i = row0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < a.n_rows) {
      v = aggregate_chunk<KIND>(a, i, c, c < C4, self_coef);
      if (a.agg_out && c < C4) reinterpret_cast<f32x4*>(a.agg_out + i * a.ld_agg)[c] = v;
    }
    if (c < C16) reinterpret_cast<f32x4*>(tile + r * a.SD)[c] = c < C4 ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cc = c + LG; cc < C16; cc += LG) reinterpret_cast<f32x4*>(tile + r * a.SD)[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  // ---- phase 2: [16 x F16] tile A @ W1^T ----
  if constexpr (STATS) {
    float* zt = tile + kTileRows * a.SD;    // tile B: z of all 16 rows (rows past n_rows hold b1: neither stored nor counted)
    tile_times_wt(tile, a.SD, a.F, a.F16, a.w1, a.ldw1, a.H, a.b1, 0, zt, a.SH, 0, kTileRows);
    __syncthreads();
    const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
    keep_tile_rows(zt, a.SH, a.H, rows_here, a.out, a.ldo, row0);
    const int64_t t = a.tile0 + blockIdx.x;
    if (tid < a.H) {
      float mean, m2;
      column_mean_m2(zt + tid, a.SH, rows_here, mean, m2);
      a.partials[t * 2 * a.H + tid] = mean;
      a.partials[(t * 2 + 1) * a.H + tid] = m2;
    }
    if (tid == 0) a.counts[t] = rows_here;
    return;
  }
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

// aggregate only, any F: one wave per row, one feature per lane and 64-feature block
template <int KIND>
__global__ void __launch_bounds__(256) gin_aggregate_kernel(gin_args a)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_rows) return;
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  const float self_coef = 1.f + (a.eps ? *a.eps : 0.f);
  const float* self = reinterpret_cast<const float*>(self_row<KIND>(a, i));
  for (int f0 = 0; f0 < a.F; f0 += 64) {
    const int f = f0 + lane;
    if (f >= a.F) continue;
    float acc = 0.f;
    for (int e = s; e < t; ++e) acc += x_row<KIND>(a.x, a.ldx, a.src_ids, a.col[e])[f];
    if (self) acc += self_coef * self[f];
    a.out[i * a.ldo + f] = acc;
  }
}

__global__ void __launch_bounds__(256) segment_sum_kernel(const float* __restrict__ x, int64_t ldx, int F,
                                                          const int64_t* __restrict__ offsets, int64_t n_seg,
                                                          float* __restrict__ out, int64_t ldo)
{
  const int lane = threadIdx.x & 63;
  const int n_fb = (F + 63) / 64;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= n_seg * n_fb) return;
  const int64_t g = item / n_fb;
  const int f = (int)(item % n_fb) * 64 + lane;
  if (f >= F) return;
  const int64_t s = offsets[g], t = offsets[g + 1];
  float acc = 0.f;
  for (int64_t r = s; r < t; ++r) acc += x[r * ldx + f];
  out[g * ldo + f] = acc;
}

template <int KIND, int LG, bool STATS>
void launch_one(const gin_args& a, hipStream_t st)
{
  auto kern = gin_layer_kernel<KIND, LG, STATS>;
  const dim3 grid((unsigned)((a.n_rows + kTileRows - 1) / kTileRows));
  const size_t lds = (size_t)kTileRows * (a.SD + (a.w2 || STATS ? a.SH : 0)) * 4;      // at most 2 x 16 x 260 floats = 33 KB
  kern<<<grid, kThreads, lds, st>>>(a);
}

template <int KIND, bool STATS = false>
void launch_layer(const gin_args& a, hipStream_t st)
{
  const int c4 = a.F / 4;
  if (c4 <= 4) launch_one<KIND, 4, STATS>(a, st);
  else if (c4 <= 8) launch_one<KIND, 8, STATS>(a, st);
  else if (c4 <= 16) launch_one<KIND, 16, STATS>(a, st);
  else if (c4 <= 32) launch_one<KIND, 32, STATS>(a, st);
  else launch_one<KIND, 64, STATS>(a, st);
}

gin_args make_args(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
                   const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps)
{
  gin_args a{};
  a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F, a.src_ids = src_ids;
  a.self_rows = self_rows, a.x_dst = x_dst, a.ldx_dst = ldx_dst, a.eps = eps;
  return a;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_gin_layer_supported(int F, int H, int N)
{
  if (!(F > 0 && F % 4 == 0 && F <= 256 && H > 0 && H <= 256 && N >= 0 && N <= 256)) return 0;
  return N == 0 || H % 4 == 0;
}

extern "C" wholememory_error_code_t wgamd_gin_layer_f32_train(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                              int64_t ldx, int F, const void* src_ids,
                                                              wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                              const float* x_dst, int64_t ldx_dst, const float* eps,
                                                              const float* w1, int64_t ldw1, int H, const float* b1,
                                                              const float* w2, int64_t ldw2, int N, const float* b2, int flags,
                                                              float* out, int64_t ldo, float* agg_out, int64_t ld_agg,
                                                              float* hidden_out, int64_t ld_hidden, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gin_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    WG_REQUIRE_INPUT((w2 == nullptr) == (N == 0), "N is 0 exactly when w2 is null (the one-product form)");
    if (!wgamd_gin_layer_supported(F, H, N))
      throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, <= 256), H=%d (<= 256; multiple of 4 with a second product), "
                            "N=%d (<= 256)", F, H, N));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && w1 && out, "null pointer");
    const int n_out = w2 ? N : H;
    WG_REQUIRE_INPUT(ldw1 >= F && (w2 == nullptr || ldw2 >= H) && ldo >= n_out, "leading dimension too small");
    WG_REQUIRE_INPUT((agg_out == nullptr || ld_agg >= F) && (hidden_out == nullptr || ld_hidden >= H) &&
                       (x_dst == nullptr || ldx_dst >= F), "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(w1, ldw1) || (w2 && !aligned_rows(w2, ldw2)) ||
        (x_dst && !aligned_rows(x_dst, ldx_dst)) || (agg_out && !aligned_rows(agg_out, ld_agg)) ||
        (hidden_out && !aligned_rows(hidden_out, ld_hidden)))
      throw logic_error("x / x_dst / w1 / w2 / agg_out / hidden_out rows must be 16-B aligned");
    gin_args a = make_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, x_dst, ldx_dst, eps);
    a.w1 = w1, a.ldw1 = ldw1, a.H = H, a.b1 = b1, a.relu1 = (flags & WGAMD_GIN_RELU_HIDDEN) != 0;
    a.w2 = w2, a.ldw2 = ldw2, a.N = N, a.b2 = b2, a.relu2 = (flags & WGAMD_GIN_RELU_OUT) != 0;
    a.out = out, a.ldo = ldo, a.agg_out = agg_out, a.ld_agg = ld_agg;
    a.hidden_out = w2 ? hidden_out : nullptr, a.ld_hidden = ld_hidden;
    a.F16 = (F + 15) / 16 * 16, a.SD = a.F16 + 4;      // rows 4 banks apart, as the GCN tile
    a.H16 = (H + 15) / 16 * 16, a.SH = a.H16 + 4;
    with_kind(kind, [&](auto k) { launch_layer<decltype(k)::value>(a, static_cast<hipStream_t>(stream)); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gin_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                        int64_t ldx, int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                        const int64_t* self_rows, const float* x_dst, int64_t ldx_dst,
                                                        const float* eps, const float* w1, int64_t ldw1, int H, const float* b1,
                                                        const float* w2, int64_t ldw2, int N, const float* b2, int flags,
                                                        float* out, int64_t ldo, void* stream)
{
  return wgamd_gin_layer_f32_train(row_ptr, col, n_rows, x, ldx, F, src_ids, src_ids_dtype, self_rows, x_dst, ldx_dst, eps, w1,
                                   ldw1, H, b1, w2, ldw2, N, b2, flags, out, ldo, nullptr, 0, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_gin_layer_f32_stats(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                              int64_t ldx, int F, const void* src_ids,
                                                              wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                              const float* x_dst, int64_t ldx_dst, const float* eps,
                                                              const float* w1, int64_t ldw1, int H, const float* b1, float* z_out,
                                                              int64_t ldz, float* agg_out, int64_t ld_agg, float* partials,
                                                              int* counts, int64_t tile0, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gin_layer_f32_stats", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && tile0 >= 0, "bad sizes");
    if (!wgamd_gin_layer_supported(F, H, 0) || H % 4 != 0)
      throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, <= 256), H=%d (multiple of 4, <= 256)", F, H));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && w1 && z_out && partials && counts, "null pointer");
    WG_REQUIRE_INPUT(ldw1 >= F && ldz >= H && (agg_out == nullptr || ld_agg >= F) && (x_dst == nullptr || ldx_dst >= F),
                     "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(w1, ldw1) || !aligned_rows(z_out, ldz) ||
        (x_dst && !aligned_rows(x_dst, ldx_dst)) || (agg_out && !aligned_rows(agg_out, ld_agg)))
      throw logic_error("x / x_dst / w1 / z_out / agg_out rows must be 16-B aligned");
    gin_args a = make_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, x_dst, ldx_dst, eps);
    a.w1 = w1, a.ldw1 = ldw1, a.H = H, a.b1 = b1;
    a.out = z_out, a.ldo = ldz, a.agg_out = agg_out, a.ld_agg = ld_agg;
    a.partials = partials, a.counts = counts, a.tile0 = tile0;
    a.F16 = (F + 15) / 16 * 16, a.SD = a.F16 + 4;
    a.H16 = (H + 15) / 16 * 16, a.SH = a.H16 + 4;
    with_kind(kind, [&](auto k) { launch_layer<decltype(k)::value, true>(a, static_cast<hipStream_t>(stream)); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gin_aggregate_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                            int64_t ldx, int F, const void* src_ids,
                                                            wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                            const float* x_dst, int64_t ldx_dst, const float* eps, float* out,
                                                            int64_t ldo, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gin_aggregate_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && F > 0, "bad sizes");
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && out, "null pointer");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT((kind == 3 || ldx >= F) && ldo >= F && (x_dst == nullptr || ldx_dst >= F), "leading dimension too small");
    if ((reinterpret_cast<uintptr_t>(x) & 3) || (x_dst && (reinterpret_cast<uintptr_t>(x_dst) & 3)))
      throw logic_error("x / x_dst must be 4-B aligned");
    gin_args a = make_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, x_dst, ldx_dst, eps);
    a.out = out, a.ldo = ldo;
    auto st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n_rows + 3) / 4);
    with_kind(kind, [&](auto k) { gin_aggregate_kernel<decltype(k)::value><<<blocks, 256, 0, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_segment_sum_f32(const float* x, int64_t ldx, int F, const int64_t* offsets,
                                                          int64_t n_segments, float* out, int64_t ldo, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_segment_sum_f32", [&] {
    WG_REQUIRE_INPUT(n_segments >= 0 && F > 0, "bad sizes");
    if (n_segments == 0) return;
    WG_REQUIRE_INPUT(offsets && out, "null pointer");      // (x may be null when every segment is empty)
    WG_REQUIRE_INPUT(ldx >= F && ldo >= F, "leading dimension too small");
    const int64_t items = n_segments * ((F + 63) / 64);
    segment_sum_kernel<<<(unsigned)((items + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(x, ldx, F, offsets, n_segments,
                                                                                                  out, ldo);
    WG_HIP_CHECK(hipGetLastError());
  });
}
