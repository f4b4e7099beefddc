// GCN layer (torch_geometric.nn.GCNConv, flow source_to_target, sum aggregation) over a sampled hop:
//     out[i, :] = act( dinv_i ( sum_{e = (j -> i), j != i} w_e dinv_j X[j]  +  loopw_i dinv_i X[i] ) @ W^T + b )
// with dinv = deg^-1/2 of add_remaining_self_loops (a sampled loop edge j == i is not summed: it sets loopw_i to its weight;
// loopw_i = fill = 1, or 2 when improved, otherwise), X[r] = x[src_ids[r]] when the rows are read through a node list.
// The GCN model of the reference's headline example (python/cugraph-pyg/cugraph_pyg/examples/gcn_dist_mnmg.py).
//
// Pieces:
//   * gcn_degrees_kernel — dinv of a layer's input rows from the hops that have those rows as destinations: one launch for
//     all hops of a layer graph (the degree of a vertex is the one of its row in the hop whose frontier it is in).
//   * gcn_layer_kernel — the whole layer, one launch per hop: 16-row tiles, 4 waves.  Phase 1: lane groups of LG lanes
//     (LG >= F / 4; one float4 of a row per lane) walk a destination row's edges 8 at a time (ids, dinv and rows of 8 edges
//     in flight per lane group), sum in CSR order and store the normalised aggregate row to the LDS tile (and to agg_out for
//     the weight gradient).  Phase 2: the [16 x F] tile times W^T (tile_times_wt, wg_layer_parts.hpp); W is read in its
//     torch.nn.Linear layout [N, F], no transposed copy.  Occupancy (several tiles per CU) overlaps the two phases; the layer
//     is bound by the latency of phase 1's dependent loads (row bounds -> column ids -> node ids / dinv -> rows), so small
//     tiles (more of them resident per CU, fewer accumulators) beat large ones: 16 rows 4.14 ms, 32 rows 4.38, 64 rows 5.03
//     at the products layer-1 shape (tools/bench_gcn.py).
//     The same kernel runs the input gradient over the hop's transpose (dinv_src / dinv_dst swapped, W^T as the weight).
//   * gcn_aggregate_kernel — the normalised aggregate alone for any F (shapes outside the layer kernel's domain: the
//     caller multiplies with a library GEMM).
//   * gcn_wgrad_kernel + gcn_wgrad_reduce_kernel — dW = dZ^T agg, db = colsum(dZ) (ReLU mask folded into dZ): split-K over
//     row ranges on fp32 MFMA, partial sums added in workgroup order (no atomics: the same bits from run to run).
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kUnroll = 8;

struct gcn_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* x;
  int64_t ldx;
  int F;
  const void* src_ids;
  const int64_t* self_rows;   // input row of destination i itself; < 0 = none (a source-only row of a transposed hop)
  const float* edge_w;        // nullable: 1 per edge
  const float* dinv_src;      // nullable (no normalisation): dinv of the input rows
  const float* dinv_dst;      // nullable: dinv_src[self_rows[i]] (or 1 when dinv_src is null too)
  float fill;
  int add_loops;
  const float* w;             // [N, ldw] row-major: out = agg W^T
  int64_t ldw;
  int N;
  const float* bias;
  int relu;
  float* out;
  int64_t ldo;
  float* agg_out;             // nullable
  int64_t ld_agg;
  int F16;                    // F rounded up to 16 (the MFMA k extent; the tile's columns past F are zero)
  int SD;                     // floats per LDS tile row
};

// The normalised aggregate of destination row i, features [4 c, 4 c + 4) (c < F / 4): same sums for every caller
template <int KIND>
__device__ __forceinline__ f32x4 aggregate_chunk(const gcn_args& a, int64_t i, int c, bool active)
{
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  const int64_t self = a.self_rows[i];
  float loopw = a.fill;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int e = s; e < t; e += kUnroll) {
    int j[kUnroll];
    float cf[kUnroll];
    bool take[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) j[u] = e + u < t ? a.col[e + u] : -1;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      take[u] = false;
      cf[u]   = 0.f;
      if (j[u] >= 0) {
        const float wgt = a.edge_w ? a.edge_w[e + u] : 1.f;
        if (a.add_loops && (int64_t)j[u] == self) {
          loopw = wgt;             // the loop edge is not summed: it gives the added loop its weight (the last one wins)
        } else {
          take[u] = true;
          cf[u]   = a.dinv_src ? wgt * a.dinv_src[j[u]] : wgt;
        }
      }
    }
    f32x4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (take[u] && active) v[u] = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j[u]))[c];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) acc += cf[u] * v[u];
  }
  if (a.add_loops && self >= 0) {
    const float cs = a.dinv_src ? loopw * a.dinv_src[self] : loopw;
    if (active) acc += cs * reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, self))[c];
  }
  const float scale = a.dinv_dst ? a.dinv_dst[i] : (a.dinv_src && self >= 0 ? a.dinv_src[self] : 1.f);
  return scale * acc;
}

template <int KIND, int LG>
__global__ void __launch_bounds__(kThreads) gcn_layer_kernel(gcn_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;

  // ---- phase 1: the normalised aggregate rows of the tile -> LDS (and agg_out) ----
  constexpr int kGroups = kThreads / LG;
  const int grp = tid / LG, c = tid % LG;
  const int C4 = a.F / 4, C16 = a.F16 / 4;
  for (int r = grp; r < kTileRows; r += kGroups) {
    const int64_t i = row0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < a.n_rows) {
      v = aggregate_chunk<KIND>(a, i, c, c < C4);
      if (a.agg_out && c < C4) reinterpret_cast<f32x4*>(a.agg_out + i * a.ld_agg)[c] = v;
    }
    if (c < C16) reinterpret_cast<f32x4*>(tile + r * a.SD)[c] = c < C4 ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cc = c + LG; cc < C16; cc += LG) reinterpret_cast<f32x4*>(tile + r * a.SD)[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  // ---- phase 2: [16 x F16] tile @ W^T ----
  tile_times_wt(tile, a.SD, a.F, a.F16, a.w, a.ldw, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows);
}

// normalised aggregate only, any F: one wave per row, one feature per lane and 64-feature block
template <int KIND>
__global__ void __launch_bounds__(256) gcn_aggregate_kernel(gcn_args a)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_rows) return;
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  const int64_t self = a.self_rows[i];
  float loopw = a.fill;
  for (int e = s; e < t; ++e)
    if (a.add_loops && (int64_t)a.col[e] == self) loopw = a.edge_w ? a.edge_w[e] : 1.f;
  const float cs = a.dinv_src && self >= 0 ? loopw * a.dinv_src[self] : loopw;
  const float scale = a.dinv_dst ? a.dinv_dst[i] : (a.dinv_src && self >= 0 ? a.dinv_src[self] : 1.f);
  for (int f0 = 0; f0 < a.F; f0 += 64) {
    const int f = f0 + lane;
    float acc = 0.f;
    for (int e = s; e < t; ++e) {
      const int j = a.col[e];
      if (a.add_loops && (int64_t)j == self) continue;
      const float wgt = a.edge_w ? a.edge_w[e] : 1.f;
      const float cf  = a.dinv_src ? wgt * a.dinv_src[j] : wgt;
      if (f < a.F) acc += cf * x_row<KIND>(a.x, a.ldx, a.src_ids, j)[f];
    }
    if (a.add_loops && self >= 0 && f < a.F) acc += cs * x_row<KIND>(a.x, a.ldx, a.src_ids, self)[f];
    if (f < a.F) a.out[i * a.ldo + f] = scale * acc;
  }
}

struct degree_hops {
  const int* row_ptr[WGAMD_GCN_MAX_HOPS];
  const int* col[WGAMD_GCN_MAX_HOPS];
  const int64_t* self_rows[WGAMD_GCN_MAX_HOPS];
  const float* edge_w[WGAMD_GCN_MAX_HOPS];
  int64_t first[WGAMD_GCN_MAX_HOPS + 1];   // prefix of the hops' row counts
  int64_t out_base[WGAMD_GCN_MAX_HOPS];    // output index = out_base + i, or self_rows[i] when < 0
  int n_hops;
};

__global__ void __launch_bounds__(256) gcn_degrees_kernel(degree_hops d, float fill, int add_loops, float* dinv, int64_t n_out)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < d.first[d.n_hops]; r += (int64_t)gridDim.x * blockDim.x) {
    int h = 0;
    while (r >= d.first[h + 1]) ++h;
    const int64_t i = r - d.first[h];
    const int s = d.row_ptr[h][i], t = d.row_ptr[h][i + 1];
    const int64_t self = d.self_rows[h][i];
    const float* ew = d.edge_w[h];
    float deg = 0.f, loopw = fill;
    for (int e = s; e < t; ++e) {
      const float wgt = ew ? ew[e] : 1.f;
      if (add_loops && (int64_t)d.col[h][e] == self) loopw = wgt;
      else deg += wgt;
    }
    if (add_loops) deg += loopw;
    const int64_t o = d.out_base[h] >= 0 ? d.out_base[h] + i : self;
    if (o >= 0 && o < n_out) dinv[o] = deg > 0.f ? 1.f / sqrtf(deg) : 0.f;
  }
}

// dW partial sums: workgroup (bx, by) owns rows [bx rpb, (bx + 1) rpb) and features [64 by, 64 by + 64); wave w owns the
// outputs [64 w, 64 w + 64) as 4 x 4 tiles of 16 x 16.  A = dZ^T (16 outputs x 4 rows), B = agg (4 rows x 16 features).
template <bool MASK>
__global__ void __launch_bounds__(256) gcn_wgrad_kernel(const float* __restrict__ agg, int64_t ld_agg, int64_t n_rows, int F,
                                                        const float* __restrict__ g, int64_t ldg, const float* __restrict__ act,
                                                        int64_t ld_act, int N, int64_t rows_per_block, float* __restrict__ part)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const int n0 = wave * 64, f0 = blockIdx.y * 64;
  if (n0 >= N) return;
  const int64_t r_begin = blockIdx.x * rows_per_block, r_end = std::min(n_rows, r_begin + rows_per_block);
  f32x4 acc[4][4];
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = r_begin; r0 < r_end; r0 += 4) {
    const int64_t r = r0 + kq;
    float av[4], bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 16 * t + m, f = f0 + 16 * t + m;
      av[t] = 0.f;
      bv[t] = 0.f;
      if (r < r_end && n < N) {
        av[t] = g[r * ldg + n];
        if (MASK && !(act[r * ld_act + n] > 0.f)) av[t] = 0.f;
      }
      if (r < r_end && f < F) bv[t] = agg[r * ld_agg + f];
      bsum[t] += av[t];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
  const int64_t NF = (int64_t)N * F;
  float* p = part + ((int64_t)blockIdx.x) * (NF + N);
  // C/D: col (feature) = lane & 15, row (output) = 4 (lane >> 4) + reg
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int n = n0 + 16 * a + 4 * kq + reg, f = f0 + 16 * b + m;
        if (n < N && f < F) p[(int64_t)n * F + f] = acc[a][b][reg];
      }
  if (blockIdx.y == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float v = bsum[t];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      const int n = n0 + 16 * t + m;
      if (kq == 0 && n < N) p[NF + n] = v;
    }
  }
}

__global__ void gcn_wgrad_reduce_kernel(const float* __restrict__ part, int grid_x, int N, int F, float* grad_w, float* grad_b,
                                        int accumulate)
{
  const int64_t NF = (int64_t)N * F, total = NF + N;
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    if (o >= NF && grad_b == nullptr) continue;
    float s = 0.f;
    for (int b = 0; b < grid_x; ++b) s += part[(int64_t)b * total + o];
    float* dst = o < NF ? grad_w + o : grad_b + (o - NF);
    *dst = accumulate ? *dst + s : s;
  }
}

constexpr int kWgradMaxGridX     = 128;
constexpr int kWgradMaxGridXWide = 1024;   // _split: operands of many more rows than a hop has (a link head's whole tables)

int wgrad_grid_x(int64_t n_rows, int max_split = kWgradMaxGridX)
{
  return (int)std::max<int64_t>(1, std::min<int64_t>(max_split, (n_rows + 511) / 512));
}

template <int KIND>
void launch_layer(const gcn_args& a, hipStream_t st)
{
  const int c4 = a.F / 4;
  if (c4 <= 4) launch_tiles(gcn_layer_kernel<KIND, 4>, a, st);
  else if (c4 <= 8) launch_tiles(gcn_layer_kernel<KIND, 8>, a, st);
  else if (c4 <= 16) launch_tiles(gcn_layer_kernel<KIND, 16>, a, st);
  else if (c4 <= 32) launch_tiles(gcn_layer_kernel<KIND, 32>, a, st);
  else launch_tiles(gcn_layer_kernel<KIND, 64>, a, st);
}

gcn_args make_args(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
                   const int64_t* self_rows, const float* edge_w, const float* dinv_src, const float* dinv_dst, float fill,
                   int flags)
{
  gcn_args a{};
  a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F, a.src_ids = src_ids;
  a.self_rows = self_rows, a.edge_w = edge_w, a.dinv_src = dinv_src, a.dinv_dst = dinv_dst, a.fill = fill;
  a.add_loops = (flags & WGAMD_GCN_ADD_SELF_LOOPS) != 0;
  a.relu      = (flags & WGAMD_GCN_RELU) != 0;
  return a;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_gcn_layer_supported(int F, int N) { return F > 0 && F % 4 == 0 && F <= 256 && N > 0 && N <= 256; }

extern "C" wholememory_error_code_t wgamd_gcn_degrees_f32(int n_hops, const int* const* row_ptr, const int* const* col,
                                                          const int64_t* const* self_rows, const float* const* edge_weight,
                                                          const int64_t* n_rows, const int64_t* out_base, float fill,
                                                          int add_self_loops, float* dinv, int64_t n_out, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gcn_degrees_f32", [&] {
    WG_REQUIRE_INPUT(n_hops >= 0 && n_hops <= WGAMD_GCN_MAX_HOPS, "n_hops must be in [0, %d]", WGAMD_GCN_MAX_HOPS);
    WG_REQUIRE_INPUT(n_out >= 0 && (n_out == 0 || dinv != nullptr), "bad output");
    degree_hops d{};
    d.n_hops = n_hops;
    for (int h = 0; h < n_hops; ++h) {
      WG_REQUIRE_INPUT(n_rows[h] >= 0, "bad row count");
      WG_REQUIRE_INPUT(n_rows[h] == 0 || (row_ptr[h] && col[h] && self_rows[h]), "null pointer");
      d.row_ptr[h] = row_ptr[h], d.col[h] = col[h], d.self_rows[h] = self_rows[h];
      d.edge_w[h]   = edge_weight ? edge_weight[h] : nullptr;
      d.out_base[h] = out_base[h];
      d.first[h + 1] = d.first[h] + n_rows[h];
    }
    if (d.first[n_hops] == 0) return;
    auto st          = static_cast<hipStream_t>(stream);
    const int blocks = (int)std::min<int64_t>((d.first[n_hops] + 255) / 256, 8192);
    gcn_degrees_kernel<<<blocks, 256, 0, st>>>(d, fill, add_self_loops, dinv, n_out);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gcn_layer_f32_train(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                              int64_t ldx, int F, const void* src_ids,
                                                              wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                              const float* edge_weight, const float* dinv_src,
                                                              const float* dinv_dst, float fill, const float* w, int64_t ldw,
                                                              int N, const float* bias, int flags, float* out, int64_t ldo,
                                                              float* agg_out, int64_t ld_agg, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gcn_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    if (!wgamd_gcn_layer_supported(F, N)) throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, <= 256), N=%d (<= 256)", F, N));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && self_rows && w && out, "null pointer");
    WG_REQUIRE_INPUT(ldw >= F && ldo >= N && (agg_out == nullptr || ld_agg >= F), "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(w, ldw) || (agg_out && !aligned_rows(agg_out, ld_agg)))
      throw logic_error("x / w / agg_out rows must be 16-B aligned");
    gcn_args a = make_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, edge_weight, dinv_src, dinv_dst, fill, flags);
    a.w = w, a.ldw = ldw, a.N = N, a.bias = bias, a.out = out, a.ldo = ldo, a.agg_out = agg_out, a.ld_agg = ld_agg;
    a.F16 = (F + 15) / 16 * 16;
    a.SD  = a.F16 + 4;      // rows 4 banks apart: the 16 rows of a fragment read spread over the 64 banks
    with_kind(kind, [&](auto k) { launch_layer<decltype(k)::value>(a, static_cast<hipStream_t>(stream)); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gcn_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                        int64_t ldx, int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                        const int64_t* self_rows, const float* edge_weight, const float* dinv_src,
                                                        const float* dinv_dst, float fill, const float* w, int64_t ldw, int N,
                                                        const float* bias, int flags, float* out, int64_t ldo, void* stream)
{
  return wgamd_gcn_layer_f32_train(row_ptr, col, n_rows, x, ldx, F, src_ids, src_ids_dtype, self_rows, edge_weight, dinv_src,
                                   dinv_dst, fill, w, ldw, N, bias, flags, out, ldo, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_gcn_aggregate_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                            int64_t ldx, int F, const void* src_ids,
                                                            wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                            const float* edge_weight, const float* dinv_src,
                                                            const float* dinv_dst, float fill, int flags, float* out,
                                                            int64_t ldo, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gcn_aggregate_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && F > 0, "bad sizes");
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && self_rows && out, "null pointer");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT((kind == 3 || ldx >= F) && ldo >= F, "leading dimension too small");
    gcn_args a = make_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, edge_weight, dinv_src, dinv_dst, fill, flags);
    a.out = out, a.ldo = ldo;
    auto st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n_rows + 3) / 4);
    with_kind(kind, [&](auto k) { gcn_aggregate_kernel<decltype(k)::value><<<blocks, 256, 0, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" size_t wgamd_gcn_wgrad_split_workspace_bytes(int64_t n_rows, int F, int N, int max_split)
{
  using namespace wgamd;
  if (F <= 0 || N <= 0 || F > 256 || N > 256 || max_split < 1 || max_split > kWgradMaxGridXWide) return 0;
  return (size_t)wgrad_grid_x(n_rows, max_split) * ((size_t)N * F + N) * 4;
}

extern "C" size_t wgamd_gcn_wgrad_workspace_bytes(int64_t n_rows, int F, int N)
{
  return wgamd_gcn_wgrad_split_workspace_bytes(n_rows, F, N, wgamd::kWgradMaxGridX);
}

extern "C" wholememory_error_code_t wgamd_gcn_wgrad_split_f32(const float* agg, int64_t ld_agg, int64_t n_rows, int F,
                                                              const float* grad_out, int64_t ldg, const float* act_out,
                                                              int64_t ld_act, int N, float* grad_w, float* grad_bias, int accumulate,
                                                              int max_split, void* workspace, size_t workspace_bytes, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gcn_wgrad_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && F > 0 && N > 0 && max_split >= 1 && max_split <= kWgradMaxGridXWide, "bad sizes");
    if (F > 256 || N > 256) throw logic_error(fmt("unsupported shape: F=%d, N=%d (both <= 256)", F, N));
    WG_REQUIRE_INPUT(grad_w != nullptr, "null pointer");
    auto st = static_cast<hipStream_t>(stream);
    if (n_rows == 0) {
      if (!accumulate) {
        WG_HIP_CHECK(hipMemsetAsync(grad_w, 0, (size_t)N * F * 4, st));
        if (grad_bias) WG_HIP_CHECK(hipMemsetAsync(grad_bias, 0, (size_t)N * 4, st));
      }
      return;
    }
    WG_REQUIRE_INPUT(agg && grad_out && workspace, "null pointer");
    WG_REQUIRE_INPUT(ld_agg >= F && ldg >= N && (act_out == nullptr || ld_act >= N), "leading dimension too small");
    WG_REQUIRE_INPUT(workspace_bytes >= wgamd_gcn_wgrad_split_workspace_bytes(n_rows, F, N, max_split), "workspace too small");
    const int gx      = wgrad_grid_x(n_rows, max_split);
    const int64_t rpb = ((n_rows + gx - 1) / gx + 3) / 4 * 4;
    const int gx_used = (int)((n_rows + rpb - 1) / rpb);
    float* part       = static_cast<float*>(workspace);
    const dim3 grid(gx_used, (F + 63) / 64);
    if (act_out) gcn_wgrad_kernel<true><<<grid, 256, 0, st>>>(agg, ld_agg, n_rows, F, grad_out, ldg, act_out, ld_act, N, rpb, part);
    else gcn_wgrad_kernel<false><<<grid, 256, 0, st>>>(agg, ld_agg, n_rows, F, grad_out, ldg, act_out, ld_act, N, rpb, part);
    WG_HIP_CHECK(hipGetLastError());
    const int64_t total = (int64_t)N * F + N;
    gcn_wgrad_reduce_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(part, gx_used, N, F, grad_w, grad_bias, accumulate);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gcn_wgrad_f32(const float* agg, int64_t ld_agg, int64_t n_rows, int F,
                                                        const float* grad_out, int64_t ldg, const float* act_out, int64_t ld_act,
                                                        int N, float* grad_w, float* grad_bias, int accumulate, void* workspace,
                                                        size_t workspace_bytes, void* stream)
{
  return wgamd_gcn_wgrad_split_f32(agg, ld_agg, n_rows, F, grad_out, ldg, act_out, ld_act, N, grad_w, grad_bias, accumulate,
                                   wgamd::kWgradMaxGridX, workspace, workspace_bytes, stream);
}
