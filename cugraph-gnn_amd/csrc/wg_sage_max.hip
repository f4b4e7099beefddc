// SAGE layer with the max ("pooling") or min aggregator (torch_geometric.nn.SAGEConv(aggr="max" | "min"), flow
// source_to_target) over a sampled hop, forward and the routing half of its backward:
//     out[i, :] = act( W_l red_{e in row i} X[col[e]]  +  W_r X[self_rows[i]]  +  b ),      red = element-wise max or min
// X[r] = x[src_ids[r]] when the rows are read through a node list.  An empty row reduces to 0 (PyG's result for an isolated
// node).  The reduce is a compare-and-select walk, not a sum: it cannot ride the MFMA operands of the mean / sum layer kernels,
// and its backward is a routing problem — every (row, feature) sends its gradient to exactly ONE edge.
//
// Pieces:
//   * sage_max_layer_kernel — the whole layer, one launch per hop: 16-row tiles, 4 waves, one LDS tile [16 x K16], K = 2 F (F
//     without a root weight).  Phase 1: lane groups of LG lanes (the power of two >= F / 4; one float4 of a row per lane) walk a
//     destination row's edges 8 at a time (ids and rows of 8 edges in flight per lane group) and keep a running float4 best
//     and, when the argument is asked for, an int4 of the CSR edge SLOT e that produced it.  The compare is strict, so the
//     lowest slot wins a tie; the first edge of a row is always taken, so +-inf rows behave as IEEE compares do (NaN inputs are
//     outside the contract).  Best -> tile columns [0, F) (and agg_out, arg_out), the self row -> [F, 2 F), padding zeroed.
//     Phase 2: the tile times [W_l | W_r]^T read as two torch.nn.Linear weights (tile_times_two_wt, wg_layer_parts.hpp) on
//     the exact fp32 matrix pipe, bias and ReLU fused, one store.  MIN is a compile-time flag of the same body.
//   * sage_max_bwd_src_kernel — gx[j, f] = sum over the entries t of row j of the hop's transpose of
//     [arg[col_t[t], f] == perm[t]] dAgg[col_t[t], f]: the gradient of the reduce w.r.t. the input rows.  The compare is
//     against the edge slot, not the source id: a sampled duplicate edge (same source, two slots) is counted once.  No
//     atomics.  A workgroup owns 16 source rows; a row of at most 64 entries is one lane group's walk, a longer one (a hub
//     source is a row of thousands) is cut into 64-entry pieces that ALL lane groups of the workgroup take round-robin, each
//     adding its pieces up in order, and the groups' sums are added in group order from LDS: a fixed order, the same bits
//     from run to run.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int kUnroll = 8;
constexpr int kPiece  = 64;   // entries per piece of a long transposed row

struct sage_max_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* x;
  int64_t ldx;
  int F;
  const void* src_ids;
  const int64_t* self_rows;   // null exactly when w_r is: no root block
  const float* w_l;           // [N, ldwl] row-major
  int64_t ldwl;
  const float* w_r;           // nullable: [N, ldwr] row-major
  int64_t ldwr;
  int N;
  const float* bias;
  int relu;
  float* out;
  int64_t ldo;
  float* agg_out;             // nullable
  int64_t ld_agg;
  int* arg_out;               // ARG: [n_rows, ld_arg] CSR edge slots, -1 for an empty row
  int64_t ld_arg;
  int lg_shift;               // a lane group is 1 << lg_shift lanes (>= F / 4)
  int K, K16, SD;             // tile: width, width rounded up to 16, floats per row
};

// The reduce of destination row i, features [4 c, 4 c + 4) (c < F / 4), and the CSR slots it came from
template <int KIND, bool MIN, bool ARG>
__device__ __forceinline__ void reduce_chunk(const sage_max_args& a, int64_t i, int c, bool active, f32x4& best, i32x4& slot)
{
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  best = f32x4{0.f, 0.f, 0.f, 0.f};
  slot = i32x4{-1, -1, -1, -1};
#pragma unroll 1      // (unrolled further the select chains of two batches cost 260 VGPRs instead of 90: one wave per SIMD)
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
    for (int u = 0; u < kUnroll; ++u) {
      if (j[u] < 0) continue;
      const bool first = e + u == s;      // the row's first edge is taken whatever it holds (-inf under max included)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool take = first || (MIN ? v[u][k] < best[k] : v[u][k] > best[k]);
        best[k] = take ? v[u][k] : best[k];
        if constexpr (ARG) slot[k] = take ? e + u : slot[k];
      }
    }
  }
}

template <int KIND, bool MIN, bool ARG>
__global__ void __launch_bounds__(kThreads) sage_max_layer_kernel(sage_max_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;

  // ---- phase 1: [ reduce | self ] rows of the tile -> LDS (and agg_out, arg_out) ----
  const int groups = kThreads >> a.lg_shift;
  const int grp = tid >> a.lg_shift, c = tid & ((1 << a.lg_shift) - 1);
  const bool active = c < a.F / 4;
  for (int r = grp; r < kTileRows; r += groups) {
    const int64_t i = row0 + r;
    f32x4 best = {0.f, 0.f, 0.f, 0.f}, self = {0.f, 0.f, 0.f, 0.f};
    if (i < a.n_rows) {
      i32x4 slot;
      reduce_chunk<KIND, MIN, ARG>(a, i, c, active, best, slot);
      if (active) {
        if (a.agg_out) reinterpret_cast<f32x4*>(a.agg_out + i * a.ld_agg)[c] = best;
        if constexpr (ARG) reinterpret_cast<i32x4*>(a.arg_out + i * a.ld_arg)[c] = slot;
        if (a.self_rows) {
          const int64_t sr = a.self_rows[i];
          if (sr >= 0) self = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, sr))[c];
        }
      }
    }
    if (active) {
      reinterpret_cast<f32x4*>(tile + r * a.SD)[c] = best;
      if (a.self_rows) reinterpret_cast<f32x4*>(tile + r * a.SD + a.F)[c] = self;
    }
  }
  zero_tile_padding(tile, a.SD, a.K, a.K16);
  __syncthreads();

  // ---- phase 2: [16 x K16] tile @ [W_l | W_r]^T ----
  tile_times_two_wt(tile, a.SD, a.F, a.K, a.K16, a.w_l, a.ldwl, a.w_r, a.ldwr, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows);
}

struct sage_max_bwd_args {
  const int* row_ptr_t;       // the hop's transpose: rows = input rows
  const int* col_t;           // destination row of every entry
  const int* perm;            // the hop's CSR edge slot of every entry
  int64_t n_src;
  const int* arg;             // [n_dst, ld_arg]: what the forward kept
  int64_t ld_arg;
  const float* dagg;          // [n_dst, ld_dagg] = dZ W_l
  int64_t ld_dagg;
  int F;
  float* gx;                  // [n_src, ldgx], every row written
  int64_t ldgx;
  int lg_shift;
};

// sum over the entries [s, t) of [arg[col_t, f] == perm] dagg[col_t, f], features [4 c, 4 c + 4), in entry order
__device__ __forceinline__ f32x4 route_entries(const sage_max_bwd_args& a, int s, int t, int c, bool active)
{
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int e = s; e < t; e += kUnroll) {
    int d[kUnroll], p[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      d[u] = e + u < t ? a.col_t[e + u] : -1;
      p[u] = e + u < t ? a.perm[e + u] : -2;      // (never a kept slot: those are -1 or an edge)
    }
    i32x4 w[kUnroll];
    f32x4 g[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      w[u] = i32x4{-1, -1, -1, -1};
      g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (d[u] >= 0 && active) {
        w[u] = reinterpret_cast<const i32x4*>(a.arg + (int64_t)d[u] * a.ld_arg)[c];
        g[u] = reinterpret_cast<const f32x4*>(a.dagg + (int64_t)d[u] * a.ld_dagg)[c];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += w[u][k] == p[u] ? g[u][k] : 0.f;
  }
  return acc;
}

__global__ void __launch_bounds__(kThreads) sage_max_bwd_src_kernel(sage_max_bwd_args a)
{
  __shared__ f32x4 part[kThreads];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int LG = 1 << a.lg_shift, groups = kThreads >> a.lg_shift;
  const int grp = tid >> a.lg_shift, c = tid & (LG - 1);
  const bool active = c < a.F / 4;

  // rows of at most kPiece entries: one lane group each
  for (int r = grp; r < kTileRows; r += groups) {
    const int64_t j = row0 + r;
    if (j >= a.n_src) break;
    const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
    if (t - s > kPiece) continue;
    const f32x4 acc = route_entries(a, s, t, c, active);
    if (active) reinterpret_cast<f32x4*>(a.gx + j * a.ldgx)[c] = acc;
  }

  // longer rows: every lane group takes pieces round-robin (r, s, t are the same in every thread: the barriers are uniform)
  for (int r = 0; r < kTileRows; ++r) {
    const int64_t j = row0 + r;
    if (j >= a.n_src) break;
    const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
    if (t - s <= kPiece) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p0 = s + grp * kPiece; p0 < t; p0 += groups * kPiece) {
      const f32x4 piece = route_entries(a, p0, std::min(t, p0 + kPiece), c, active);
      acc += piece;
    }
    __syncthreads();      // (the previous long row's sums have been read)
    part[tid] = acc;
    __syncthreads();
    if (grp == 0 && active) {
      f32x4 total = part[c];
      for (int g = 1; g < groups; ++g) total += part[g * LG + c];
      reinterpret_cast<f32x4*>(a.gx + j * a.ldgx)[c] = total;
    }
  }
}

// the power of two >= F / 4, at least 4 lanes
int lane_group_shift(int F)
{
  int s = 2;
  while ((1 << s) < F / 4) ++s;
  return s;
}

template <int KIND, bool MIN>
void launch_layer(const sage_max_args& a, hipStream_t st)
{
  if (a.arg_out) launch_tiles(sage_max_layer_kernel<KIND, MIN, true>, a, st);
  else launch_tiles(sage_max_layer_kernel<KIND, MIN, false>, a, st);
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_sage_max_layer_supported(int F, int N, int has_root)
{
  return F >= 4 && F % 4 == 0 && (has_root ? 2 * F : F) <= 1024 && N >= 1 && N <= 256;
}

extern "C" wholememory_error_code_t wgamd_sage_max_layer_f32_train(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                                   int64_t ldx, int F, const void* src_ids,
                                                                   wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                                   const float* w_l, int64_t ldwl, const float* w_r, int64_t ldwr,
                                                                   int N, const float* bias, int flags, float* out, int64_t ldo,
                                                                   float* agg_out, int64_t ld_agg, int* arg_out, int64_t ld_arg,
                                                                   void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_sage_max_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    const bool has_root = w_r != nullptr;
    if (!wgamd_sage_max_layer_supported(F, N, has_root))
      throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, >= 4, tile width %d <= 1024), N=%d (1 .. 256)", F,
                            has_root ? 2 * F : F, N));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && w_l && out, "null pointer");
    WG_REQUIRE_INPUT(has_root == (self_rows != nullptr), "self_rows is given exactly when w_r is");
    WG_REQUIRE_INPUT(ldwl >= F && (!has_root || ldwr >= F) && ldo >= N && (agg_out == nullptr || ld_agg >= F) &&
                       (arg_out == nullptr || ld_arg >= F), "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(w_l, ldwl) || (has_root && !aligned_rows(w_r, ldwr)) ||
        (agg_out && !aligned_rows(agg_out, ld_agg)) || (arg_out && !aligned_rows(arg_out, ld_arg)))
      throw logic_error("x / w_l / w_r / agg_out / arg_out rows must be 16-B aligned");
    sage_max_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F, a.src_ids = src_ids;
    a.self_rows = self_rows, a.w_l = w_l, a.ldwl = ldwl, a.w_r = w_r, a.ldwr = ldwr, a.N = N, a.bias = bias;
    a.relu = (flags & WGAMD_SAGE_MAX_RELU) != 0;
    a.out = out, a.ldo = ldo, a.agg_out = agg_out, a.ld_agg = ld_agg, a.arg_out = arg_out, a.ld_arg = ld_arg;
    a.lg_shift = lane_group_shift(F);
    a.K   = has_root ? 2 * F : F;
    tile_geometry(a.K, a.K16, a.SD);
    auto st = static_cast<hipStream_t>(stream);
    with_kind(kind, [&](auto k) {
      if (flags & WGAMD_SAGE_MAX_MIN) launch_layer<decltype(k)::value, true>(a, st);
      else launch_layer<decltype(k)::value, false>(a, st);
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_sage_max_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                             int64_t ldx, int F, const void* src_ids,
                                                             wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                             const float* w_l, int64_t ldwl, const float* w_r, int64_t ldwr, int N,
                                                             const float* bias, int flags, float* out, int64_t ldo, void* stream)
{
  return wgamd_sage_max_layer_f32_train(row_ptr, col, n_rows, x, ldx, F, src_ids, src_ids_dtype, self_rows, w_l, ldwl, w_r, ldwr, N,
                                        bias, flags, out, ldo, nullptr, 0, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_sage_max_bwd_src_f32(const int* row_ptr_t, const int* col_t, const int* perm, int64_t n_src,
                                                               const int* arg, int64_t ld_arg, const float* dagg, int64_t ld_dagg,
                                                               int F, float* gx, int64_t ldgx, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_sage_max_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    if (!(F >= 4 && F % 4 == 0 && F <= 1024)) throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, 4 .. 1024)", F));
    if (n_src == 0) return;
    WG_REQUIRE_INPUT(row_ptr_t && col_t && perm && arg && dagg && gx, "null pointer");
    WG_REQUIRE_INPUT(ld_arg >= F && ld_dagg >= F && ldgx >= F, "leading dimension too small");
    if (!aligned_rows(arg, ld_arg) || !aligned_rows(dagg, ld_dagg) || !aligned_rows(gx, ldgx))
      throw logic_error("arg / dagg / gx rows must be 16-B aligned");
    sage_max_bwd_args a{row_ptr_t, col_t, perm, n_src, arg, ld_arg, dagg, ld_dagg, F, gx, ldgx, lane_group_shift(F)};
    const unsigned blocks = (unsigned)((n_src + kTileRows - 1) / kTileRows);
    sage_max_bwd_src_kernel<<<blocks, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
