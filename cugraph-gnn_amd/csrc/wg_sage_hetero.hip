// Heterogeneous SAGE layer (torch_geometric.nn.HeteroConv({edge type: SAGEConv}, aggr="sum"), what to_hetero makes of a SAGEConv
// layer) over one (hop, destination type) of a call group — the sum over the relations ending in the type as ONE product:
//     C[i]   = [ REDUCE_{r_1}(i) | REDUCE_{r_2}(i) | ... | XD[dst_rows[i]] ]           K = sum_r F_r + F_dst floats
//     out[p] = act( C[i] @ wt^T + bias + acc_in[i] ),  p = out_rows ? out_rows[i] : i
//     REDUCE_r(i) = (mean ? 1 / deg_r(i) : 1) sum_{e in row i of r} s_r[col_r[e]] X_r[col_r[e]]      (s_r nullable = 1)
// with wt = [ W_l^{r_1} | W_l^{r_2} | ... | sum_r W_r^r ] ([N, K]) and bias = sum_r b_r built by the host.  Every relation has
// its own CSR over the same n_rows frontier entries, its own input rows (X_r[j] = x_r[ids_r ? ids_r[j] : j], the kind of the
// node list chosen per relation at run time: node types of one call group are lazy or resident independently) and its own
// width F_r.
//
// hetero_sage_kernel — one workgroup of 256 threads per 16-row tile, as the other layer kernels.  Phase 1: the C row is K / 4
// <= 256 float4 chunks, one chunk per thread (chunk -> relation block and feature float4), held in a register while the thread
// walks its relation's edges of its rows, scaled and flushed to the LDS tile at each row boundary; sums run in CSR order, compensated
// (Kahan): a row of thousands of edges is as close to float64 as a short one.  The
// chain bounds -> column -> id -> row is what bounds such a walk, not bytes, so it is cut in two: the tile's edges (one range
// of every relation's CSR) are resolved to row addresses by all 256 threads, one edge per thread, and staged in LDS piece by
// piece; the walk then has the row loads alone in flight, 16 per thread.  When K / 4 <= 128 several rows are built at once
// (P = 2, 4, ... slots of K / 4 threads).  Phase 2:
// tile_times_wt (wg_layer_parts.hpp) with the running sum of an earlier launch and the row placement.
// The same kernel runs the input gradient of a source type over the relations' transposes: rows = the type's input rows, one
// descriptor per (hop, relation) leaving it with x = that group's dZ, col = the transpose's destination rows, s = 1 / deg of
// the destination row for a mean relation, wt = the relations' W_l transposed and stacked.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kUnroll = 16;
constexpr int kMaxK   = 1024;
constexpr int kMaxRel = WGAMD_HETERO_SAGE_MAX_RELATIONS;
constexpr int kStage  = 768;    // edges staged per piece, all relations together (9 KB next to the tile: 3 workgroups per CU at K = 640)

struct hsage_args : hetero_frame {              // (kept = c_out: the C rows)
  wgamd_hetero_sage_relation_t rel[kMaxRel];
  int Q, P;                   // Q = K / 4 chunks; P row slots (power of 2, P Q <= 256)
};

__global__ void __launch_bounds__(kThreads) hetero_sage_kernel(hsage_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int rp[kMaxRel][kTileRows + 1];
  __shared__ const float* srow[kStage];     // a piece's edges as row addresses ...
  __shared__ float sw[kStage];              // ... and per-source-row factors
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
  load_row_windows(rp, a.rel, a.n_rel, row0, rows_here);
  zero_tile_padding(tile, a.SD, a.K, a.K16);
  __syncthreads();

  // ---- phase 1: C rows -> LDS.  Thread = (slot, chunk q); chunk q is feature float4 c of relation block b (or of the root) ----
  const int slot = tid / a.Q, q = tid % a.Q;
  const int rps = kTileRows / a.P;
  const int lr0 = slot * rps, lr1 = slot < a.P ? std::min(lr0 + rps, rows_here) : lr0;
  const bool root = slot < a.P && a.x_dst != nullptr && 4 * q >= a.root_col0;
  if (root) {                                                     // the root block: the destination's own row
    const int c = q - a.root_col0 / 4;
    for (int lr = lr0; lr < lr1; ++lr) {
      const int64_t self = a.dst_rows ? a.dst_rows[row0 + lr] : row0 + lr;
      reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] =
        reinterpret_cast<const f32x4*>(row_of(a.x_dst, a.ldx_dst, a.dst_ids, a.dst_kind, self))[c];
    }
  }
  // a relation block: the tile's edges of every relation are one range of its CSR.  They are taken in pieces of `cap` edges per
  // relation: all 256 threads resolve the piece's edges to row addresses (column -> node id -> address, every edge its own
  // thread: the dependent loads of a piece run side by side) and stage them in LDS, then the chunk threads walk their rows'
  // edges of the piece with the row loads alone in flight.
  int b = 0;
  while (b + 1 < a.n_rel && 4 * q >= a.rel[b + 1].col0) ++b;
  const bool walks = slot < a.P && !root && a.n_rel > 0 && lr0 < lr1;
  const int c = a.n_rel > 0 ? q - a.rel[b].col0 / 4 : 0;
  const bool scaled = a.n_rel > 0 && a.rel[b].src_scale != nullptr;
  const bool mean = a.n_rel > 0 && a.rel[b].mean != 0;
  const int* rpb = rp[b];
  int lr = lr0, row_end = walks ? rpb[lr0 + 1] : 0;
  int e = walks ? rpb[lr0] : 0;
  const int e_end = walks ? rpb[lr1] : 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  f32x4 lost = {0.f, 0.f, 0.f, 0.f};          // Kahan: what the adds into acc rounded away so far (a 3000-edge mean row within 1e-6)
  const int cap = a.n_rel > 0 ? (kStage / a.n_rel) & ~15 : kStage;
  int n_pieces = 0;
  for (int r = 0; r < a.n_rel; ++r) n_pieces = std::max(n_pieces, (rp[r][rows_here] - rp[r][0] + cap - 1) / cap);
  for (int piece = 0; piece < n_pieces; ++piece) {
    for (int i = tid; i < a.n_rel * cap; i += kThreads) {
      const int r = i / cap, k = i % cap;
      const int es = rp[r][0] + piece * cap + k;
      if (es < rp[r][rows_here]) {
        const wgamd_hetero_sage_relation_t& R = a.rel[r];
        const int j = R.col[es];
        srow[i] = row_of(R.x, R.ldx, R.src_ids, R.ids_kind, j);
        sw[i]   = R.src_scale ? R.src_scale[j] : 1.f;
      }
    }
    __syncthreads();
    if (walks) {
      const int p0 = rpb[0] + piece * cap;                        // the piece's first edge of my relation
      const int p_end = std::min(e_end, p0 + cap);
      const float* const* prow = srow + b * cap - p0;
      const float* pw = sw + b * cap - p0;
      const bool mine = e < p_end;                 // (false: my rows' edges start in a later piece, or are done)
      for (; e < p_end; e += kUnroll) {
        f32x4 v[kUnroll];
        float w[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          w[u] = 1.f;
          if (e + u < p_end) {
            v[u] = reinterpret_cast<const f32x4*>(prow[e + u])[c];
            if (scaled) w[u] = pw[e + u];
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (e + u < p_end) {
            while (e + u >= row_end) {                // the edge starts a later row: the finished row goes to the tile
              const int deg = rpb[lr + 1] - rpb[lr];
              if (mean && deg > 1) acc *= 1.f / (float)deg;
              reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] = acc;
              acc     = f32x4{0.f, 0.f, 0.f, 0.f};
              lost    = f32x4{0.f, 0.f, 0.f, 0.f};
              row_end = rpb[++lr + 1];
            }
            const f32x4 y = (scaled ? w[u] * v[u] : v[u]) - lost;
            const f32x4 s = acc + y;
            lost = (s - acc) - y;
            acc  = s;
          }
        }
      }
      if (mine) e = p_end;                         // (the last batch of the piece may have run past its end)
    }
    __syncthreads();
  }
  if (slot < a.P) {
    if (!root && a.n_rel > 0) {
      for (; lr < lr1; ++lr) {                        // the last row with edges, then rows without
        const int deg = rpb[lr + 1] - rpb[lr];
        if (mean && deg > 1) acc *= 1.f / (float)deg;
        reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] = acc;
        acc = lost = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    for (int lz = std::max(lr0, rows_here); lz < lr0 + rps; ++lz)   // tile rows past the last row: zero
      reinterpret_cast<f32x4*>(tile + lz * a.SD)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  if (a.kept) keep_tile_rows(tile, a.SD, a.K, rows_here, a.kept, a.ld_kept, row0);   // C, for the weight gradient

  // ---- phase 2: [16 x K16] tile @ wt^T ----
  tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldw, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows, a.acc_in, a.ld_acc,
                a.out_rows);
}

int64_t total_k(const int* F, int n_rel, int F_dst)
{
  int64_t K = F_dst;
  for (int r = 0; r < n_rel; ++r) K += F[r];
  return K;
}

wholememory_error_code_t launch(const char* what, const wgamd_hetero_sage_relation_t* rels, int n_rel, int64_t n_rows,
                                const float* x_dst, int64_t ldx_dst, int F_dst, const int64_t* dst_rows, const void* dst_ids,
                                int dst_ids_kind, const float* wt, int64_t ldw, int N, const float* bias, int flags,
                                const float* acc_in, int64_t ld_acc, const int64_t* out_rows, float* out, int64_t ldo, float* c_out,
                                int64_t ldc, void* stream)
{
  return guarded(what, [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && n_rel >= 0 && n_rel <= kMaxRel && F_dst >= 0, "bad sizes");
    WG_REQUIRE_INPUT(n_rel == 0 || rels != nullptr, "null pointer");
    int Fs[kMaxRel];
    for (int r = 0; r < n_rel; ++r) Fs[r] = rels[r].F;
    if (!wgamd_hetero_sage_layer_supported(Fs, n_rel, x_dst ? F_dst : 0, N))
      throw logic_error(fmt("unsupported shape: every F a multiple of 4, N=%d (<= 256), K=%lld (in (0, %d])", N,
                            (long long)total_k(Fs, n_rel, x_dst ? F_dst : 0), kMaxK));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(wt && out, "null pointer");
    hsage_args a{};
    int at = 0;
    for (int r = 0; r < n_rel; ++r) {
      const wgamd_hetero_sage_relation_t& R = rels[r];
      WG_REQUIRE_INPUT(R.row_ptr && R.col && R.x, "null pointer");
      WG_REQUIRE_INPUT(R.ids_kind >= 0 && R.ids_kind <= 2 && (R.ids_kind == 0) == (R.src_ids == nullptr), "bad node list kind");
      WG_REQUIRE_INPUT(R.ldx >= R.F, "leading dimension too small");
      WG_REQUIRE_INPUT(R.col0 == at, "relation blocks must be back to back from column 0");
      if (!aligned_rows(R.x, R.ldx)) throw logic_error("x rows must be 16-B aligned");
      a.rel[r] = R;
      at += R.F;
    }
    fill_hetero_frame(a, n_rel, n_rows, at, x_dst, ldx_dst, F_dst, dst_rows, dst_ids, dst_ids_kind, wt, ldw, N, bias,
                      flags & WGAMD_HETERO_SAGE_RELU, acc_in, ld_acc, out_rows, out, ldo, c_out, ldc,
                      "c_out rows must be 16-B aligned, ldc >= K");
    a.Q   = a.K / 4;
    a.P   = 1;
    while (a.P < kTileRows && 2 * a.P * a.Q <= kThreads) a.P *= 2;
    launch_tiles(hetero_sage_kernel, a, static_cast<hipStream_t>(stream));
    WG_HIP_CHECK(hipGetLastError());
  });
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_hetero_sage_layer_supported(const int* F, int n_rel, int F_dst, int N)
{
  if (n_rel < 0 || n_rel > wgamd::kMaxRel || F_dst < 0 || F_dst % 4 != 0 || N <= 0 || N > 256) return 0;
  for (int r = 0; r < n_rel; ++r)
    if (F[r] <= 0 || F[r] % 4 != 0) return 0;
  const int64_t K = wgamd::total_k(F, n_rel, F_dst);
  return K > 0 && K <= wgamd::kMaxK;
}

extern "C" wholememory_error_code_t wgamd_hetero_sage_layer_f32(const wgamd_hetero_sage_relation_t* rels, int n_rel, int64_t n_rows,
                                                                const float* x_dst, int64_t ldx_dst, int F_dst,
                                                                const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind,
                                                                const float* wt, int64_t ldw, int N, const float* bias, int flags,
                                                                const float* acc_in, int64_t ld_acc, const int64_t* out_rows,
                                                                float* out, int64_t ldo, void* stream)
{
  return wgamd::launch("wgamd_hetero_sage_layer_f32", rels, n_rel, n_rows, x_dst, ldx_dst, F_dst, dst_rows, dst_ids, dst_ids_kind, wt,
                       ldw, N, bias, flags, acc_in, ld_acc, out_rows, out, ldo, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_hetero_sage_layer_f32_train(const wgamd_hetero_sage_relation_t* rels, int n_rel,
                                                                      int64_t n_rows, const float* x_dst, int64_t ldx_dst, int F_dst,
                                                                      const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind,
                                                                      const float* wt, int64_t ldw, int N, const float* bias,
                                                                      int flags, const float* acc_in, int64_t ld_acc,
                                                                      const int64_t* out_rows, float* out, int64_t ldo, float* c_out,
                                                                      int64_t ldc, void* stream)
{
  if (c_out == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  return wgamd::launch("wgamd_hetero_sage_layer_f32_train", rels, n_rel, n_rows, x_dst, ldx_dst, F_dst, dst_rows, dst_ids,
                       dst_ids_kind, wt, ldw, N, bias, flags, acc_in, ld_acc, out_rows, out, ldo, c_out, ldc, stream);
}
