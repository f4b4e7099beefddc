// Relational GCN layer (torch_geometric.nn.RGCNConv / FastRGCNConv, flow source_to_target) over a sampled hop:
//     out[i, :] = act( sum_b C_b[i] @ basis_b  +  X[self_rows[i]] @ root  +  bias )
//     C_b[i]    = sum_{e = (j -> i)} n_e comp[r_e, b] X[j]          (b < B; comp = I and B = R without bases)
// with n_e = 1 / |{e' into i : r_e' = r_e}| (aggr "mean") or 1 ("add"), X[r] = x[src_ids[r]] when the rows are read through a
// node list.  The model of the reference's cugraph-pyg example rgcn_link_class_mnmg.py (FastRGCNConv, num_bases = 30).
//
// Pieces:
//   * rgcn_coef_kernel — one launch per hop: per edge rel (int32) and n_e (float32).  One wave per destination row; the count of
//     an edge's relation in its row is a ballot match over the relation id's bits (ceil(log2 R) ballots per 64 x 64 edge
//     block), so any degree is exact; rows of <= 64 edges (every sampled hop) are a single block.  An id outside [0, R) gets
//     n_e = 0 and rel 0: no later read depends on it (the caller refuses such ids before launching; this keeps the device safe).
//   * rgcn_layer_kernel — the whole layer, one launch per hop: 16-row tiles, 256 threads.  Phase 1: the C row of a destination
//     is K = (B + root) F floats, K / 4 <= 256 float4 chunks, one chunk per thread held in a register while the thread walks
//     the edges of its rows (edge metadata of 16 edges in flight, then their row chunks), flushed to the LDS tile at each row
//     boundary.  When K / 4 <= 128 several rows are built at once (P = 2, 4, ... slots of K / 4 threads).  Phase 2: the
//     [16 x K] tile times the stacked weight [basis_0; ...; basis_{B-1}; root] (tile_times_wt, wg_layer_parts.hpp); the
//     weight is passed transposed ([N, K]) so a lane reads one float4 along k.
//     The same kernel runs the input gradient over the hop's transpose (dZ as x, basis_b^T / root^T as the weight).
//   * rgcn_wgrad_kernel + rgcn_wgrad_reduce_kernel — M[s] = sum_{p in segment s} c_p X[src_p]^T G[dst_p] over (source row,
//     gradient row, coefficient) pairs sorted by segment (relation, or R for the root's self pairs): work items of at most S
//     pairs of one segment on fp32 MFMA, the item partials added in item order — no atomics, the same bits from run to run.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kUnroll = 16;
constexpr int kMaxK   = 1024;

// ---- per-edge coefficients ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) rgcn_coef_kernel(const int* __restrict__ row_ptr, int64_t n_rows, const T* __restrict__ etype,
                                                        int R, int nbits, int mean, int* __restrict__ rel, float* __restrict__ coef)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_rows) return;          // (wave-uniform)
  const int s = row_ptr[i], t = row_ptr[i + 1];
  for (int a0 = s; a0 < t; a0 += 64) {
    const int ea = a0 + lane;
    int ra = -1;
    if (ea < t) {
      const T v = etype[ea];
      ra = (v >= 0 && v < (T)R) ? (int)v : -1;
    }
    int cnt = 0;
    if (mean) {
      for (int b0 = s; b0 < t; b0 += 64) {
        const int eb = b0 + lane;
        int rb = -1;
        if (eb < t) {
          const T v = etype[eb];
          rb = (v >= 0 && v < (T)R) ? (int)v : -1;
        }
        uint64_t m = __ballot(rb >= 0);
        for (int k = 0; k < nbits; ++k) {
          const uint64_t bk = __ballot(rb >= 0 && ((rb >> k) & 1));
          m &= ((ra >> k) & 1) ? bk : ~bk;
        }
        cnt += __popcll(m);
      }
    }
    if (ea < t) {
      rel[ea]  = ra < 0 ? 0 : ra;
      coef[ea] = ra < 0 ? 0.f : (mean ? 1.f / (float)cnt : 1.f);
    }
  }
}

// ---- the layer ----------------------------------------------------------------------------------------------------------------
struct rgcn_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* x;
  int64_t ldx;
  int F;
  const void* src_ids;
  const int64_t* self_rows;   // input row of destination i itself (< 0: none); read only with the root block
  const int* rel;
  const float* coef;
  const float* comp;          // [R, B] row-major; null = identity (B = R)
  int B;
  int has_root;
  const float* wt;            // [N, ldw]: wt[n, b F + f] = basis_b[f, n], wt[n, B F + f] = root[f, n]
  int64_t ldw;
  int N;
  const float* bias;
  int relu;
  float* out;
  int64_t ldo;
  int K, K16, SD, Q, P;       // K = (B + has_root) F; Q = K / 4 chunks; P row slots (power of 2, P Q <= 256)
};

template <int KIND>
__global__ void __launch_bounds__(kThreads) rgcn_layer_kernel(rgcn_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int rp[kTileRows + 1];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
  if (tid <= kTileRows) rp[tid] = a.row_ptr[row0 + std::min(tid, rows_here)];
  zero_tile_padding(tile, a.SD, a.K, a.K16);
  __syncthreads();

  // ---- phase 1: C rows -> LDS.  Thread = (slot, chunk q); chunk q is feature float4 c of block b ----
  const int slot = tid / a.Q, q = tid % a.Q;
  if (slot < a.P) {
    const int C4 = a.F / 4, b = q / C4, c = q % C4;
    const int rps = kTileRows / a.P;
    const int lr0 = slot * rps, lr1 = std::min(lr0 + rps, rows_here);
    if (b == a.B) {                                   // the root block: the destination's own row
      for (int lr = lr0; lr < lr1; ++lr) {
        const int64_t self = a.self_rows[row0 + lr];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (self >= 0) v = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, self))[c];
        reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] = v;
      }
    } else if (lr0 < lr1) {
      int lr = lr0, row_end = rp[lr0 + 1];
      const int e_end = rp[lr1];
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int e = rp[lr0]; e < e_end; e += kUnroll) {
        int j[kUnroll];
        float w[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          j[u] = -1;
          w[u] = 0.f;
          if (e + u < e_end) {
            j[u]          = a.col[e + u];
            const int r   = a.rel[e + u];
            const float n = a.coef[e + u];
            w[u] = a.comp ? n * a.comp[(int64_t)r * a.B + b] : (r == b ? n : 0.f);
          }
        }
        f32x4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (w[u] != 0.f) v[u] = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j[u]))[c];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (e + u < e_end) {
            while (e + u >= row_end) {                // the edge starts a later row: the finished row goes to the tile
              reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] = acc;
              acc     = f32x4{0.f, 0.f, 0.f, 0.f};
              row_end = rp[++lr + 1];
            }
            acc += w[u] * v[u];
          }
        }
      }
      for (; lr < lr1; ++lr) {                        // the last row with edges, then rows without
        reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] = acc;
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    for (int lr = std::max(lr0, rows_here); lr < lr0 + rps; ++lr)   // tile rows past the last row: zero
      reinterpret_cast<f32x4*>(tile + lr * a.SD)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  // ---- phase 2: [16 x K16] tile @ wt^T ----
  tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldw, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows);
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------
// Workgroup (item, by): item = (segment s, k-th run of at most S pairs of it); features [64 by, 64 by + 64), wave w the outputs
// [64 w, 64 w + 64) as 4 x 4 tiles of 16 x 16.  A = G^T (16 outputs x 4 pairs), B = c X (4 pairs x 16 features).
template <int KIND>
__global__ void __launch_bounds__(256) rgcn_wgrad_kernel(const float* __restrict__ x, int64_t ldx, int F, const void* src_ids,
                                                         const int64_t* __restrict__ psrc, const int64_t* __restrict__ pdst,
                                                         const float* __restrict__ pcoef, const float* __restrict__ g, int64_t ldg,
                                                         int N, const int64_t* __restrict__ item_start,
                                                         const int64_t* __restrict__ seg_ptr, int n_seg, int64_t S,
                                                         float* __restrict__ part)
{
  const int64_t item = blockIdx.x;
  if (item >= item_start[n_seg]) return;
  int lo = 0, hi = n_seg - 1;                         // the segment: last s with item_start[s] <= item
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (item_start[mid] <= item) lo = mid;
    else hi = mid - 1;
  }
  const int64_t p_begin = seg_ptr[lo] + (item - item_start[lo]) * S, p_end = std::min(seg_ptr[lo + 1], p_begin + S);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const int n0 = wave * 64, f0 = blockIdx.y * 64;
  if (n0 >= N) return;
  f32x4 acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t p0 = p_begin; p0 < p_end; p0 += 4) {
    const int64_t p = p0 + kq;
    float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p < p_end) {
      const float* gr = g + pdst[p] * ldg;
      const float* xr = x_row<KIND>(x, ldx, src_ids, psrc[p]);
      const float cf  = pcoef[p];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + m, f = f0 + 16 * t + m;
        if (n < N) av[t] = gr[n];
        if (f < F) bv[t] = cf * xr[f];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[v], acc[u][v], 0, 0, 0);
  }
  float* out = part + item * ((int64_t)F * N);
  // C/D: col (feature) = lane & 15, row (output) = 4 (lane >> 4) + reg; stored [F, N]
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int n = n0 + 16 * u + 4 * kq + reg, f = f0 + 16 * v + m;
        if (n < N && f < F) out[(int64_t)f * N + n] = acc[u][v][reg];
      }
}

__global__ void rgcn_wgrad_reduce_kernel(const float* __restrict__ part, const int64_t* __restrict__ item_start, int n_seg, int64_t FN,
                                         float* __restrict__ M)
{
  const int64_t total = (int64_t)n_seg * FN;
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = o / FN, w = o % FN;
    float acc = 0.f;
    for (int64_t it = item_start[s]; it < item_start[s + 1]; ++it) acc += part[it * FN + w];
    M[o] = acc;
  }
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_rgcn_layer_supported(int F, int N, int B, int has_root)
{
  const int64_t K = ((int64_t)B + (has_root ? 1 : 0)) * F;
  return F > 0 && F % 4 == 0 && N > 0 && N <= 256 && B >= 0 && K > 0 && K <= wgamd::kMaxK;
}

extern "C" wholememory_error_code_t wgamd_rgcn_edge_coef(const int* row_ptr, int64_t n_rows, const void* edge_type,
                                                         wholememory_dtype_t edge_type_dtype, int R, int mean, int* rel, float* coef,
                                                         void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_rgcn_edge_coef", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && R > 0, "bad sizes");
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && edge_type && rel && coef, "null pointer");
    int nbits = 1;
    while ((1LL << nbits) < (int64_t)R) ++nbits;
    auto st              = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n_rows + 3) / 4);
    if (edge_type_dtype == WHOLEMEMORY_DT_INT)
      rgcn_coef_kernel<int32_t><<<blocks, 256, 0, st>>>(row_ptr, n_rows, static_cast<const int32_t*>(edge_type), R, nbits, mean, rel, coef);
    else if (edge_type_dtype == WHOLEMEMORY_DT_INT64)
      rgcn_coef_kernel<int64_t><<<blocks, 256, 0, st>>>(row_ptr, n_rows, static_cast<const int64_t*>(edge_type), R, nbits, mean, rel, coef);
    else throw invalid_input("edge_type must be INT or INT64");
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_rgcn_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                         int64_t ldx, int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                         const int64_t* self_rows, const int* rel, const float* coef,
                                                         const float* comp, int B, int has_root, const float* wt, int64_t ldw,
                                                         int N, const float* bias, int relu, float* out, int64_t ldo, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_rgcn_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    if (!wgamd_rgcn_layer_supported(F, N, B, has_root))
      throw logic_error(fmt("unsupported shape: F=%d (multiple of 4), N=%d (<= 256), (B + root) F = %lld (<= %d)", F, N,
                            (long long)(B + (has_root ? 1 : 0)) * F, kMaxK));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && wt && out && (B == 0 || (rel && coef)) && (!has_root || self_rows), "null pointer");
    WG_REQUIRE_INPUT(ldo >= N, "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    rgcn_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F, a.src_ids = src_ids;
    a.self_rows = self_rows, a.rel = rel, a.coef = coef, a.comp = comp, a.B = B, a.has_root = has_root ? 1 : 0;
    a.wt = wt, a.ldw = ldw, a.N = N, a.bias = bias, a.relu = relu ? 1 : 0, a.out = out, a.ldo = ldo;
    a.K   = (B + a.has_root) * F;
    a.K16 = (a.K + 15) / 16 * 16;
    a.SD  = a.K16 + 4;      // rows 4 banks apart: the 16 rows of a fragment read spread over the 64 banks
    a.Q   = a.K / 4;
    a.P   = 1;
    while (a.P < kTileRows && 2 * a.P * a.Q <= kThreads) a.P *= 2;
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    WG_REQUIRE_INPUT(ldw >= a.K, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(wt, ldw)) throw logic_error("x / wt rows must be 16-B aligned");
    with_kind(kind, [&](auto k) { launch_tiles(rgcn_layer_kernel<decltype(k)::value>, a, static_cast<hipStream_t>(stream)); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" size_t wgamd_rgcn_wgrad_workspace_bytes(int64_t max_items, int F, int N)
{
  if (F <= 0 || N <= 0 || N > 256 || max_items < 0) return 0;
  return (size_t)max_items * F * N * 4;
}

extern "C" wholememory_error_code_t wgamd_rgcn_wgrad_f32(const float* x, int64_t ldx, int F, const void* src_ids,
                                                         wholememory_dtype_t src_ids_dtype, const int64_t* pair_src,
                                                         const int64_t* pair_dst, const float* pair_coef, const float* grad,
                                                         int64_t ldg, int N, const int64_t* item_start, const int64_t* seg_ptr,
                                                         int n_seg, int64_t pairs_per_item, int64_t max_items, float* M,
                                                         void* workspace, size_t workspace_bytes, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_rgcn_wgrad_f32", [&] {
    WG_REQUIRE_INPUT(F > 0 && N > 0 && n_seg > 0 && max_items >= 0 && pairs_per_item > 0 && pairs_per_item % 4 == 0, "bad sizes");
    if (N > 256) throw logic_error(fmt("unsupported shape: N=%d (<= 256)", N));
    WG_REQUIRE_INPUT(M && item_start && seg_ptr, "null pointer");
    auto st = static_cast<hipStream_t>(stream);
    const int64_t FN = (int64_t)F * N;
    if (max_items > 0) {
      WG_REQUIRE_INPUT(x && pair_src && pair_dst && pair_coef && grad && workspace, "null pointer");
      WG_REQUIRE_INPUT(workspace_bytes >= wgamd_rgcn_wgrad_workspace_bytes(max_items, F, N), "workspace too small");
      const int kind = ids_kind(src_ids, src_ids_dtype);
      WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
      WG_REQUIRE_INPUT(ldg >= N, "leading dimension too small");
      float* part = static_cast<float*>(workspace);
      const dim3 grid((unsigned)max_items, (F + 63) / 64);
      with_kind(kind, [&](auto k) {
        rgcn_wgrad_kernel<decltype(k)::value><<<grid, 256, 0, st>>>(x, ldx, F, src_ids, pair_src, pair_dst, pair_coef, grad, ldg, N,
                                                                      item_start, seg_ptr, n_seg, pairs_per_item, part);
      });
      WG_HIP_CHECK(hipGetLastError());
    }
    const int64_t total = (int64_t)n_seg * FN;
    const int blocks    = (int)std::min<int64_t>((total + 255) / 256, 16384);
    rgcn_wgrad_reduce_kernel<<<blocks, 256, 0, st>>>(static_cast<const float*>(workspace), item_start, n_seg, FN, M);
    WG_HIP_CHECK(hipGetLastError());
  });
}
