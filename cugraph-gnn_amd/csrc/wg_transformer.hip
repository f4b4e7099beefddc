// Graph transformer layer (torch_geometric.nn.TransformerConv, flow source_to_target) over a sampled hop, aggregate-first:
//     s_ijh   = u_ih . X[j] + w_ih . a_ij                      (u = W_k^T q / sqrt(C), w = W_e^T q / sqrt(C): per destination)
//     alpha   = softmax_j(s_ijh)                               (per destination row and head)
//     A_i     = [ agg_i0 | ... | agg_i(H-1) | XD[self_rows[i]] ],  agg_ih = sum_j alpha_ijh [X[j] | a_ij | 1 | 0 pad]
//     out_i   = act( A_i @ Wstack + bias )
// The query-key product q_i . k_j is linear in X[j], so the logits need only the per-destination vectors u, w (one library GEMM
// over the destination rows); lin_key's bias is constant over a row and cancels.  Each head block of A is W4 = ceil4(F + D + 1)
// wide (the tail is zero) so every block starts 16-B aligned.  The model of the reference's cugraph-pyg example mag_lp_mnmg.py.
//
// Pieces:
//   * tconv_layer_kernel — the whole layer, one launch per hop: 16-row tiles, 256 threads.  Phase 1: one wave per destination
//     row, lane = one float4 of the source row (F <= 256) and, for lane <= D, one column of [a_ij | 1].  The row's edges go by
//     in groups of 4 (4 neighbour rows in flight); each group's H logits are wave sums (xor butterflies: every lane ends with
//     the same bits) and an online softmax (running max and sum, accumulators rescaled once per group) keeps any degree exact.
//     The finished row goes to the LDS tile (and, when training, to A in global memory: the weight gradient reads it, and the
//     backward's row sums sum_j alpha dalpha are dA_ih . A_ih — cheaper to keep than to rebuild).  The logits are written to
//     alpha [E, H] as they are made and turned into alpha by a second pass over the row once its max and sum are known.
//     Phase 2: the [16 x K] tile times Wstack (passed transposed, [N, K]; tile_times_wt, wg_layer_parts.hpp), bias and
//     ReLU fused.
//   * tconv_bwd_dst_kernel — destination-major: per edge and head dalpha = dA_ih . [X[j] | a_ij | 1] and
//     ds = alpha (dalpha - dA_ih . A_ih); du_ih = sum ds X[j], dw_ih = sum ds a_ij, ds written [E, H].  One wave per row.
//   * tconv_bwd_src_kernel — source-major over the hop's transpose (HopGraph.transposed with the edge permutation):
//     dX[j] = sum_e sum_h (alpha dA_ih[:F] + ds u_ih) plus the skip block of dA where input row j is a destination itself.
//     One wave per input row.
// No atomics anywhere: every sum runs in CSR (or transposed-CSR) order, the same bits from run to run.
#include "wg_transformer_parts.hpp"

namespace wgamd {
namespace {

struct tconv_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* x;             // source rows X[r] = x[src_ids ? src_ids[r] : r]
  int64_t ldx;
  int F;
  const void* src_ids;
  const float* xd;            // destination rows XD[self_rows[i]]; read through src_ids when xd_ids
  int64_t ldxd;
  int Fd;                     // 0: no skip block
  const int64_t* self_rows;
  int xd_ids;
  const float* edge_attr;     // [E, D] in CSR order (D = 0: none)
  int D;
  const float* u;             // [n_rows, ldu]: u[i, h F + f]
  int64_t ldu;
  const float* w;             // [n_rows, ldw]: w[i, h D + d]
  int64_t ldw;
  int H;
  const float* wt;            // [N, ldwt] = Wstack^T
  int64_t ldwt;
  int N;
  const float* bias;
  int relu;
  float* out;
  int64_t ldo;
  float* alpha;               // [E, H] or null
  float* a_save;              // [n_rows, K] or null
  int W4, K, K16, SD;
};

template <int KIND, int HM>
__global__ void __launch_bounds__(kThreads) tconv_layer_kernel(tconv_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int rp[kTileRows + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
  if (tid <= kTileRows) rp[tid] = a.row_ptr[row0 + std::min(tid, rows_here)];
  zero_tile_padding(tile, a.SD, a.K, a.K16);
  __syncthreads();

  // ---- phase 1: one wave per destination row (tconv_row_walk, wg_transformer_parts.hpp) ----
  for (int lr = wave; lr < kTileRows; lr += 4) {
    float* trow = tile + lr * a.SD;
    if (lr >= rows_here) {
      for (int q = lane; q < a.K / 4; q += 64) reinterpret_cast<f32x4*>(trow)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const int64_t i = row0 + lr;
    const auto row_at = [x = a.x, ldx = a.ldx, ids = a.src_ids](int64_t j) { return x_row<KIND>(x, ldx, ids, j); };
    tconv_row_walk<HM>(a, a.W4, row_at, trow, i, rp[lr], rp[lr + 1], lane);
    if (a.Fd > 0 && lane < a.Fd / 4) {
      const int64_t self = a.self_rows[i];
      const float* xr = a.xd_ids ? x_row<KIND>(a.xd, a.ldxd, a.src_ids, self) : a.xd + self * a.ldxd;
      reinterpret_cast<f32x4*>(trow + a.H * a.W4)[lane] = reinterpret_cast<const f32x4*>(xr)[lane];
    }
  }
  __syncthreads();
  if (a.a_save) keep_tile_rows(tile, a.SD, a.K, rows_here, a.a_save, a.K, row0);   // A for the backward, row-major

  // ---- phase 2: [16 x K16] tile @ wt^T ----
  tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldwt, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows);
}

// ---- destination-major backward ---------------------------------------------------------------------------------------------
struct tconv_bwd_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* x;
  int64_t ldx;
  int F;
  const void* src_ids;
  const float* ea;
  int D;
  int H, W4;
  const float* alpha;         // [E, H]
  const float* dA;            // [n_rows, ldda]
  int64_t ldda;
  const float* A;             // [n_rows, lda]: the forward's saved rows
  int64_t lda;
  float* du;                  // [n_rows, H F]
  float* dw;                  // [n_rows, H D] (D > 0)
  float* ds;                  // [E, H]
};

template <int KIND, int HM>
__global__ void __launch_bounds__(256) tconv_bwd_dst_kernel(tconv_bwd_args a)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_rows) return;                      // (wave-uniform)
  const int F4 = a.F / 4, H = a.H, D = a.D;
  const bool fx = lane < F4;
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  f32x4 dah[HM], gu[HM];
  float dae[HM], gw[HM], rdot[HM];
#pragma unroll
  for (int h = 0; h < HM; ++h) {
    dah[h] = gu[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    dae[h] = gw[h] = rdot[h] = 0.f;
    if (h < H) {
      const float* dr = a.dA + i * a.ldda + (int64_t)h * a.W4;
      const float* ar = a.A + i * a.lda + (int64_t)h * a.W4;
      float p = 0.f;
      if (fx) {
        dah[h] = reinterpret_cast<const f32x4*>(dr)[lane];
        p = dot4(dah[h], reinterpret_cast<const f32x4*>(ar)[lane]);
      }
      if (lane <= D) {
        dae[h] = dr[a.F + lane];
        p += dae[h] * ar[a.F + lane];
      }
      rdot[h] = wave_sum(p);                      // sum_j alpha dalpha = dA_ih . agg_ih
    }
  }
  for (int e0 = s; e0 < t; e0 += 4) {
    f32x4 xv[4];
    float av[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int e = e0 + v;
      xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      av[v] = 0.f;
      if (e < t) {
        const int j = a.col[e];
        if (fx) xv[v] = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j))[lane];
        av[v] = lane < D ? a.ea[(int64_t)e * D + lane] : (lane == D ? 1.f : 0.f);
      }
    }
#pragma unroll
    for (int h = 0; h < HM; ++h) {
      if (h >= H) break;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float dal = wave_sum(dot4(dah[h], xv[v]) + dae[h] * av[v]);
        if (e0 + v < t) {
          const int64_t eh = (int64_t)(e0 + v) * H + h;
          const float dsv = a.alpha[eh] * (dal - rdot[h]);
          gu[h] += dsv * xv[v];
          gw[h] += dsv * av[v];
          if (lane == v) a.ds[eh] = dsv;
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < HM; ++h) {
    if (h >= H) break;
    if (fx) reinterpret_cast<f32x4*>(a.du + i * ((int64_t)H * a.F) + (int64_t)h * a.F)[lane] = gu[h];
    if (lane < D) a.dw[i * ((int64_t)H * D) + h * D + lane] = gw[h];
  }
}

// ---- source-major backward: the input rows' gradient -----------------------------------------------------------------------
__global__ void __launch_bounds__(256) tconv_bwd_src_kernel(const int* __restrict__ row_ptr_t, const int* __restrict__ col_t,
                                                            const int* __restrict__ perm, const int64_t* __restrict__ self_t,
                                                            int64_t n_rows, int64_t n_src, int F, int H, int W4, int skip_at,
                                                            const float* __restrict__ alpha, const float* __restrict__ ds,
                                                            const float* __restrict__ dA, int64_t ldda, const float* __restrict__ u,
                                                            int64_t ldu, float* __restrict__ gx, int64_t ldgx, int accumulate)
{
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n_src || lane >= F / 4) return;
  const int s = row_ptr_t[j], t = row_ptr_t[j + 1];
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  for (int p = s; p < t; ++p) {
    const int64_t i = col_t[p], e = perm[p];
    for (int h = 0; h < H; ++h) {
      const float al = alpha[e * H + h], dv = ds[e * H + h];
      const f32x4 d  = reinterpret_cast<const f32x4*>(dA + i * ldda + (int64_t)h * W4)[lane];
      const f32x4 uu = reinterpret_cast<const f32x4*>(u + i * ldu + (int64_t)h * F)[lane];
      g += al * d + dv * uu;
    }
  }
  if (self_t && skip_at >= 0) {                   // self_t[j] = n_rows + i (input row j is destination i), else 2 n_rows
    const int64_t i = self_t[j] - n_rows;
    if (i >= 0 && i < n_rows) g += reinterpret_cast<const f32x4*>(dA + i * ldda + skip_at)[lane];
  }
  f32x4* o = reinterpret_cast<f32x4*>(gx + j * ldgx) + lane;
  *o = accumulate ? *o + g : g;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_transformer_layer_supported(int F_src, int F_dst, int D, int H, int N)
{
  using namespace wgamd;
  if (F_src <= 0 || F_src % 4 != 0 || F_src > kMaxF || F_dst < 0 || F_dst % 4 != 0 || F_dst > kMaxF) return 0;
  if (D < 0 || D > kMaxD || H < 1 || H > kMaxH || N < 1 || N > 256) return 0;
  const int64_t K = (int64_t)H * block_width(F_src, D) + F_dst;
  return K <= kMaxK;
}

extern "C" int wgamd_transformer_block_width(int F_src, int D) { return wgamd::block_width(F_src, D); }

extern "C" wholememory_error_code_t wgamd_transformer_layer_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F_src, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const float* x_dst, int64_t ldx_dst, int F_dst, const int64_t* self_rows, int x_dst_ids,
    const float* edge_attr, int D, const float* u, int64_t ldu, const float* w, int64_t ldw, int H, const float* wt, int64_t ldwt,
    int N, const float* bias, int relu, float* out, int64_t ldo, float* alpha, float* a_save, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_transformer_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    if (!wgamd_transformer_layer_supported(F_src, F_dst, D, H, N))
      throw logic_error(fmt("unsupported shape: F_src=%d, F_dst=%d (multiples of 4, <= %d), D=%d (<= %d), H=%d (<= %d), N=%d "
                            "(<= 256), K <= %d", F_src, F_dst, kMaxF, D, kMaxD, H, kMaxH, N, kMaxK));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && u && wt && out && (D == 0 || (edge_attr && w)) && (F_dst == 0 || (x_dst && self_rows)),
                     "null pointer");
    WG_REQUIRE_INPUT(ldo >= N && ldu >= (int64_t)H * F_src && (D == 0 || ldw >= (int64_t)H * D), "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(!x_dst_ids || kind != 0, "x_dst_ids needs src_ids");
    tconv_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F_src, a.src_ids = src_ids;
    a.xd = x_dst, a.ldxd = ldx_dst, a.Fd = F_dst, a.self_rows = self_rows, a.xd_ids = x_dst_ids ? 1 : 0;
    a.edge_attr = edge_attr, a.D = D, a.u = u, a.ldu = ldu, a.w = w, a.ldw = ldw, a.H = H;
    a.wt = wt, a.ldwt = ldwt, a.N = N, a.bias = bias, a.relu = relu ? 1 : 0, a.out = out, a.ldo = ldo;
    a.alpha = alpha, a.a_save = a_save;
    a.W4  = block_width(F_src, D);
    a.K   = H * a.W4 + F_dst;
    a.K16 = (a.K + 15) / 16 * 16;
    a.SD  = a.K16 + 4;      // rows 4 banks apart: the 16 rows of a fragment read spread over the 64 banks
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F_src, "leading dimension too small");
    WG_REQUIRE_INPUT(F_dst == 0 || (x_dst_ids && kind == 3) || ldx_dst >= F_dst, "leading dimension too small");
    WG_REQUIRE_INPUT(ldwt >= a.K, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || (F_dst > 0 && !aligned_rows(x_dst, ldx_dst)) || !aligned_rows(wt, ldwt) ||
        !aligned_rows(u, ldu) || (a_save && !aligned_rows(a_save, 0)))
      throw logic_error("x / x_dst / u / wt / a_save rows must be 16-B aligned");
    with_kind(kind, [&](auto k) {
      with_heads(H, [&](auto hm) {
        launch_tiles(tconv_layer_kernel<decltype(k)::value, decltype(hm)::value>, a, static_cast<hipStream_t>(stream));
      });
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_transformer_bwd_dst_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F_src, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const float* edge_attr, int D, int H, const float* alpha, const float* dA, int64_t ldda,
    const float* A, int64_t lda, float* du, float* dw, float* ds, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_transformer_bwd_dst_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    if (!wgamd_transformer_layer_supported(F_src, 0, D, H, 1))
      throw logic_error(fmt("unsupported shape: F_src=%d, D=%d, H=%d", F_src, D, H));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && alpha && dA && A && du && ds && (D == 0 || (edge_attr && dw)), "null pointer");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    tconv_bwd_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.x = x, a.ldx = ldx, a.F = F_src, a.src_ids = src_ids;
    a.ea = edge_attr, a.D = D, a.H = H, a.W4 = block_width(F_src, D), a.alpha = alpha, a.dA = dA, a.ldda = ldda, a.A = A, a.lda = lda;
    a.du = du, a.dw = dw, a.ds = ds;
    WG_REQUIRE_INPUT(ldda >= (int64_t)H * a.W4 && lda >= (int64_t)H * a.W4, "leading dimension too small");
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F_src, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(dA, ldda) || !aligned_rows(A, lda) || !aligned_rows(du, 0))
      throw logic_error("x / dA / A / du rows must be 16-B aligned");
    const dim3 grid((unsigned)((n_rows + 3) / 4));
    with_kind(kind, [&](auto k) {
      with_heads(H, [&](auto hm) {
        tconv_bwd_dst_kernel<decltype(k)::value, decltype(hm)::value><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
      });
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_transformer_bwd_src_f32(
    const int* row_ptr_t, const int* col_t, const int* perm, const int64_t* self_t, int64_t n_rows, int64_t n_src, int F_src, int D,
    int H, int skip_at, const float* alpha, const float* ds, const float* dA, int64_t ldda, const float* u, int64_t ldu, float* gx,
    int64_t ldgx, int accumulate, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_transformer_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0 && n_rows >= 0, "bad sizes");
    if (!wgamd_transformer_layer_supported(F_src, 0, D, H, 1))
      throw logic_error(fmt("unsupported shape: F_src=%d, D=%d, H=%d", F_src, D, H));
    if (n_src == 0) return;
    WG_REQUIRE_INPUT(row_ptr_t && col_t && perm && alpha && ds && dA && u && gx, "null pointer");
    const int W4 = wgamd::block_width(F_src, D);
    WG_REQUIRE_INPUT(ldda >= (int64_t)H * W4 && ldu >= (int64_t)H * F_src && ldgx >= F_src, "leading dimension too small");
    WG_REQUIRE_INPUT(skip_at < 0 || (skip_at % 4 == 0 && ldda >= (int64_t)skip_at + F_src), "bad skip offset");
    if (!aligned_rows(dA, ldda) || !aligned_rows(u, ldu) || !aligned_rows(gx, ldgx))
      throw logic_error("dA / u / gx rows must be 16-B aligned");
    auto st = static_cast<hipStream_t>(stream);
    wgamd::tconv_bwd_src_kernel<<<(unsigned)((n_src + 3) / 4), 256, 0, st>>>(row_ptr_t, col_t, perm, self_t, n_rows, n_src, F_src, H,
                                                                              W4, skip_at, alpha, ds, dA, ldda, u, ldu, gx, ldgx,
                                                                              accumulate ? 1 : 0);
    WG_HIP_CHECK(hipGetLastError());
  });
}
