// Heterogeneous graph transformer layer (torch_geometric.nn.HeteroConv({edge type: TransformerConv}, aggr="sum"), what
// to_hetero makes of the encoder of the reference's cugraph-pyg example mag_lp_mnmg.py) over one (hop, destination type) of a
// call group.  The softmax is per relation, the sum over the relations ending in the type is linear, so the relations' rows sit
// side by side in ONE tile and meet ONE stacked weight:
//     A[i]   = [ blk^{r_1}_0 | ... | blk^{r_1}_{H_1 - 1} | blk^{r_2}_0 | ... | XD[dst_rows[i]] ]     K = sum_r H_r W4_r + F_dst
//     blk^r_h = sum_{e in row i of r} alpha^r_eh [ X_r[col_r[e]] | a^r_e | 1 | 0 pad ],    W4_r = ceil4(F_r + D_r + 1)
//     alpha^r = softmax over the edges of row i of relation r of  u^r_ih . X_r[j] + w^r_ih . a^r_e        (wg_transformer.hip)
//     out[p] = act( A[i] @ wt^T + bias + acc_in[i] ),  p = out_rows ? out_rows[i] : i
// with wt = [ Wstack^{r_1} | Wstack^{r_2} | ... | sum_r lin_skip^r ] ([N, K]) and bias = sum_r b_skip^r built by the host.  Every
// relation has its own CSR over the same n_rows frontier entries, its own input rows (X_r[j] = x_r[ids_r ? ids_r[j] : j], the
// kind of the node list chosen per relation at run time), its own u^r, w^r, edge attributes and F_r, D_r, H_r.  A row without
// edges in a relation leaves that relation's blocks exactly zero: no message and no value bias come from it.
//
// hetero_tconv_kernel — one workgroup of 256 threads per 16-row tile, one wave per destination row (as tconv_layer_kernel).
// Phase 1: for every relation in turn the wave walks the relation's edges of its row exactly as tconv_layer_kernel's phase 1
// does — lane = one float4 of the source row and, for lane <= D, one column of [a | 1]; groups of 4 edges; wave sums by xor
// butterflies; an online softmax (running max and sum per head, accumulators rescaled once per group); the logits go to
// alpha^r [E_r, H_r] as they are made and become alpha in a second pass over the row — and writes the relation's H_r blocks at
// col0_r of the row's LDS tile; the root block follows, read through dst_ids for a lazy destination type.  (The row walk is
// tconv_row_walk of wg_transformer_parts.hpp, the one tconv_layer_kernel runs, here with run-time node-list kinds.)  Phase 2:
// tile_times_wt (wg_layer_parts.hpp) with the running sum of an earlier launch, bias, ReLU and the row placement.
// No atomics: every sum runs in CSR order, the same bits from run to run.
#include "wg_transformer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kMaxRel = WGAMD_HETERO_TRANSFORMER_MAX_RELATIONS;

struct htconv_args : hetero_frame {             // (kept = a_save: the A rows)
  wgamd_hetero_transformer_relation_t rel[kMaxRel];
};

template <int HM>
__global__ void __launch_bounds__(kThreads) hetero_tconv_kernel(htconv_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int rp[kMaxRel][kTileRows + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
  load_row_windows(rp, a.rel, a.n_rel, row0, rows_here);
  zero_tile_padding(tile, a.SD, a.K, a.K16);
  __syncthreads();

  // ---- phase 1: one wave per destination row, the relations in turn ----
  for (int lr = wave; lr < kTileRows; lr += 4) {
    float* trow = tile + lr * a.SD;
    if (lr >= rows_here) {
      for (int q = lane; q < a.K / 4; q += 64) reinterpret_cast<f32x4*>(trow)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const int64_t i = row0 + lr;
    for (int r = 0; r < a.n_rel; ++r) {
      const wgamd_hetero_transformer_relation_t& R = a.rel[r];
      const auto row_at = [x = R.x, ldx = R.ldx, ids = R.src_ids, kind = R.ids_kind](int64_t j) { return row_of(x, ldx, ids, kind, j); };
      tconv_row_walk<HM>(R, block_width(R.F, R.D), row_at, trow + R.col0, i, rp[r][lr], rp[r][lr + 1], lane);
    }
    if (a.x_dst != nullptr && lane < a.F_dst / 4) {
      const int64_t self = a.dst_rows ? a.dst_rows[i] : i;
      reinterpret_cast<f32x4*>(trow + a.root_col0)[lane] =
        reinterpret_cast<const f32x4*>(row_of(a.x_dst, a.ldx_dst, a.dst_ids, a.dst_kind, self))[lane];
    }
  }
  __syncthreads();
  if (a.kept) keep_tile_rows(tile, a.SD, a.K, rows_here, a.kept, a.ld_kept, row0);   // A for the backward

  // ---- phase 2: [16 x K16] tile @ wt^T ----
  tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldw, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows, a.acc_in, a.ld_acc,
                a.out_rows);
}

int64_t total_k(const int* F, const int* D, const int* H, int n_rel, int F_dst)
{
  int64_t K = F_dst;
  for (int r = 0; r < n_rel; ++r) K += (int64_t)H[r] * block_width(F[r], D[r]);
  return K;
}

wholememory_error_code_t launch(const char* what, const wgamd_hetero_transformer_relation_t* rels, int n_rel, int64_t n_rows,
                                const float* x_dst, int64_t ldx_dst, int F_dst, const int64_t* dst_rows, const void* dst_ids,
                                int dst_ids_kind, const float* wt, int64_t ldw, int N, const float* bias, int flags,
                                const float* acc_in, int64_t ld_acc, const int64_t* out_rows, float* out, int64_t ldo, float* a_save,
                                int64_t lda, void* stream)
{
  return guarded(what, [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && n_rel >= 0 && n_rel <= kMaxRel && F_dst >= 0, "bad sizes");
    WG_REQUIRE_INPUT(n_rel == 0 || rels != nullptr, "null pointer");
    int Fs[kMaxRel], Ds[kMaxRel], Hs[kMaxRel];
    for (int r = 0; r < n_rel; ++r) Fs[r] = rels[r].F, Ds[r] = rels[r].D, Hs[r] = rels[r].H;
    if (!wgamd_hetero_transformer_layer_supported(Fs, Ds, Hs, n_rel, x_dst ? F_dst : 0, N))
      throw logic_error(fmt("unsupported shape: every F and F_dst a multiple of 4 and <= %d, D <= %d, H <= %d, N=%d (<= 256), "
                            "K=%lld (in (0, %d])", kMaxF, kMaxD, kMaxH, N,
                            (long long)total_k(Fs, Ds, Hs, n_rel, x_dst ? F_dst : 0), kMaxK));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(wt && out, "null pointer");
    htconv_args a{};
    int at = 0, h_max = 1;
    for (int r = 0; r < n_rel; ++r) {
      const wgamd_hetero_transformer_relation_t& R = rels[r];
      WG_REQUIRE_INPUT(R.row_ptr && R.col && R.x && R.u && (R.D == 0 || (R.edge_attr && R.w)), "null pointer");
      WG_REQUIRE_INPUT(R.ids_kind >= 0 && R.ids_kind <= 2 && (R.ids_kind == 0) == (R.src_ids == nullptr), "bad node list kind");
      WG_REQUIRE_INPUT(R.ldx >= R.F && R.ldu >= (int64_t)R.H * R.F && (R.D == 0 || R.ldw >= (int64_t)R.H * R.D),
                       "leading dimension too small");
      WG_REQUIRE_INPUT(R.col0 == at, "relation blocks must be back to back from column 0");
      if (!aligned_rows(R.x, R.ldx) || !aligned_rows(R.u, R.ldu)) throw logic_error("x / u rows must be 16-B aligned");
      a.rel[r] = R;
      at += R.H * block_width(R.F, R.D);
      h_max = std::max(h_max, R.H);
    }
    fill_hetero_frame(a, n_rel, n_rows, at, x_dst, ldx_dst, F_dst, dst_rows, dst_ids, dst_ids_kind, wt, ldw, N, bias,
                      flags & WGAMD_HETERO_TRANSFORMER_RELU, acc_in, ld_acc, out_rows, out, ldo, a_save, lda,
                      "a_save rows must be 16-B aligned, lda >= K");
    with_heads(h_max, [&](auto hm) {
      launch_tiles(hetero_tconv_kernel<decltype(hm)::value>, a, static_cast<hipStream_t>(stream));
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_hetero_transformer_layer_supported(const int* F, const int* D, const int* H, int n_rel, int F_dst, int N)
{
  using namespace wgamd;
  if (n_rel < 0 || n_rel > kMaxRel || F_dst < 0 || F_dst % 4 != 0 || F_dst > kMaxF || N <= 0 || N > 256) return 0;
  for (int r = 0; r < n_rel; ++r)
    if (F[r] <= 0 || F[r] % 4 != 0 || F[r] > kMaxF || D[r] < 0 || D[r] > kMaxD || H[r] < 1 || H[r] > kMaxH) return 0;
  const int64_t K = total_k(F, D, H, n_rel, F_dst);
  return K > 0 && K <= kMaxK;
}

extern "C" wholememory_error_code_t wgamd_hetero_transformer_layer_f32(
    const wgamd_hetero_transformer_relation_t* rels, int n_rel, int64_t n_rows, const float* x_dst, int64_t ldx_dst, int F_dst,
    const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind, const float* wt, int64_t ldw, int N, const float* bias, int flags,
    const float* acc_in, int64_t ld_acc, const int64_t* out_rows, float* out, int64_t ldo, void* stream)
{
  return wgamd::launch("wgamd_hetero_transformer_layer_f32", rels, n_rel, n_rows, x_dst, ldx_dst, F_dst, dst_rows, dst_ids,
                       dst_ids_kind, wt, ldw, N, bias, flags, acc_in, ld_acc, out_rows, out, ldo, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_hetero_transformer_layer_f32_train(
    const wgamd_hetero_transformer_relation_t* rels, int n_rel, int64_t n_rows, const float* x_dst, int64_t ldx_dst, int F_dst,
    const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind, const float* wt, int64_t ldw, int N, const float* bias, int flags,
    const float* acc_in, int64_t ld_acc, const int64_t* out_rows, float* out, int64_t ldo, float* a_save, int64_t lda, void* stream)
{
  if (a_save == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  for (int r = 0; r < n_rel && rels != nullptr; ++r)
    if (rels[r].alpha == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  return wgamd::launch("wgamd_hetero_transformer_layer_f32_train", rels, n_rel, n_rows, x_dst, ldx_dst, F_dst, dst_rows, dst_ids,
                       dst_ids_kind, wt, ldw, N, bias, flags, acc_in, ld_acc, out_rows, out, ldo, a_save, lda, stream);
}
