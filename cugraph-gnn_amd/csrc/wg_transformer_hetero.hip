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
// col0_r of the row's LDS tile; the root block follows, read through dst_ids for a lazy destination type.  (The row walk is a
// copy of wg_transformer.hip's with run-time node-list kinds; the two are to be folded into one header.)  Phase 2:
// tile_times_wt (wg_layer_parts.hpp) with the running sum of an earlier launch, bias, ReLU and the row placement.
// No atomics: every sum runs in CSR order, the same bits from run to run.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kMaxK   = 1024;
constexpr int kMaxF   = 256;     // one float4 of a source row per lane
constexpr int kMaxD   = 32;      // [a | 1 | pad] within one wave's lanes
constexpr int kMaxH   = 8;
constexpr int kMaxRel = WGAMD_HETERO_TRANSFORMER_MAX_RELATIONS;

// sum over the wave; xor butterflies give every lane the same bits (each step adds the same two values, commuted)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// a row read through a node list whose kind is known at run time only (0 = by row, 1 = int32, 2 = int64)
__device__ __forceinline__ const float* row_of(const float* x, int64_t ldx, const void* ids, int kind, int64_t r)
{
  if (kind == 1) r = static_cast<const int32_t*>(ids)[r];
  else if (kind == 2) r = static_cast<const int64_t*>(ids)[r];
  return x + r * ldx;
}

struct htconv_args {
  wgamd_hetero_transformer_relation_t rel[kMaxRel];
  int n_rel;
  int64_t n_rows;
  const float* x_dst;         // the skip block: null = none
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
  float* a_save;              // _train: the A rows
  int64_t lda;
  int K, K16, SD;
};

// One relation's blocks of one destination row: the edges [s, t) of the relation's CSR row i -> blk[h W4 + :] for h < H.
template <int HM>
__device__ __forceinline__ void relation_row(const wgamd_hetero_transformer_relation_t& R, float* blk, int64_t i, int s, int t,
                                             int lane)
{
  const int F = R.F, F4 = F / 4, H = R.H, D = R.D;
  const int W4 = (F + D + 1 + 3) / 4 * 4;
  const bool fx = lane < F4;
  const int ext_w = W4 - F;                       // [a | 1 | pad] columns of a head block
  f32x4 uh[HM], acc[HM];
  float wh[HM], ext[HM], m[HM], l[HM];
#pragma unroll
  for (int h = 0; h < HM; ++h) {
    uh[h] = acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    wh[h] = ext[h] = l[h] = 0.f;
    m[h] = -INFINITY;
    if (h < H && s < t) {
      if (fx) uh[h] = reinterpret_cast<const f32x4*>(R.u + i * R.ldu + (int64_t)h * F)[lane];
      if (lane < D) wh[h] = R.w[i * R.ldw + h * D + lane];
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
        const int j = R.col[e];
        if (fx) xv[v] = reinterpret_cast<const f32x4*>(row_of(R.x, R.ldx, R.src_ids, R.ids_kind, j))[lane];
        av[v] = lane < D ? R.edge_attr[(int64_t)e * D + lane] : (lane == D ? 1.f : 0.f);
      }
    }
#pragma unroll
    for (int h = 0; h < HM; ++h) {
      if (h >= H) break;
      float sc[4];
      float mx = m[h];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        sc[v] = wave_sum(dot4(uh[h], xv[v]) + (lane < D ? wh[h] * av[v] : 0.f));
        if (e0 + v < t) mx = fmaxf(mx, sc[v]);
      }
      const float r = expf(m[h] - mx);            // (m = -inf before the first group: r = 0)
      acc[h] *= r;
      ext[h] *= r;
      l[h] *= r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (e0 + v < t) {
          const float p = expf(sc[v] - mx);
          acc[h] += p * xv[v];
          ext[h] += p * av[v];
          l[h] += p;
          if (R.alpha && lane == v) R.alpha[(int64_t)(e0 + v) * H + h] = sc[v];   // the logit; alpha after the row
        }
      }
      m[h] = mx;
    }
  }
#pragma unroll
  for (int h = 0; h < HM; ++h) {
    if (h >= H) break;
    const float inv = l[h] > 0.f ? 1.f / l[h] : 0.f;          // (no edges: acc = ext = 0 and inv = 0 — the block is exactly zero)
    if (fx) reinterpret_cast<f32x4*>(blk + h * W4)[lane] = acc[h] * inv;
    if (lane < ext_w) blk[h * W4 + F + lane] = ext[h] * inv;
    l[h] = inv;
  }
  if (R.alpha && s < t) {
    __threadfence_block();                        // the logits this wave wrote, read back by other lanes
    for (int e = s + lane; e < t; e += 64)
#pragma unroll
      for (int h = 0; h < HM; ++h) {
        if (h >= H) break;
        float* p = R.alpha + (int64_t)e * H + h;
        *p = expf(*p - m[h]) * l[h];
      }
  }
}

template <int HM>
__global__ void __launch_bounds__(kThreads) hetero_tconv_kernel(htconv_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int rp[kMaxRel][kTileRows + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
  if (tid < a.n_rel * (kTileRows + 1)) {
    const int r = tid / (kTileRows + 1), t = tid % (kTileRows + 1);
    rp[r][t] = a.rel[r].row_ptr[row0 + std::min(t, rows_here)];
  }
  const int pad4 = (a.K16 - a.K) / 4;             // the tile's k padding [K, K16) is zero
  for (int p = tid; p < kTileRows * pad4; p += kThreads)
    reinterpret_cast<f32x4*>(tile + (p / pad4) * a.SD + a.K)[p % pad4] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  // ---- phase 1: one wave per destination row, the relations in turn ----
  for (int lr = wave; lr < kTileRows; lr += 4) {
    float* trow = tile + lr * a.SD;
    if (lr >= rows_here) {
      for (int q = lane; q < a.K / 4; q += 64) reinterpret_cast<f32x4*>(trow)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const int64_t i = row0 + lr;
    for (int r = 0; r < a.n_rel; ++r) relation_row<HM>(a.rel[r], trow + a.rel[r].col0, i, rp[r][lr], rp[r][lr + 1], lane);
    if (a.x_dst != nullptr && lane < a.F_dst / 4) {
      const int64_t self = a.dst_rows ? a.dst_rows[i] : i;
      reinterpret_cast<f32x4*>(trow + a.root_col0)[lane] =
        reinterpret_cast<const f32x4*>(row_of(a.x_dst, a.ldx_dst, a.dst_ids, a.dst_kind, self))[lane];
    }
  }
  __syncthreads();
  if (a.a_save) {                                 // A for the backward: rows_here x K, rows lda apart
    const int K4 = a.K / 4;
    for (int p = tid; p < rows_here * K4; p += kThreads)
      reinterpret_cast<f32x4*>(a.a_save + (row0 + p / K4) * a.lda)[p % K4] = reinterpret_cast<const f32x4*>(tile + (p / K4) * a.SD)[p % K4];
  }

  // ---- phase 2: [16 x K16] tile @ wt^T ----
  tile_times_wt(tile, a.SD, a.K, a.K16, a.wt, a.ldw, a.N, a.bias, a.relu, a.out, a.ldo, row0, a.n_rows, a.acc_in, a.ld_acc,
                a.out_rows);
}

int block_width(int F, int D) { return (F + D + 1 + 3) / 4 * 4; }

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
    a.n_rel = n_rel, a.n_rows = n_rows;
    if (x_dst) {
      WG_REQUIRE_INPUT(F_dst > 0 && ldx_dst >= F_dst, "leading dimension too small");
      WG_REQUIRE_INPUT(dst_ids_kind >= 0 && dst_ids_kind <= 2 && (dst_ids_kind == 0) == (dst_ids == nullptr), "bad node list kind");
      if (!aligned_rows(x_dst, ldx_dst)) throw logic_error("x_dst rows must be 16-B aligned");
      a.x_dst = x_dst, a.ldx_dst = ldx_dst, a.F_dst = F_dst, a.dst_rows = dst_rows, a.dst_ids = dst_ids, a.dst_kind = dst_ids_kind;
      a.root_col0 = at;
      at += F_dst;
    }
    a.wt = wt, a.ldw = ldw, a.N = N, a.bias = bias, a.relu = (flags & WGAMD_HETERO_TRANSFORMER_RELU) ? 1 : 0;
    a.acc_in = acc_in, a.ld_acc = ld_acc, a.out_rows = out_rows, a.out = out, a.ldo = ldo, a.a_save = a_save, a.lda = lda;
    a.K   = at;
    a.K16 = (a.K + 15) / 16 * 16;
    a.SD  = a.K16 + 4;      // rows 4 banks apart: the 16 rows of a fragment read spread over the 64 banks
    WG_REQUIRE_INPUT(ldw >= a.K && ldo >= N && (acc_in == nullptr || ld_acc >= N), "leading dimension too small");
    if (!aligned_rows(wt, ldw)) throw logic_error("wt rows must be 16-B aligned");
    if (a_save != nullptr && (lda < a.K || !aligned_rows(a_save, lda))) throw logic_error("a_save rows must be 16-B aligned, lda >= K");
    auto st = static_cast<hipStream_t>(stream);
    if (h_max <= 1) launch_tiles(hetero_tconv_kernel<1>, a, st);
    else if (h_max <= 2) launch_tiles(hetero_tconv_kernel<2>, a, st);
    else if (h_max <= 4) launch_tiles(hetero_tconv_kernel<4>, a, st);
    else launch_tiles(hetero_tconv_kernel<8>, a, st);
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
