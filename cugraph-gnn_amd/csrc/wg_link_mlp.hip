// The MLP edge decoder of link prediction (include/wgamd_ext.h: wgamd_pair_mlp_*): the EdgeDecoder of the reference's
// cugraph_pyg/examples/movielens_mnmg.py and taobao_mnmg.py,
//   a_p = [x_src[i_p] | x_dst[j_p]]          K = C_src + C_dst
//   h_p = relu(a_p W1^T + b1)                W1 [H, K]
//   s_p = h_p . w2 + b2                      w2 [H], b2 ONE float on the device
// and, with labels, the binary cross-entropy of wg_link.hip over s_p (loss, c_p = w_p (sigmoid(s_p) - y_p), the sum of weights).
//   * pair_mlp_fwd_kernel — ONE launch.  A workgroup takes 16-pair tiles (tile t, t + grid, ...: the grid is bounded so that one
//     BCE state serves every call).  Phase 1: the 16 index pairs, checked against their tables, then the two rows of every pair
//     side by side into LDS tile A [16][K16 + 4] as float4 (columns [K, K16) and the rows of absent or out-of-range pairs zero):
//     no [P, .] copy of the inputs reaches memory.  Phase 2: tile A times W1^T with b1 and ReLU (tile_times_wt: fp32 MFMA) into
//     LDS tile B, and into hidden_out when the caller keeps it for the backward.  Phase 3: 16 lanes per row, row . w2 by a
//     shuffle tree of fixed shape, + b2; then the BCE term of the pair.  The loss partials are added by the last workgroup in
//     workgroup order (bce_finish).
//   * pair_mlp_bwd_kernel — ONE launch over the kept hidden [P, H]: overwrites it with dZ_p = g_p w2 * [h_p > 0] and forms
//     dw2 = sum_p g_p h_p, db2 = sum_p g_p from per-workgroup partials added in workgroup order by the last workgroup.  No float
//     atomics: the same bits from run to run.  The sums over a row's incident pairs and the products with W1 / the tables are
//     existing entry points (wgamd_pair_grad_f32, wgamd_gcn_wgrad_f32) and library GEMMs.
// A pair with an index outside its table reads nothing: its score is NaN, its coefficient 0, its hidden_out row 0, and it adds
// nothing to any gradient.
#include "wg_layer_parts.hpp"
#include "wg_link_parts.hpp"

namespace wgamd {
namespace {

static_assert(kThreads == kLinkThreads && kTileRows * 16 == kThreads, "16 rows x 16 lanes in phase 3");

constexpr int kMlpMaxK      = 1024;
constexpr int kMlpMaxH      = 256;   // four waves x four 16-column tiles of tile_times_wt
constexpr int kMlpBwdGrid   = 512;
constexpr int kMlpCopyAhead = 4;     // float4 row reads a thread has in flight in phase 1
constexpr int kMlpRowsAhead = 8;     // hidden rows a row group of the backward has in flight

struct mlp_args {
  const float* xs;
  int64_t lds, n_src;
  const float* xd;
  int64_t ldd, n_dst;
  int Cs, Cd;
  const int64_t* isrc;
  const int64_t* idst;
  int64_t P;
  const float* w1;            // [H, ldw1] row-major
  int64_t ldw1;
  int H;
  const float* b1;            // nullable
  const float* w2;            // [H]
  const float* b2;            // nullable: ONE float on the device
  const float* label;         // BCE only
  const float* weight;        // nullable
  float* score;               // nullable with BCE
  float* coef;                // BCE: [P + 1]
  float* state;
  float* loss_out;
  int mean;
  float* hidden_out;          // nullable; [P, ld_hidden], columns [0, H rounded up to 4) written
  int64_t ld_hidden;
  int K, K16, SD;             // tile A: C_src + C_dst, rounded up to 16, floats per row
  int H16, SH;                // tile B
};

template <bool BCE>
__global__ void __launch_bounds__(kThreads) pair_mlp_fwd_kernel(mlp_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int64_t s_i[kTileRows], s_j[kTileRows];     // the tile's rows of the two tables; s_i < 0: the pair reads nothing
  float* hid = tile + kTileRows * a.SD;
  const int tid = threadIdx.x;
  const int64_t n_tiles = (a.P + kTileRows - 1) / kTileRows;
  const int K4 = a.K16 / 4, Cs4 = a.Cs / 4, Kq = a.K / 4, Hq = (a.H + 3) / 4;
  const float b2 = a.b2 ? *a.b2 : 0.f;
  float loss = 0.f, wsum = 0.f;

  // (the loop bound is the workgroup's: every thread reaches the barriers)
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t p0 = t * kTileRows;
    __syncthreads();                                     // the last tile's phase 3 is done with s_i and tile B
    // ---- phase 1: the index pairs, then the rows side by side -> LDS tile A ----
    if (tid < kTileRows) {
      const bool live = p0 + tid < a.P;
      const int64_t i = live ? a.isrc[p0 + tid] : -1, j = live ? a.idst[p0 + tid] : -1;
      const bool ok = i >= 0 && i < a.n_src && j >= 0 && j < a.n_dst;
      s_i[tid] = ok ? i : -1;
      s_j[tid] = ok ? j : -1;
    }
    __syncthreads();
    for (int e0 = tid; e0 < kTileRows * K4; e0 += kThreads * kMlpCopyAhead) {
      f32x4 v[kMlpCopyAhead];
#pragma unroll
      for (int u = 0; u < kMlpCopyAhead; ++u) {
        const int e = e0 + u * kThreads;
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < kTileRows * K4) {
          const int r = e / K4, q = e % K4;
          const int64_t i = s_i[r];
          if (i >= 0 && q < Kq)
            v[u] = q < Cs4 ? reinterpret_cast<const f32x4*>(a.xs + i * a.lds)[q]
                           : reinterpret_cast<const f32x4*>(a.xd + s_j[r] * a.ldd)[q - Cs4];
        }
      }
#pragma unroll
      for (int u = 0; u < kMlpCopyAhead; ++u) {
        const int e = e0 + u * kThreads;
        if (e < kTileRows * K4) reinterpret_cast<f32x4*>(tile + (e / K4) * a.SD)[e % K4] = v[u];
      }
    }
    for (int idx = tid; idx < kTileRows * (a.H16 - a.H); idx += kThreads) {
      const int r = idx / (a.H16 - a.H), n = a.H + idx % (a.H16 - a.H);
      hid[r * a.SH + n] = 0.f;
    }
    __syncthreads();

    // ---- phase 2: [16 x K16] tile A @ W1^T, b1, ReLU -> LDS tile B (all 16 rows: a row that read nothing holds relu(b1)) ----
    tile_times_wt(tile, a.SD, a.K, a.K16, a.w1, a.ldw1, a.H, a.b1, 1, hid, a.SH, 0, kTileRows);
    __syncthreads();
    if (a.hidden_out) {
      for (int idx = tid; idx < kTileRows * Hq; idx += kThreads) {
        const int r = idx / Hq, q = idx % Hq;
        if (p0 + r < a.P)
          reinterpret_cast<f32x4*>(a.hidden_out + (p0 + r) * a.ld_hidden)[q] =
            s_i[r] >= 0 ? reinterpret_cast<const f32x4*>(hid + r * a.SH)[q] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }

    // ---- phase 3: 16 lanes per row, hidden row . w2 + b2, then the pair's loss term ----
    const int r = tid >> 4, sub = tid & 15;
    float s = 0.f;
    for (int n = sub; n < a.H; n += 16) s += hid[r * a.SH + n] * a.w2[n];
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    const int64_t p = p0 + r;
    if (sub == 0 && p < a.P) {
      const bool good = s_i[r] >= 0;
      s = good ? s + b2 : __builtin_nanf("");
      if (a.score) a.score[p] = s;
      if constexpr (BCE) {
        const float w = a.weight ? a.weight[p] : 1.f;
        // (a pair that read nothing AND weighs nothing is masked out: its NaN stays out of the loss)
        a.coef[p] = good || w != 0.f ? bce_pair(s, good, a.label[p], w, loss, wsum) : 0.f;
      }
    }
  }
  if constexpr (BCE) bce_finish(loss, wsum, a.state, a.coef, a.P, a.loss_out, a.mean);
}

// workspace: [0] the ticket (as int), then per workgroup H + 1 floats (dw2, db2)
__global__ void __launch_bounds__(kThreads)
pair_mlp_bwd_kernel(float* __restrict__ hidden, int64_t ldh, int64_t P, int H, int lgh, const float* __restrict__ w2,
                    const float* __restrict__ g, const float* __restrict__ scale_num, const float* __restrict__ scale_den,
                    const int64_t* __restrict__ isrc, int64_t n_src, const int64_t* __restrict__ idst, int64_t n_dst,
                    int64_t rows_per_block, float* __restrict__ grad_w2, float* __restrict__ grad_b2, float* __restrict__ ws)
{
  __shared__ float s_w[kThreads], s_b[kThreads];
  __shared__ int s_last;
  const int tid = threadIdx.x, HB = 1 << lgh, n = tid & (HB - 1), grp = tid >> lgh, groups = kThreads >> lgh;
  const float scale = (scale_num ? *scale_num : 1.f) / (scale_den ? *scale_den : 1.f);
  const float w = n < H ? w2[n] : 0.f;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block, r_end = min(P, r_begin + rows_per_block);
  float dw = 0.f, db = 0.f;
  // (kMlpRowsAhead rows of the group in flight: a row costs two dependent round trips, index then hidden)
  for (int64_t p0 = r_begin + grp; p0 < r_end; p0 += (int64_t)groups * kMlpRowsAhead) {
    float gp[kMlpRowsAhead], h[kMlpRowsAhead];
#pragma unroll
    for (int u = 0; u < kMlpRowsAhead; ++u) {
      const int64_t p = p0 + (int64_t)u * groups;
      const bool live = p < r_end;
      const int64_t i = live ? isrc[p] : -1, j = live ? idst[p] : -1;
      const bool ok = i >= 0 && i < n_src && j >= 0 && j < n_dst;
      gp[u] = ok ? scale * g[p] : 0.f;            // (a pair that read nothing: whatever came down its NaN score is dropped)
      h[u]  = live && n < H ? hidden[p * ldh + n] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kMlpRowsAhead; ++u) {
      const int64_t p = p0 + (int64_t)u * groups;
      db += gp[u];
      dw += gp[u] * h[u];
      if (p < r_end && n < H) hidden[p * ldh + n] = h[u] > 0.f ? gp[u] * w : 0.f;
    }
  }
  // the row groups of the workgroup in group order, then the workgroups in workgroup order
  s_w[tid] = dw;
  s_b[tid] = db;
  __syncthreads();
  float* part = ws + 4 + (int64_t)blockIdx.x * (H + 1);
  if (grp == 0) {
    float sw = 0.f, sb = 0.f;
    for (int k = 0; k < groups; k++) sw += s_w[k * HB + n], sb += s_b[k * HB + n];
    if (n < H) part[n] = sw;
    if (n == 0) part[H] = sb;
  }
  __threadfence();
  __syncthreads();
  int* ticket = reinterpret_cast<int*>(ws);
  if (tid == 0) s_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  for (int c = tid; c <= H; c += kThreads) {
    float sum = 0.f;
#pragma unroll 8
    for (unsigned k = 0; k < gridDim.x; k++)
      sum += __hip_atomic_load(ws + 4 + (int64_t)k * (H + 1) + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c < H) {
      if (grad_w2) grad_w2[c] = sum;
    } else if (grad_b2) {
      *grad_b2 = sum;
    }
  }
  if (tid == 0) *ticket = 0;     // (the workspace is reusable without a memset)
}

inline int mlp_fwd_grid(int64_t P)
{
  return (int)std::max<int64_t>(1, std::min<int64_t>((P + kTileRows - 1) / kTileRows, kLinkMaxGrid));
}

}  // namespace
}  // namespace wgamd

extern "C" {

int wgamd_pair_mlp_supported(int c_src, int c_dst, int hidden)
{
  using namespace wgamd;
  return c_src > 0 && c_dst > 0 && c_src % 4 == 0 && c_dst % 4 == 0 && c_src <= kMlpMaxK && c_dst <= kMlpMaxK &&
         c_src + c_dst <= kMlpMaxK && hidden >= 1 && hidden <= kMlpMaxH;
}

wholememory_error_code_t wgamd_pair_mlp_forward_f32(const float* x_src, int64_t ld_src, int64_t n_src, const float* x_dst,
                                                    int64_t ld_dst, int64_t n_dst, int c_src, int c_dst, const int64_t* index_src,
                                                    const int64_t* index_dst, int64_t n_pairs, const float* w1, int64_t ldw1,
                                                    int hidden, const float* b1, const float* w2, const float* b2,
                                                    const float* label, const float* pair_weight, int mean, float* score,
                                                    float* coef, void* state, int state_is_zeroed, float* loss_out,
                                                    float* hidden_out, int64_t ld_hidden, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pair_mlp_forward_f32", [&] {
    WG_REQUIRE_INPUT(n_pairs >= 0 && n_src >= 0 && n_dst >= 0, "bad shape");
    if (!wgamd_pair_mlp_supported(c_src, c_dst, hidden))
      throw logic_error(fmt("unsupported shape: C_src=%d, C_dst=%d (multiples of 4, sum <= %d), H=%d (1..%d)", c_src, c_dst, kMlpMaxK,
                            hidden, kMlpMaxH));
    const bool bce = label != nullptr;
    WG_REQUIRE_INPUT(!bce || n_pairs >= 1, "the loss needs a pair");
    if (n_pairs == 0) return;
    const int K = c_src + c_dst, Hq = (hidden + 3) / 4 * 4;
    WG_REQUIRE_INPUT(ld_src >= c_src && ld_dst >= c_dst && ldw1 >= K && (hidden_out == nullptr || ld_hidden >= Hq),
                     "leading dimension too small");
    WG_REQUIRE_INPUT(index_src && index_dst && w1 && w2 && (x_src || n_src == 0) && (x_dst || n_dst == 0), "null pointer");
    WG_REQUIRE_INPUT(bce ? (coef && state && loss_out) : (score != nullptr), "null pointer");
    if (!aligned_rows(x_src, ld_src) || !aligned_rows(x_dst, ld_dst) || !aligned_rows(w1, ldw1) ||
        (hidden_out && !aligned_rows(hidden_out, ld_hidden)))
      throw logic_error("x_src / x_dst / w1 / hidden_out rows must be 16-B aligned");
    auto st = static_cast<hipStream_t>(stream);
    if (bce && !state_is_zeroed) WG_HIP_CHECK(hipMemsetAsync(state, 0, wgamd_pair_bce_state_bytes(n_pairs), st));
    mlp_args a{};
    a.xs = x_src, a.lds = ld_src, a.n_src = n_src, a.xd = x_dst, a.ldd = ld_dst, a.n_dst = n_dst, a.Cs = c_src, a.Cd = c_dst;
    a.isrc = index_src, a.idst = index_dst, a.P = n_pairs;
    a.w1 = w1, a.ldw1 = ldw1, a.H = hidden, a.b1 = b1, a.w2 = w2, a.b2 = b2;
    a.label = label, a.weight = pair_weight, a.score = score, a.coef = coef, a.state = static_cast<float*>(state);
    a.loss_out = loss_out, a.mean = mean, a.hidden_out = hidden_out, a.ld_hidden = ld_hidden;
    a.K = K, a.K16 = (K + 15) / 16 * 16, a.SD = a.K16 + 4;      // rows 4 banks apart, as every layer tile
    a.H16 = (hidden + 15) / 16 * 16, a.SH = a.H16 + 4;
    const size_t lds = (size_t)kTileRows * (a.SD + a.SH) * 4;   // at most 16 x (1028 + 260) floats = 82 KB: above the 64 KB default
    auto kern = bce ? pair_mlp_fwd_kernel<true> : pair_mlp_fwd_kernel<false>;
    WG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<mlp_fwd_grid(n_pairs), kThreads, lds, st>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

size_t wgamd_pair_mlp_backward_workspace_bytes(int hidden)
{
  (void)hidden;   // (one size for every call, so one workspace serves them all)
  return sizeof(float) * (size_t)(4 + wgamd::kMlpBwdGrid * (wgamd::kMlpMaxH + 1)) + 16;
}

wholememory_error_code_t wgamd_pair_mlp_backward_f32(float* hidden_io, int64_t ld_hidden, int64_t n_pairs, int hidden,
                                                     const float* w2, const float* g, const float* scale_num,
                                                     const float* scale_den, const int64_t* index_src, int64_t n_src,
                                                     const int64_t* index_dst, int64_t n_dst, float* grad_w2, float* grad_b2,
                                                     void* workspace, size_t workspace_bytes, int workspace_is_zeroed,
                                                     void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pair_mlp_backward_f32", [&] {
    WG_REQUIRE_INPUT(n_pairs >= 0 && n_src >= 0 && n_dst >= 0 && hidden >= 1 && hidden <= kMlpMaxH && ld_hidden >= hidden, "bad shape");
    auto st = static_cast<hipStream_t>(stream);
    if (n_pairs == 0) {
      if (grad_w2) WG_HIP_CHECK(hipMemsetAsync(grad_w2, 0, sizeof(float) * (size_t)hidden, st));
      if (grad_b2) WG_HIP_CHECK(hipMemsetAsync(grad_b2, 0, sizeof(float), st));
      return;
    }
    WG_REQUIRE_INPUT(hidden_io && w2 && g && index_src && index_dst && workspace, "null pointer");
    WG_REQUIRE_INPUT(workspace_bytes >= wgamd_pair_mlp_backward_workspace_bytes(hidden), "workspace too small");
    float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 15) / 16 * 16);
    if (!workspace_is_zeroed) WG_HIP_CHECK(hipMemsetAsync(ws, 0, 16, st));
    int lgh = 0;
    while ((1 << lgh) < hidden) lgh++;
    const int64_t groups = kThreads >> lgh;
    // whole passes of a workgroup's row groups, at least 8 of them per workgroup
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>((n_pairs + 8 * groups - 1) / (8 * groups), kMlpBwdGrid));
    const int64_t rpb  = ((n_pairs + want - 1) / want + groups - 1) / groups * groups;
    const int grid     = (int)((n_pairs + rpb - 1) / rpb);
    pair_mlp_bwd_kernel<<<grid, kThreads, 0, st>>>(hidden_io, ld_hidden, n_pairs, hidden, lgh, w2, g, scale_num, scale_den, index_src,
                                                  n_src, index_dst, n_dst, rpb, grad_w2, grad_b2, ws);
    WG_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
