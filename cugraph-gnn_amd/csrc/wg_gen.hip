// GEN layer (torch_geometric.nn.GENConv of DeeperGCN with aggr="softmax", flow source_to_target) over a sampled hop:
//     m_j       = max(X[j], 0) + eps_m                                       (the message of source row j, the same on every edge)
//     agg[i, c] = sum_{e = (j -> i)} p_ec m_jc ,   p_ec = exp(t m_jc) / sum_{e' = (k -> i)} exp(t m_kc)      (0 without edges)
//     A[i, :]   = agg[i, :] + X_self[i, :]
//     out[i, :] = act2( max(A[i] @ W1^T + b1, 0) @ W2^T + b2 )
// The softmax runs PER CHANNEL: the weight of an edge depends on the value it weighs, so the running maximum and the denominator
// are per (row, channel) — not per (row, head) as in the attention kernels — and the [E, C] messages, exponentials and weights of
// the torch-ops formulation (1 KiB per edge each at C = 256) are never written.  t is ONE float on the device (a learnt
// temperature costs no host read); it may be negative or zero (t = 0: the mean).
//
//   * gen_layer_kernel — the whole layer, one launch per hop, in the frame of gin_layer_kernel (16-row tiles, 4 waves, two LDS
//     tiles; phases 2 and 3 are wg_gin_parts.hpp's).  Phase 1: a lane group of LG >= C / 4 lanes per destination row, a lane = one
//     float4 of the row, the edges eight at a time in CSR order.  Per channel three registers: the extreme message so far (the
//     largest with t > 0, the smallest with t < 0), the denominator sum w and the numerator sum w (m - extreme), both relative to
//     that extreme.  One edge, base 2 with t' = t log2 e: d = t' (m - extreme); one exp2(-|d|); where d > 0 the extreme moves and
//     the two sums are rescaled by it, elsewhere the edge's term is added — the exponent is formed from a DIFFERENCE of messages, so
//     its rounding error is relative to d, not to t' m, no exponential can overflow, and a row of equal messages gives that message
//     exactly.  agg = extreme + num / den, and with a training launch
//     L = t' extreme + log2 den (the per-channel log-sum-exp, base 2), agg and A are stored per destination row: every weight is
//     p = exp2(t' m - L) again in the backward.  With a null W1 the kernel stores A and ends (the mlp then runs outside).
//   * gen_bwd_src_kernel — over the hop's transpose, a lane group per SOURCE row holding m_j: every entry reads the rows L, agg
//     and dA of its destination and adds  dm_j += p dA (1 + t (m_j - agg)),  dt += dA p m_j (m_j - agg);  the row's sum is masked by
//     X[j] > 0 and, where input row j is a destination itself, dA of that row is added.  wg_sage_max.hip's routing walk: a
//     workgroup owns 16 source rows at a time, a row of at most 64 entries is one lane group's, a longer one is cut into 64-entry
//     pieces that all lane groups take round-robin and whose sums are added in group order from LDS.  The grid is bounded
//     (min(tiles, 4 x CUs) workgroups at a FIXED stride over the tiles); a thread's dt stays in one register over all its tiles,
//     the workgroup's sum (lanes by xor shuffles, waves in wave order) leaves as one partial per workgroup.
// No atomics anywhere: the same bits from run to run.  Matrix instructions do not fit phase 1 (a per-channel recurrence along the
// edges, no product); the two products are on the fp32 matrix pipe.
#include <cfloat>

#include "wg_gin_parts.hpp"

namespace wgamd {
namespace {

constexpr int kGenWgCu  = 4;      // workgroups per CU of the backward
constexpr int kGenPiece = 64;     // entries per piece of a long transposed row
constexpr int kGenBwdUnroll = 4;  // entries of a source row in flight (three destination rows each)
constexpr float kLog2e = 1.4426950408889634f;

struct gen_args : gin_args {
  const float* t;             // ONE float on the device
  float msg_eps;
  float* sum_out;             // nullable: agg [n_rows, ld_sum] (agg_out of gin_args holds A)
  int64_t ld_sum;
  float* lse_out;             // nullable: L [n_rows, ld_lse]
  int64_t ld_lse;
};

// the extreme a row starts from: the first edge always moves it (den = 0, so nothing is rescaled); t = 0 never does (every d = 0,
// every term 1: the mean around 0)
__device__ __forceinline__ float gen_start(float t2) { return t2 > 0.f ? -FLT_MAX : (t2 < 0.f ? FLT_MAX : 0.f); }

// agg of destination row i, channels [4 c, 4 c + 4), and its L
template <int KIND>
__device__ __forceinline__ f32x4 gen_chunk(const gen_args& a, int64_t i, int c, bool active, float t2, f32x4& lse)
{
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  const float ext0 = gen_start(t2);
  f32x4 ext = {ext0, ext0, ext0, ext0}, den = {0.f, 0.f, 0.f, 0.f}, num = den;      // num: sum of w (m - ext)
  for (int e = s; e < t; e += kGinUnroll) {
    int j[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) j[u] = e + u < t ? a.col[e + u] : -1;
    f32x4 v[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j[u] >= 0 && active) v[u] = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j[u]))[c];
    }
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      if (j[u] >= 0) {                                     // (the same for a whole lane group)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float m = fmaxf(v[u][k], 0.f) + a.msg_eps;
          const float dm = m - ext[k];
          const float d = t2 * dm;
          const float w = __builtin_amdgcn_exp2f(-fabsf(d));
          const bool moved = d > 0.f;                      // the sums go over to the new extreme: every old deviation grows by -dm
          num[k] = moved ? w * __builtin_fmaf(den[k], -dm, num[k]) : __builtin_fmaf(w, dm, num[k]);
          den[k] = moved ? __builtin_fmaf(den[k], w, 1.f) : den[k] + w;
          ext[k] = moved ? m : ext[k];
        }
      }
    }
  }
  f32x4 agg = {0.f, 0.f, 0.f, 0.f};
  lse = agg;
  if (t > s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      agg[k] = ext[k] + num[k] / den[k];
      lse[k] = __builtin_fmaf(t2, ext[k], log2f(den[k]));
    }
  }
  return agg;
}

template <int KIND, int LG>
__global__ void __launch_bounds__(kThreads) gen_layer_kernel(gen_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int kGroups = kThreads / LG;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int grp = tid / LG, c = tid % LG;
  const int C4 = a.F / 4;
  const float t2 = *a.t * kLog2e;

  // ---- phase 1: A = agg + self row of the tile's rows -> LDS tile A (and agg_out, sum_out, lse_out) ----
  for (int r = grp; r < kTileRows; r += kGroups) {
    const int64_t i = row0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < a.n_rows) {
      f32x4 lse;
      const f32x4 agg = gen_chunk<KIND>(a, i, c, c < C4, t2, lse);
      v = agg;
      const f32x4* self = self_row<KIND>(a, i);
      if (self && c < C4) v += self[c];
      if (c < C4) {
        if (a.sum_out) reinterpret_cast<f32x4*>(a.sum_out + i * a.ld_sum)[c] = agg;
        if (a.lse_out) reinterpret_cast<f32x4*>(a.lse_out + i * a.ld_lse)[c] = lse;
        if (a.agg_out) reinterpret_cast<f32x4*>(a.agg_out + i * a.ld_agg)[c] = v;
      }
    }
    if (a.w1) store_agg_chunk<LG>(tile, a, r, c, v);
  }
  if (a.w1 == nullptr) return;                           // (uniform) A alone: agg_out is the output
  __syncthreads();
  gin_tile_products(a, tile, row0);
}

template <int KIND, int LG>
void launch_one(const gen_args& a, hipStream_t st)
{
  auto kern = gen_layer_kernel<KIND, LG>;
  const dim3 grid((unsigned)((a.n_rows + kTileRows - 1) / kTileRows));
  const size_t lds = a.w1 ? (size_t)kTileRows * (a.SD + (a.w2 ? a.SH : 0)) * 4 : 0;      // at most 2 x 16 x 260 floats = 33 KB
  kern<<<grid, kThreads, lds, st>>>(a);
}

// ---- source-major backward: the input rows' gradient and dt ---------------------------------------------------------------------
struct gen_src_args {
  const int* row_ptr_t;       // the hop's transpose: rows = input rows
  const int* col_t;           // destination row of every entry
  int64_t n_src;
  int n_tiles;
  const float* x;             // the layer's input rows (read by row or through src_ids)
  int64_t ldx;
  const void* src_ids;
  int F;
  const float* t;
  float msg_eps;
  const float* lse;           // [n_dst, ld_lse]
  int64_t ld_lse;
  const float* agg;           // [n_dst, ld_agg]
  int64_t ld_agg;
  const float* dagg;          // [n_dst, ld_dagg]
  int64_t ld_dagg;
  const int64_t* self_t;      // nullable; the destination row that input row j is itself, < 0 = none
  float* gx;                  // [n_src, ldgx], every row written
  int64_t ldgx;
  float* dt_part;             // [gridDim.x]
  int lg_shift;
};

// dm of the message m over the entries [s, t), channels [4 c, 4 c + 4), in entry order; dt of the same entries is added to `dt`
__device__ __forceinline__ f32x4 gen_entries(const gen_src_args& a, int s, int t, int c, bool active, f32x4 m, float tn, float t2,
                                             float& dt)
{
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int e = s; e < t; e += kGenBwdUnroll) {
    int d[kGenBwdUnroll];
#pragma unroll
    for (int u = 0; u < kGenBwdUnroll; ++u) d[u] = e + u < t ? a.col_t[e + u] : -1;
    f32x4 L[kGenBwdUnroll], g[kGenBwdUnroll], ag[kGenBwdUnroll];
#pragma unroll
    for (int u = 0; u < kGenBwdUnroll; ++u) {
      L[u] = g[u] = ag[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (d[u] >= 0 && active) {
        L[u]  = reinterpret_cast<const f32x4*>(a.lse + (int64_t)d[u] * a.ld_lse)[c];
        ag[u] = reinterpret_cast<const f32x4*>(a.agg + (int64_t)d[u] * a.ld_agg)[c];
        g[u]  = reinterpret_cast<const f32x4*>(a.dagg + (int64_t)d[u] * a.ld_dagg)[c];
      }
    }
#pragma unroll
    for (int u = 0; u < kGenBwdUnroll; ++u) {
      if (d[u] >= 0 && active) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float pg = __builtin_amdgcn_exp2f(__builtin_fmaf(t2, m[k], -L[u][k])) * g[u][k];      // p dA
          const float dev = m[k] - ag[u][k];
          acc[k] += pg * __builtin_fmaf(tn, dev, 1.f);
          dt = __builtin_fmaf(pg * m[k], dev, dt);
        }
      }
    }
  }
  return acc;
}

// the finished sum of input row j, masked by x > 0, plus its root term -> gx
__device__ __forceinline__ void gen_store_row(const gen_src_args& a, int64_t j, int c, f32x4 total, f32x4 xv)
{
#pragma unroll
  for (int k = 0; k < 4; ++k) total[k] = xv[k] > 0.f ? total[k] : 0.f;
  const int64_t self = a.self_t ? a.self_t[j] : -1;
  if (self >= 0) total += reinterpret_cast<const f32x4*>(a.dagg + self * a.ld_dagg)[c];
  reinterpret_cast<f32x4*>(a.gx + j * a.ldgx)[c] = total;
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) gen_bwd_src_kernel(gen_src_args a)
{
  __shared__ f32x4 part[kThreads];
  __shared__ float wave_dt[kThreads / 64];
  const int tid = threadIdx.x;
  const int LG = 1 << a.lg_shift, groups = kThreads >> a.lg_shift;
  const int grp = tid >> a.lg_shift, c = tid & (LG - 1);
  const bool active = c < a.F / 4;
  const float tn = *a.t, t2 = tn * kLog2e;
  float dt = 0.f;

  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {            // (a fixed stride: the same sums every run)
    const int64_t row0 = (int64_t)tile * kTileRows;
    // rows of at most kGenPiece entries: one lane group each
    for (int r = grp; r < kTileRows; r += groups) {
      const int64_t j = row0 + r;
      if (j >= a.n_src) break;
      const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
      if (t - s > kGenPiece || !active) continue;
      const f32x4 xv = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j))[c];
      f32x4 m;
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = fmaxf(xv[k], 0.f) + a.msg_eps;
      gen_store_row(a, j, c, gen_entries(a, s, t, c, true, m, tn, t2, dt), xv);
    }

    // longer rows: every lane group takes pieces round-robin (r, s, t are the same in every thread: the barriers are uniform)
    for (int r = 0; r < kTileRows; ++r) {
      const int64_t j = row0 + r;
      if (j >= a.n_src) break;
      const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
      if (t - s <= kGenPiece) continue;
      f32x4 xv = {0.f, 0.f, 0.f, 0.f}, m, acc = xv;
      if (active) xv = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j))[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = fmaxf(xv[k], 0.f) + a.msg_eps;
      for (int p0 = s + grp * kGenPiece; p0 < t; p0 += groups * kGenPiece) {
        const f32x4 piece = gen_entries(a, p0, std::min(t, p0 + kGenPiece), c, active, m, tn, t2, dt);
        acc += piece;
      }
      __syncthreads();      // (the previous long row's sums have been read)
      part[tid] = acc;
      __syncthreads();
      if (grp == 0 && active) {
        f32x4 total = part[c];
        for (int g = 1; g < groups; ++g) total += part[g * LG + c];
        gen_store_row(a, j, c, total, xv);
      }
    }
  }

  // the workgroup's dt: lanes by xor shuffles, waves in wave order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dt += __shfl_xor(dt, o);
  if ((tid & 63) == 0) wave_dt[tid >> 6] = dt;
  __syncthreads();
  if (tid == 0) a.dt_part[blockIdx.x] = ((wave_dt[0] + wave_dt[1]) + wave_dt[2]) + wave_dt[3];
}

void gen_require_shape(int F, int H, int N)
{
  if (!wgamd_gen_layer_supported(F, H, N))
    throw logic_error(fmt("unsupported shape: C=%d (multiple of 4, <= 256), H=%d (<= 256; multiple of 4 with a second product), "
                          "N=%d (<= 256)", F, H, N));
}

int64_t gen_tiles(int64_t n_rows) { return n_rows <= 0 ? 0 : (n_rows + kTileRows - 1) / kTileRows; }

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_gen_layer_supported(int F, int H, int N) { return wgamd_gin_layer_supported(F, H, N); }

extern "C" int64_t wgamd_gen_bwd_blocks(int64_t n_src, int max_blocks)
{
  const int64_t cap = max_blocks > 0 ? max_blocks : (int64_t)wgamd::kGenWgCu * wgamd::stream_cu_count(nullptr);
  return std::min<int64_t>(wgamd::gen_tiles(n_src), cap);
}

extern "C" wholememory_error_code_t wgamd_gen_layer_f32_train(
    const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* t, float msg_eps,
    const float* w1, int64_t ldw1, int H, const float* b1, const float* w2, int64_t ldw2, int N, const float* b2, int flags,
    float* out, int64_t ldo, float* a_out, int64_t ld_a, float* hidden_out, int64_t ld_hidden, float* agg_out, int64_t ld_agg,
    float* lse_out, int64_t ld_lse, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gen_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    WG_REQUIRE_INPUT((w1 == nullptr) == (w2 == nullptr), "w1 and w2 come together (the two-layer mlp), or neither (A alone)");
    WG_REQUIRE_INPUT((w2 == nullptr) == (N == 0) && (w1 == nullptr) == (H == 0), "H and N are 0 exactly without w1 and w2");
    gen_require_shape(F, w1 ? H : 1, N);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && out && t, "null pointer");
    WG_REQUIRE_INPUT((w1 == nullptr || (ldw1 >= F && ldw2 >= H)) && ldo >= (w2 ? N : F), "leading dimension too small");
    WG_REQUIRE_INPUT((a_out == nullptr || ld_a >= F) && (hidden_out == nullptr || ld_hidden >= H) && (agg_out == nullptr || ld_agg >= F) &&
                       (lse_out == nullptr || ld_lse >= F) && (x_dst == nullptr || ldx_dst >= F), "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || (w1 && (!aligned_rows(w1, ldw1) || !aligned_rows(w2, ldw2))) ||
        (x_dst && !aligned_rows(x_dst, ldx_dst)) || (a_out && !aligned_rows(a_out, ld_a)) ||
        (hidden_out && !aligned_rows(hidden_out, ld_hidden)) || (agg_out && !aligned_rows(agg_out, ld_agg)) ||
        (lse_out && !aligned_rows(lse_out, ld_lse)) || (w1 == nullptr && !aligned_rows(out, ldo)))
      throw logic_error("x / x_dst / w1 / w2 / a_out / hidden_out / agg_out / lse_out rows must be 16-B aligned");
    gen_args a{};
    static_cast<gin_args&>(a) = make_gin_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, x_dst, ldx_dst, nullptr);
    a.w1 = w1, a.ldw1 = ldw1, a.H = H, a.b1 = b1, a.relu1 = 1;
    a.w2 = w2, a.ldw2 = ldw2, a.N = N, a.b2 = b2, a.relu2 = (flags & WGAMD_GIN_RELU_OUT) != 0;
    a.out = out, a.ldo = ldo, a.agg_out = a_out, a.ld_agg = ld_a;
    if (w1 == nullptr) a.agg_out = out, a.ld_agg = ldo;
    a.hidden_out = w2 ? hidden_out : nullptr, a.ld_hidden = ld_hidden;
    a.t = t, a.msg_eps = msg_eps, a.sum_out = agg_out, a.ld_sum = ld_agg, a.lse_out = lse_out, a.ld_lse = ld_lse;
    tile_geometry(F, a.F16, a.SD), tile_geometry(w1 ? H : 1, a.H16, a.SH);
    auto st = static_cast<hipStream_t>(stream);
    with_kind(kind, [&](auto k) {
      with_lane_group(F, [&](auto lg) { launch_one<decltype(k)::value, decltype(lg)::value>(a, st); });
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gen_layer_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* t, float msg_eps,
    const float* w1, int64_t ldw1, int H, const float* b1, const float* w2, int64_t ldw2, int N, const float* b2, int flags,
    float* out, int64_t ldo, void* stream)
{
  return wgamd_gen_layer_f32_train(row_ptr, col, n_rows, x, ldx, F, src_ids, src_ids_dtype, self_rows, x_dst, ldx_dst, t, msg_eps, w1,
                                   ldw1, H, b1, w2, ldw2, N, b2, flags, out, ldo, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_gen_bwd_src_f32(const int* row_ptr_t, const int* col_t, int64_t n_src, const float* x,
                                                          int64_t ldx, int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                          const float* t, float msg_eps, const float* lse, int64_t ld_lse,
                                                          const float* agg, int64_t ld_agg, const float* dagg, int64_t ld_dagg,
                                                          const int64_t* self_t, float* gx, int64_t ldgx, float* dt_part,
                                                          int64_t n_blocks, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gen_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    gen_require_shape(F, 1, 0);
    if (n_src == 0) return;
    const int64_t tiles = gen_tiles(n_src);
    WG_REQUIRE_INPUT(n_blocks >= 1 && n_blocks <= tiles && tiles <= INT32_MAX, "n_blocks: 1 .. the input rows' tiles of 16 rows");
    WG_REQUIRE_INPUT(row_ptr_t && col_t && x && t && lse && agg && dagg && gx && dt_part, "null pointer");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT((kind == 3 || ldx >= F) && ld_lse >= F && ld_agg >= F && ld_dagg >= F && ldgx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || !aligned_rows(lse, ld_lse) || !aligned_rows(agg, ld_agg) ||
        !aligned_rows(dagg, ld_dagg) || !aligned_rows(gx, ldgx))
      throw logic_error("x / lse / agg / dagg / gx rows must be 16-B aligned");
    gen_src_args a{};
    a.row_ptr_t = row_ptr_t, a.col_t = col_t, a.n_src = n_src, a.n_tiles = (int)tiles, a.x = x, a.ldx = ldx, a.src_ids = src_ids, a.F = F;
    a.t = t, a.msg_eps = msg_eps, a.lse = lse, a.ld_lse = ld_lse, a.agg = agg, a.ld_agg = ld_agg, a.dagg = dagg, a.ld_dagg = ld_dagg;
    a.self_t = self_t, a.gx = gx, a.ldgx = ldgx, a.dt_part = dt_part;
    a.lg_shift = 2;
    while ((1 << a.lg_shift) < F / 4) ++a.lg_shift;
    const dim3 grid((unsigned)n_blocks);
    auto st = static_cast<hipStream_t>(stream);
    with_kind(kind, [&](auto k) { gen_bwd_src_kernel<decltype(k)::value><<<grid, kThreads, 0, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}
