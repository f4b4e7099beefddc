// GIN layer WITH EDGE FEATURES (torch_geometric.nn.GINEConv, flow source_to_target) over a sampled hop, with the GIN paper's MLP:
//     m_e       = X[j] + b_e + W_e ea[e]                       (e = (j -> i); ea [E, D]: one row per CSR slot)
//     agg[i, :] = sum_e max(m_e, 0)  +  (1 + eps) X_self[i]    (every edge summed: loops and duplicates too; no edge row at the root)
//     out[i, :] = act2( act1(agg[i] @ W1^T + b1) @ W2^T + b2 )
// With D == 0 (a compile-time variant) the edge's row is F wide and read beside X[j]: m_e = X[j] + ea[e], no weight.
// lin(ea) and the messages are [E, F] tensors — 1 KiB per edge each at F = 256 — that these kernels never write.
//
//   * gine_layer_kernel — the whole layer, one launch per hop, in the frame of gin_layer_kernel (16-row tiles, 4 waves, two LDS
//     tiles; phases 2 and 3 are wg_gin_parts.hpp's).  Behind the tiles LDS holds W_e^T [D][LG] and b_e [LG] as float4 (zeros
//     behind F: an idle lane's message is zero) and, per lane group, the attributes of the eight edges in flight.  Phase 1: a
//     lane group of LG >= F / 4 lanes per destination row, a lane = one float4 of the row, the edges eight at a time in CSR order.
//     The group loads the batch's 8 D attributes (contiguous in slot order) with one strided read and lays them out [d][u] in its
//     LDS slice; for each d one 16-byte read of W_e^T[d] and two of the attributes feed the eight edges: m[u] += ea[u][d] w4.
//     Then acc += max(m[u], 0) in slot order.  The training variant (mask != null) stores the ReLU mask as BITS: per slot
//     ceil(F / 32) words, bit f = m[f] > 0 — a lane's four compares are a nibble, eight lanes' nibbles are OR-ed with three
//     shuffles inside the group, one lane per 32 features stores the word: 32 B per edge at F = 256 against the 1 KiB row.
//     With a null W1 the kernel ends after phase 1 (out = agg): the route of an nn that starts with no Linear.
//   * gine_bwd_dst_kernel — dW_e^T[d, f] = sum_e ea[e, d] bit_e[f] dAgg[dst(e), f] and db_e[f] = sum_e bit_e[f] dAgg[dst(e), f],
//     reading only ea, the mask words and dAgg: one wave per row, lane = one float4 of the row, edges in groups of four whose
//     4 D <= 64 attributes are one read and reach the multiply as scalars (v_readlane), sums in registers (4 columns x (DP + 1)
//     per lane, DP = D rounded up to a multiple of 4).  The grid is bounded (min(tiles, 4 x CUs) workgroups at a FIXED stride),
//     the four waves' sums are added in wave order through LDS and leave as a per-workgroup partial [D + 1, F].
//   * gine_bwd_src_kernel — over the hop's transpose: dX[j, f] = sum over the entries of row j of bit_{perm}[f] dAgg[col_t, f]
//     (+ (1 + eps) dAgg[i] where input row j is destination i itself).  wg_sage_max.hip's routing walk: a workgroup owns 16
//     source rows, a row of at most 64 entries is one lane group's, a longer one is cut into 64-entry pieces that all lane
//     groups take round-robin and whose sums are added in group order from LDS.
// No atomics anywhere: the same bits from run to run.  Matrix instructions do not fit phase 1: K = D <= 16 per edge, and the
// product is needed per edge in the lane = column layout, ahead of a ReLU, not summed in an MFMA accumulator.
#include "wg_gin_parts.hpp"

namespace wgamd {
namespace {

constexpr int kGineMaxD  = 16;    // W_e^T within 16 KB of LDS; 4 edges x D attributes within one wave's lanes in the backward
constexpr int kGineWgCu  = 4;     // workgroups per CU of the destination-major backward
constexpr int kGinePiece = 64;    // entries per piece of a long transposed row

struct gine_args : gin_args {
  const float* ea;            // [E, D] in CSR slot order ([E, F] with D == 0)
  const float* wet;           // W_e^T [D, F]
  const float* be;            // [F], nullable
  int D;
  uint32_t* mask;             // nullable: [E, MW] words
  int MW;
};

__device__ __forceinline__ void wave_sync_lds()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The aggregate of destination row i, features [4 c, 4 c + 4).  wl: W_e^T [D][LG] then b_e [LG]; stage: the group's [D][8] floats.
template <int KIND, int LG, bool LIN>
__device__ __forceinline__ f32x4 gine_chunk(const gine_args& a, int64_t i, int c, bool active, float self_coef, const f32x4* wl,
                                            float* stage)
{
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1], D = a.D;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, b4 = acc;
  if constexpr (LIN) b4 = wl[D * LG + c];
  for (int e = s; e < t; e += kGinUnroll) {
    int j[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) j[u] = e + u < t ? a.col[e + u] : -1;
    f32x4 m[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      m[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j[u] >= 0 && active) m[u] = reinterpret_cast<const f32x4*>(x_row<KIND>(a.x, a.ldx, a.src_ids, j[u]))[c];
    }
    if constexpr (LIN) {
      const int have = min(kGinUnroll, t - e) * D;       // the batch's attributes: contiguous from ea[e, 0]
      wave_sync_lds();                                   // (the previous batch's reads are done: LDS is in order within a wave)
      for (int k = c; k < kGinUnroll * D; k += LG) {
        const int u = k / D, d = k - u * D;
        stage[d * kGinUnroll + u] = k < have ? a.ea[(int64_t)e * D + k] : 0.f;
      }
      wave_sync_lds();
#pragma unroll
      for (int u = 0; u < kGinUnroll; ++u) m[u] += b4;
      for (int d = 0; d < D; ++d) {
        const f32x4 w4 = wl[d * LG + c];
        const f32x4 lo = *reinterpret_cast<const f32x4*>(stage + d * kGinUnroll);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(stage + d * kGinUnroll + 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          m[u] += lo[u] * w4;
          m[4 + u] += hi[u] * w4;
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < kGinUnroll; ++u)
        if (j[u] >= 0 && active) m[u] += reinterpret_cast<const f32x4*>(a.ea + (int64_t)(e + u) * a.F)[c];
    }
    if (a.mask) {                                        // (uniform) the ReLU mask of every slot, 32 features per word
#pragma unroll
      for (int u = 0; u < kGinUnroll; ++u) {
        uint32_t nib = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) nib |= (j[u] >= 0 && m[u][k] > 0.f ? 1u : 0u) << k;
        nib <<= 4 * (c & 7);
        nib |= __shfl_xor(nib, 1);
        nib |= __shfl_xor(nib, 2);
        if constexpr (LG >= 8) nib |= __shfl_xor(nib, 4);
        if (j[u] >= 0 && (c & 7) == 0 && (c >> 3) < a.MW) a.mask[(int64_t)(e + u) * a.MW + (c >> 3)] = nib;
      }
    }
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {               // (an edge behind the row's end holds b_e: not summed)
      if (j[u] >= 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += fmaxf(m[u][k], 0.f);
      }
    }
  }
  const f32x4* self = self_row<KIND>(a, i);
  if (self && active) acc += self_coef * self[c];
  return acc;
}

template <int KIND, int LG, bool LIN>
__global__ void __launch_bounds__(kThreads) gine_layer_kernel(gine_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int kGroups = kThreads / LG;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const float self_coef = 1.f + (a.eps ? *a.eps : 0.f);
  const int grp = tid / LG, c = tid % LG;
  const int C4 = a.F / 4;
  float* behind = tile + kTileRows * (a.SD + (a.w2 ? a.SH : 0));
  f32x4* wl = reinterpret_cast<f32x4*>(behind);
  float* stage = behind + (a.D + 1) * LG * 4 + grp * (kGinUnroll * a.D);
  if constexpr (LIN) {
    for (int idx = tid; idx < (a.D + 1) * LG; idx += kThreads) {
      const int d = idx / LG, l = idx % LG;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (l < C4 && d < a.D) v = reinterpret_cast<const f32x4*>(a.wet + (int64_t)d * a.F)[l];
      else if (l < C4 && a.be) v = reinterpret_cast<const f32x4*>(a.be)[l];
      wl[idx] = v;
    }
    __syncthreads();
  }

  // ---- phase 1: the aggregate rows of the tile -> LDS tile A (and agg_out) ----
  for (int r = grp; r < kTileRows; r += kGroups) {
    const int64_t i = row0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < a.n_rows) {                                  // (the same for a whole lane group: the shuffles stay inside it)
      v = gine_chunk<KIND, LG, LIN>(a, i, c, c < C4, self_coef, wl, stage);
      if (a.agg_out && c < C4) reinterpret_cast<f32x4*>(a.agg_out + i * a.ld_agg)[c] = v;
    }
    store_agg_chunk<LG>(tile, a, r, c, v);
  }
  if (a.w1 == nullptr) return;                           // (uniform) the aggregate alone: agg_out is the output
  __syncthreads();
  gin_tile_products(a, tile, row0);
}

template <int KIND, int LG, bool LIN>
void launch_one(const gine_args& a, hipStream_t st)
{
  auto kern = gine_layer_kernel<KIND, LG, LIN>;
  const dim3 grid((unsigned)((a.n_rows + kTileRows - 1) / kTileRows));
  // the two tiles (at most 33 KB), then W_e^T and b_e (17 x LG float4) and 8 D floats per lane group: 52.6 KB at most
  size_t lds = (size_t)kTileRows * (a.SD + (a.w2 ? a.SH : 0)) * 4;
  if (LIN) lds += (size_t)(a.D + 1) * LG * 16 + (size_t)(kThreads / LG) * kGinUnroll * a.D * 4;
  kern<<<grid, kThreads, lds, st>>>(a);
}

// ---- destination-major backward: dW_e^T and db_e ------------------------------------------------------------------------------
struct gine_dst_args {
  const int* row_ptr;
  int64_t n_rows;
  const float* ea;
  const uint32_t* mask;
  int MW;
  const float* dagg;          // [n_rows, ld_dagg]
  int64_t ld_dagg;
  int F, D;
  float* part;                // [n_blocks, D + 1, F]
  int n_tiles;
};

template <int DP>
__global__ void __launch_bounds__(256) gine_bwd_dst_kernel(gine_dst_args a)
{
  __shared__ f32x4 part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = a.D, F = a.F;
  const bool on = lane < F / 4;
  const int word = lane >> 3, shift = 4 * (lane & 7);
  f32x4 db = {0.f, 0.f, 0.f, 0.f}, dw[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) dw[d] = db;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {          // (a fixed stride: the same sums every run)
    const int64_t row0 = (int64_t)tile * kTileRows;
    for (int r = wave; r < kTileRows; r += 4) {
      const int64_t i = row0 + r;
      if (i >= a.n_rows) break;                   // (wave-uniform)
      const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
      if (s == t) continue;
      f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
      if (on) g4 = reinterpret_cast<const f32x4*>(a.dagg + i * a.ld_dagg)[lane];
      for (int e0 = s; e0 < t; e0 += 4) {
        const float eav = lane < min(4, t - e0) * D ? a.ea[(int64_t)e0 * D + lane] : 0.f;     // the group's rows are contiguous
        f32x4 ds[4];                              // dL/d m_e: the gradient where the ReLU passed (zeros behind the row's end)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          ds[v] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (e0 + v < t && on) {
            const uint32_t bits = a.mask[(int64_t)(e0 + v) * a.MW + word] >> shift;
#pragma unroll
            for (int k = 0; k < 4; ++k) ds[v][k] = (bits >> k) & 1u ? g4[k] : 0.f;
            db += ds[v];
          }
        }
#pragma unroll
        for (int d = 0; d < DP; ++d) {            // (a uniform branch per attribute: the padding costs nothing)
          if (d < D) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
              dw[d] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(eav), v * D + d)) * ds[v];
          }
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d <= DP; ++d) {                 // (uniform barriers: DP is the kernel's, every thread arrives)
    __syncthreads();
    part[wave][lane] = d < DP ? dw[d < DP ? d : 0] : db;
    __syncthreads();
    const int row = d < DP ? d : D;               // (the bias row sits behind the D weight rows)
    if (wave == 0 && on && (d < D || d == DP))
      reinterpret_cast<f32x4*>(a.part + ((int64_t)blockIdx.x * (D + 1) + row) * F)[lane] =
          ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
  }
}

// ---- source-major backward: the input rows' gradient --------------------------------------------------------------------------
struct gine_src_args {
  const int* row_ptr_t;       // the hop's transpose: rows = input rows
  const int* col_t;           // destination row of every entry
  const int* perm;            // the hop's CSR edge slot of every entry
  int64_t n_src;
  const uint32_t* mask;
  int MW;
  const float* dagg;          // [n_dst, ld_dagg]
  int64_t ld_dagg;
  int F;
  const int64_t* self_t;      // nullable; the destination row that input row j is itself, < 0 = none
  const float* eps;
  float* gx;                  // [n_src, ldgx], every row written
  int64_t ldgx;
  int lg_shift;
};

// sum over the entries [s, t) of bit_{perm}[f] dagg[col_t, f], features [4 c, 4 c + 4), in entry order
__device__ __forceinline__ f32x4 masked_entries(const gine_src_args& a, int s, int t, int c, bool active)
{
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int word = c >> 3, shift = 4 * (c & 7);
  for (int e = s; e < t; e += kGinUnroll) {
    int d[kGinUnroll], p[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      d[u] = e + u < t ? a.col_t[e + u] : -1;
      p[u] = e + u < t ? a.perm[e + u] : 0;
    }
    uint32_t bits[kGinUnroll];
    f32x4 g[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      bits[u] = 0;
      g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (d[u] >= 0 && active) {
        bits[u] = a.mask[(int64_t)p[u] * a.MW + word] >> shift;
        g[u] = reinterpret_cast<const f32x4*>(a.dagg + (int64_t)d[u] * a.ld_dagg)[c];
      }
    }
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += (bits[u] >> k) & 1u ? g[u][k] : 0.f;
  }
  return acc;
}

// the finished sum of input row j plus its root term -> gx
__device__ __forceinline__ void store_src_row(const gine_src_args& a, int64_t j, int c, f32x4 total, float self_coef)
{
  const int64_t self = a.self_t ? a.self_t[j] : -1;
  if (self >= 0) total += self_coef * reinterpret_cast<const f32x4*>(a.dagg + self * a.ld_dagg)[c];
  reinterpret_cast<f32x4*>(a.gx + j * a.ldgx)[c] = total;
}

__global__ void __launch_bounds__(kThreads) gine_bwd_src_kernel(gine_src_args a)
{
  __shared__ f32x4 part[kThreads];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int LG = 1 << a.lg_shift, groups = kThreads >> a.lg_shift;
  const int grp = tid >> a.lg_shift, c = tid & (LG - 1);
  const bool active = c < a.F / 4;
  const float self_coef = 1.f + (a.eps ? *a.eps : 0.f);

  // rows of at most kGinePiece entries: one lane group each
  for (int r = grp; r < kTileRows; r += groups) {
    const int64_t j = row0 + r;
    if (j >= a.n_src) break;
    const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
    if (t - s > kGinePiece) continue;
    const f32x4 acc = masked_entries(a, s, t, c, active);
    if (active) store_src_row(a, j, c, acc, self_coef);
  }

  // longer rows: every lane group takes pieces round-robin (r, s, t are the same in every thread: the barriers are uniform)
  for (int r = 0; r < kTileRows; ++r) {
    const int64_t j = row0 + r;
    if (j >= a.n_src) break;
    const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
    if (t - s <= kGinePiece) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p0 = s + grp * kGinePiece; p0 < t; p0 += groups * kGinePiece) {
      const f32x4 piece = masked_entries(a, p0, std::min(t, p0 + kGinePiece), c, active);
      acc += piece;
    }
    __syncthreads();      // (the previous long row's sums have been read)
    part[tid] = acc;
    __syncthreads();
    if (grp == 0 && active) {
      f32x4 total = part[c];
      for (int g = 1; g < groups; ++g) total += part[g * LG + c];
      store_src_row(a, j, c, total, self_coef);
    }
  }
}

void gine_require_shape(int F, int H, int N, int D)
{
  if (!wgamd_gine_layer_supported(F, H, N, D))
    throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, <= 256), H=%d (<= 256; multiple of 4 with a second product), "
                          "N=%d (<= 256), D=%d (0 = edge rows of width F, or 1 .. %d)", F, H, N, D, kGineMaxD));
}

int mask_words(int F) { return (F + 31) / 32; }

int64_t gine_tiles(int64_t n_rows) { return n_rows <= 0 ? 0 : (n_rows + kTileRows - 1) / kTileRows; }

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_gine_layer_supported(int F, int H, int N, int D)
{
  return wgamd_gin_layer_supported(F, H, N) && D >= 0 && D <= wgamd::kGineMaxD;
}

extern "C" int64_t wgamd_gine_bwd_blocks(int64_t n_rows, int max_blocks)
{
  const int64_t cap = max_blocks > 0 ? max_blocks : (int64_t)wgamd::kGineWgCu * wgamd::stream_cu_count(nullptr);
  return std::min<int64_t>(wgamd::gine_tiles(n_rows), cap);
}

extern "C" wholememory_error_code_t wgamd_gine_layer_f32_train(
    const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps,
    const float* edge_attr, const float* w_edge_t, const float* b_edge, int D, const float* w1, int64_t ldw1, int H, const float* b1,
    const float* w2, int64_t ldw2, int N, const float* b2, int flags, float* out, int64_t ldo, float* agg_out, int64_t ld_agg,
    float* hidden_out, int64_t ld_hidden, uint32_t* mask_out, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gine_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    WG_REQUIRE_INPUT((w2 == nullptr) == (N == 0), "N is 0 exactly when w2 is null (the one-product form)");
    WG_REQUIRE_INPUT(w1 != nullptr || (w2 == nullptr && H == 0), "without w1 (the aggregate alone) there is no w2 and H is 0");
    gine_require_shape(F, w1 ? H : 1, N, D);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && x && out && edge_attr && (D == 0 || w_edge_t), "null pointer");
    const int n_out = w2 ? N : (w1 ? H : F);
    WG_REQUIRE_INPUT((w1 == nullptr || ldw1 >= F) && (w2 == nullptr || ldw2 >= H) && ldo >= n_out, "leading dimension too small");
    WG_REQUIRE_INPUT((agg_out == nullptr || ld_agg >= F) && (hidden_out == nullptr || ld_hidden >= H) &&
                       (x_dst == nullptr || ldx_dst >= F), "leading dimension too small");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT(kind == 3 || ldx >= F, "leading dimension too small");
    if (!aligned_rows(x, kind == 3 ? 0 : ldx) || (w1 && !aligned_rows(w1, ldw1)) || (w2 && !aligned_rows(w2, ldw2)) ||
        (x_dst && !aligned_rows(x_dst, ldx_dst)) || (agg_out && !aligned_rows(agg_out, ld_agg)) ||
        (hidden_out && !aligned_rows(hidden_out, ld_hidden)) || (D == 0 && !aligned_rows(edge_attr, F)) ||
        (w_edge_t && !aligned_rows(w_edge_t, F)) || (b_edge && !aligned_rows(b_edge, 0)) || (w1 == nullptr && !aligned_rows(out, ldo)))
      throw logic_error("x / x_dst / w1 / w2 / agg_out / hidden_out / edge_attr / w_edge_t / b_edge rows must be 16-B aligned");
    gine_args a{};
    static_cast<gin_args&>(a) = make_gin_args(row_ptr, col, n_rows, x, ldx, F, src_ids, self_rows, x_dst, ldx_dst, eps);
    a.w1 = w1, a.ldw1 = ldw1, a.H = H, a.b1 = b1, a.relu1 = (flags & WGAMD_GIN_RELU_HIDDEN) != 0;
    a.w2 = w2, a.ldw2 = ldw2, a.N = N, a.b2 = b2, a.relu2 = (flags & WGAMD_GIN_RELU_OUT) != 0;
    a.out = out, a.ldo = ldo, a.agg_out = agg_out, a.ld_agg = ld_agg;
    if (w1 == nullptr) a.agg_out = out, a.ld_agg = ldo;
    a.hidden_out = w2 ? hidden_out : nullptr, a.ld_hidden = ld_hidden;
    a.ea = edge_attr, a.wet = w_edge_t, a.be = b_edge, a.D = D, a.mask = mask_out, a.MW = mask_words(F);
    tile_geometry(F, a.F16, a.SD), tile_geometry(w1 ? H : 1, a.H16, a.SH);
    auto st = static_cast<hipStream_t>(stream);
    with_kind(kind, [&](auto k) {
      with_lane_group(F, [&](auto lg) {
        if (D > 0) launch_one<decltype(k)::value, decltype(lg)::value, true>(a, st);
        else launch_one<decltype(k)::value, decltype(lg)::value, false>(a, st);
      });
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gine_layer_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps,
    const float* edge_attr, const float* w_edge_t, const float* b_edge, int D, const float* w1, int64_t ldw1, int H, const float* b1,
    const float* w2, int64_t ldw2, int N, const float* b2, int flags, float* out, int64_t ldo, void* stream)
{
  return wgamd_gine_layer_f32_train(row_ptr, col, n_rows, x, ldx, F, src_ids, src_ids_dtype, self_rows, x_dst, ldx_dst, eps, edge_attr,
                                    w_edge_t, b_edge, D, w1, ldw1, H, b1, w2, ldw2, N, b2, flags, out, ldo, nullptr, 0, nullptr, 0,
                                    nullptr, stream);
}

extern "C" wholememory_error_code_t wgamd_gine_bwd_dst_f32(const int* row_ptr, int64_t n_rows, const float* edge_attr, int D,
                                                           const uint32_t* mask, const float* dagg, int64_t ld_dagg, int F,
                                                           float* part, int64_t n_blocks, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gine_bwd_dst_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    gine_require_shape(F, 1, 0, D);
    WG_REQUIRE_INPUT(D >= 1, "D == 0 has no edge weight");
    if (n_rows == 0) return;
    const int64_t tiles = gine_tiles(n_rows);
    WG_REQUIRE_INPUT(n_blocks >= 1 && n_blocks <= tiles && tiles <= INT32_MAX, "n_blocks: 1 .. the hop's tiles of 16 rows");
    WG_REQUIRE_INPUT(row_ptr && edge_attr && mask && dagg && part, "null pointer");
    WG_REQUIRE_INPUT(ld_dagg >= F, "leading dimension too small");
    if (!aligned_rows(dagg, ld_dagg) || !aligned_rows(part, F)) throw logic_error("dagg / part rows must be 16-B aligned");
    gine_dst_args a{};
    a.row_ptr = row_ptr, a.n_rows = n_rows, a.ea = edge_attr, a.mask = mask, a.MW = mask_words(F), a.dagg = dagg, a.ld_dagg = ld_dagg;
    a.F = F, a.D = D, a.part = part, a.n_tiles = (int)tiles;
    const dim3 grid((unsigned)n_blocks);
    auto st = static_cast<hipStream_t>(stream);
    switch ((D + 3) / 4) {
      case 1: gine_bwd_dst_kernel<4><<<grid, 256, 0, st>>>(a); break;
      case 2: gine_bwd_dst_kernel<8><<<grid, 256, 0, st>>>(a); break;
      case 3: gine_bwd_dst_kernel<12><<<grid, 256, 0, st>>>(a); break;
      default: gine_bwd_dst_kernel<16><<<grid, 256, 0, st>>>(a); break;
    }
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gine_bwd_src_f32(const int* row_ptr_t, const int* col_t, const int* perm, int64_t n_src,
                                                           const uint32_t* mask, const float* dagg, int64_t ld_dagg, int F,
                                                           const int64_t* self_t, const float* eps, float* gx, int64_t ldgx,
                                                           void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gine_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    gine_require_shape(F, 1, 0, 0);
    if (n_src == 0) return;
    WG_REQUIRE_INPUT(row_ptr_t && col_t && perm && mask && dagg && gx, "null pointer");
    WG_REQUIRE_INPUT(ld_dagg >= F && ldgx >= F, "leading dimension too small");
    if (!aligned_rows(dagg, ld_dagg) || !aligned_rows(gx, ldgx)) throw logic_error("dagg / gx rows must be 16-B aligned");
    gine_src_args a{};
    a.row_ptr_t = row_ptr_t, a.col_t = col_t, a.perm = perm, a.n_src = n_src, a.mask = mask, a.MW = mask_words(F);
    a.dagg = dagg, a.ld_dagg = ld_dagg, a.F = F, a.self_t = self_t, a.eps = eps, a.gx = gx, a.ldgx = ldgx;
    a.lg_shift = 2;
    while ((1 << a.lg_shift) < F / 4) ++a.lg_shift;
    gine_bwd_src_kernel<<<(unsigned)((n_src + kTileRows - 1) / kTileRows), kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
