// The link-prediction head (include/wgamd_ext.h: wgamd_pair_*): the inner-product decoder of the reference's link examples
// (cugraph_pyg/examples/mag_lp_mnmg.py, GAE's InnerProductDecoder in rgcn_link_class_mnmg.py) and its binary cross-entropy,
//   s_p  = sum_c x_src[i_p, c] x_dst[j_p, c]
//   loss = sum_p w_p (max(s_p, 0) - s_p y_p + log1p(exp(-|s_p|)))   (/ sum_p w_p for the mean)
//   c_p  = w_p (sigmoid(s_p) - y_p)                                  (kept for the backward, sum_p w_p behind it)
// torch spends seven or so launches and two gathered [P, C] copies on it, and its backward scatters with float atomics.  Here
// the forward is ONE launch (a lane group per pair, several pairs in flight per group, the loss added up in workgroup order by
// the last workgroup to finish — the ticket of wg_xent.hip), and the backward is ONE launch per side over that side's incidence
// list (pairs grouped by row, in pair order): out[r] = scale * sum_k coef[pair[k]] x[other(pair[k])] (+ acc[r]).  The list is cut
// into chunks of kChunkEntries entries, a lane group per chunk, whatever rows the chunk covers: a row that lies inside one chunk
// is written at once; the pieces of a row that crosses chunks go to a workspace and are added in chunk order by whichever
// lane group finishes the row's last piece — so a hub's list of thousands of pairs costs what its pieces cost side by side, and
// every sum has a fixed order: no float atomics, run-to-run bit-identical.
// A pair with an index outside its table reads nothing: its score is NaN (so is the loss), its coefficient 0.
#include "wg_common.hpp"
#include "wg_link_parts.hpp"
#include "wgamd_ext.h"

namespace wgamd {
namespace {

constexpr int kPairsInFlight = 4;    // pairs a lane group of the forward has in flight
constexpr int kChunkEntries  = 64;   // entries of an incidence list per lane group

template <int VEC>
struct cols {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ cols<VEC> load_cols(const float* p)
{
  cols<VEC> r;
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void store_cols(float* p, const cols<VEC>& r)
{
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
    *p = r.v[0];
  }
}

// state (BCE only): as bce_finish (wg_link_parts.hpp) lays it out
template <int VEC, bool BCE>
__global__ void __launch_bounds__(kLinkThreads)
pair_fwd_kernel(const float* __restrict__ xs, int64_t lds, int64_t n_src, const float* __restrict__ xd, int64_t ldd, int64_t n_dst, int C,
                const int64_t* __restrict__ isrc, const int64_t* __restrict__ idst, int64_t P, const float* __restrict__ label,
                const float* __restrict__ weight, float* __restrict__ score, float* __restrict__ coef, float* __restrict__ state,
                float* __restrict__ loss_out, int mean, int lg2)
{
  constexpr int U = kPairsInFlight;
  const int LG = 1 << lg2, sub = threadIdx.x & (LG - 1);
  const int64_t per_block = kLinkThreads >> lg2;
  const int64_t group = threadIdx.x >> lg2, wave_group = (threadIdx.x & ~63) >> lg2;
  const int64_t stride = (int64_t)gridDim.x * per_block * U;
  float loss = 0.f, wsum = 0.f;
  // (the loop bound is the wave's, not the lane group's: every lane of a wave takes part in the shuffles below)
  for (int64_t wave0 = ((int64_t)blockIdx.x * per_block + wave_group) * U; wave0 < P; wave0 += stride) {
    const int64_t p0 = wave0 + (group - wave_group) * U;
    int64_t i[U], j[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const bool live = p0 + u < P;
      i[u]  = live ? isrc[p0 + u] : -1;
      j[u]  = live ? idst[p0 + u] : -1;
      ok[u] = i[u] >= 0 && i[u] < n_src && j[u] >= 0 && j[u] < n_dst;
    }
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; u++) acc[u] = 0.f;
    for (int c = sub * VEC; c < C; c += LG * VEC) {
      cols<VEC> a[U], b[U];
#pragma unroll
      for (int u = 0; u < U; u++) {   // 2 U row reads in flight
        a[u] = ok[u] ? load_cols<VEC>(xs + i[u] * lds + c) : cols<VEC>{};
        b[u] = ok[u] ? load_cols<VEC>(xd + j[u] * ldd + c) : cols<VEC>{};
      }
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[u] += a[u].v[q] * b[u].v[q];
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      for (int d = LG >> 1; d >= 1; d >>= 1) acc[u] += __shfl_xor(acc[u], d, 64);
    // lane `sub` of the group finishes pair u0 + sub
    for (int u0 = 0; u0 < U; u0 += LG) {
      const int u = u0 + sub;
      float s = acc[0];
      bool good = ok[0];
#pragma unroll
      for (int q = 1; q < U; q++) {
        s    = u == q ? acc[q] : s;
        good = u == q ? ok[q] : good;
      }
      const int64_t p = p0 + u;
      if (u < U && p < P) {
        s = good ? s : __builtin_nanf("");
        if (score) score[p] = s;
        if constexpr (BCE) coef[p] = bce_pair(s, good, label[p], weight ? weight[p] : 1.f, loss, wsum);
      }
    }
  }
  if constexpr (BCE) bce_finish(loss, wsum, state, coef, P, loss_out, mean);
}

// One side's gradient over its incidence list (row_ptr, pair): the lane group (>= 16 lanes) of chunk ch sums entries
// [ch K, (ch + 1) K).  It first puts the chunk's entries — row, other side's row (-1: the pair adds nothing), coefficient — into
// LDS, all lanes side by side, so that the walk over the entries depends on no global load but the rows of x themselves, eight
// of them in flight; a chunk of short rows (a link group: about one pair per row) then costs eight round trips, not one per row.
// blockIdx.y: the block of 64 VEC columns this workgroup covers (its own counters; the pieces are column-disjoint).
template <int VEC>
__global__ void __launch_bounds__(kLinkThreads)
pair_grad_kernel(const int* __restrict__ row_ptr, const int* __restrict__ pair, int64_t n_rows, int64_t E,
                 const int64_t* __restrict__ idx_row, const int64_t* __restrict__ idx_other, const float* __restrict__ coef,
                 const float* __restrict__ x, int64_t ldx, int64_t n_other, int C, const float* __restrict__ scale_num,
                 const float* __restrict__ scale_den, const float* acc, int64_t lda, float* out, int64_t ldo, float* partial,
                 int64_t ldp, int* counters, int64_t n_chunks, int lg2)
{
  constexpr int U = 8, K = kChunkEntries, kMaxGroups = kLinkThreads / 16;
  __shared__ int s_row[kMaxGroups][K], s_other[kMaxGroups][K];
  __shared__ float s_cf[kMaxGroups][K];
  const int LG = 1 << lg2, sub = threadIdx.x & (LG - 1), lane0 = (threadIdx.x & 63) & ~(LG - 1);
  const int per_block = kLinkThreads >> lg2, group = threadIdx.x >> lg2;
  const int c = ((int)blockIdx.y * LG + sub) * VEC;
  const bool mine = c < C;
  const float scale = (scale_num ? *scale_num : 1.f) / (scale_den ? *scale_den : 1.f);
  int* count = counters + (int64_t)blockIdx.y * n_chunks;
  const int* my_row   = s_row[group];
  const int* my_other = s_other[group];
  const float* my_cf  = s_cf[group];

  // a piece of row r = [rb, re) that crosses chunks: slot 2 ch when the row began before chunk ch, 2 ch + 1 when it begins there
  auto cross = [&](int64_t ch, int64_t r, int64_t rb, int64_t re, const cols<VEC>& t) {
    if (mine) store_cols<VEC>(partial + (2 * ch + (rb < ch * K ? 0 : 1)) * ldp + c, t);
    __threadfence();
    const int64_t ca = rb / K, cb = (re - 1) / K;
    int old = 0;
    if (sub == 0) old = atomicAdd(&count[ca], 1);
    old = __shfl(old, lane0, 64);
    if (old != (int)(cb - ca)) return;
    // the row's last piece to arrive adds them all, in chunk order
    if (sub == 0) count[ca] = 0;   // (reusable without a memset)
    __threadfence();
    if (!mine) return;
    cols<VEC> sum{};
#pragma unroll 4
    for (int64_t cc = ca; cc <= cb; cc++) {
      const float* piece = partial + (2 * cc + (rb < cc * K ? 0 : 1)) * ldp + c;
#pragma unroll
      for (int q = 0; q < VEC; q++) sum.v[q] += __hip_atomic_load(piece + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    cols<VEC> a{};
    if (acc) a = load_cols<VEC>(acc + r * lda + c);
#pragma unroll
    for (int q = 0; q < VEC; q++) sum.v[q] = scale * sum.v[q] + a.v[q];
    store_cols<VEC>(out + r * ldo + c, sum);
  };

  // (the loop bound is the workgroup's: every thread reaches the barriers)
  for (int64_t base = (int64_t)blockIdx.x * per_block; base < n_chunks; base += (int64_t)gridDim.x * per_block) {
    const int64_t ch = base + group, cs = ch * K;
    const int n = ch < n_chunks ? (int)(min(cs + K, E) - cs) : 0;
    __syncthreads();
    for (int e = sub; e < n; e += LG) {
      const int64_t p  = min(max((int64_t)pair[cs + e], (int64_t)0), E - 1);
      const int64_t ir = idx_row[p], io = idx_other[p];
      const int64_t r  = min(max(ir, (int64_t)0), n_rows - 1);   // (the list is built over the clamped indices)
      const bool ok    = ir == r && io >= 0 && io < n_other;
      s_row[group][e]   = (int)r;
      s_other[group][e] = ok ? (int)io : -1;
      s_cf[group][e]    = ok ? coef[p] : 0.f;
    }
    __syncthreads();
    if (n == 0) continue;
    const int r_first = my_row[0], r_last = my_row[n - 1];
    const int64_t rb_first = row_ptr[r_first], re_last = row_ptr[r_last + 1];
    const bool before = rb_first < cs, after = re_last > cs + n;
    cols<VEC> t{}, t_head{}, t_tail{};
    int seg = 0, head_end = 0, tail_start = 0;
    bool have_head = false, have_tail = false;
    for (int e0 = 0; e0 < n; e0 += U) {
      int r[U];
      float cf[U];
      bool last[U];
      cols<VEC> xv[U], av[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int e     = e0 + u;
        const bool live = e < n;
        r[u]            = live ? my_row[e] : -1;
        const int o     = live ? my_other[e] : -1;
        cf[u]           = live ? my_cf[e] : 0.f;
        last[u]         = live && (e + 1 == n || my_row[e + 1] != r[u]);
        xv[u]           = o >= 0 && mine ? load_cols<VEC>(x + (int64_t)o * ldx + c) : cols<VEC>{};
        av[u]           = last[u] && acc && mine ? load_cols<VEC>(acc + (int64_t)r[u] * lda + c) : cols<VEC>{};
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int e = e0 + u;
        if (e >= n) break;
#pragma unroll
        for (int q = 0; q < VEC; q++) t.v[q] += cf[u] * xv[u].v[q];
        if (!last[u]) continue;
        if (seg == 0 && before) {           // the row began in an earlier chunk
          t_head = t, head_end = e + 1, have_head = true;
        } else if (e + 1 == n && after) {   // the row goes on in the next chunk
          t_tail = t, tail_start = seg, have_tail = true;
        } else if (mine) {                  // a row inside this chunk: written at once
          cols<VEC> o;
#pragma unroll
          for (int q = 0; q < VEC; q++) o.v[q] = scale * t.v[q] + av[u].v[q];
          store_cols<VEC>(out + (int64_t)r[u] * ldo + c, o);
        }
        t   = cols<VEC>{};
        seg = e + 1;
      }
    }
    if (have_head) cross(ch, r_first, rb_first, head_end == n ? re_last : cs + head_end, t_head);
    if (have_tail) cross(ch, r_last, cs + tail_start, re_last, t_tail);
  }
  // rows no pair touches: zeros (or what was there to add to)
  if (mine && !(acc && acc == out && lda == ldo)) {
    for (int64_t r = (int64_t)blockIdx.x * per_block + group; r < n_rows; r += (int64_t)gridDim.x * per_block) {
      if (row_ptr[r] == row_ptr[r + 1]) store_cols<VEC>(out + r * ldo + c, acc ? load_cols<VEC>(acc + r * lda + c) : cols<VEC>{});
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int lanes_log2(int lanes)
{
  int l = 0;
  while ((1 << l) < lanes && l < 6) l++;
  return l;
}

inline int fwd_grid(int64_t P, int lg2)
{
  const int64_t per_block = (int64_t)(kLinkThreads >> lg2) * kPairsInFlight;
  return (int)std::max<int64_t>(1, std::min<int64_t>((P + per_block - 1) / per_block, kLinkMaxGrid));
}

inline int64_t chunks_of(int64_t n_pairs) { return (n_pairs + kChunkEntries - 1) / kChunkEntries; }
inline int col_blocks(int C, int vec) { return (C + 64 * vec - 1) / (64 * vec); }
inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }
// the counters are sized for the scalar-load route (the more column blocks)
inline size_t counter_bytes(int64_t n_pairs, int C) { return pad256(sizeof(int) * (size_t)chunks_of(n_pairs) * (size_t)col_blocks(C, 1)); }

void pair_forward(bool bce, const float* xs, int64_t lds, int64_t n_src, const float* xd, int64_t ldd, int64_t n_dst, int C,
                  const int64_t* isrc, const int64_t* idst, int64_t P, const float* label, const float* weight, float* score,
                  float* coef, float* state, float* loss_out, int mean, hipStream_t st)
{
  const bool v4 = C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned16(xs) && aligned16(xd);
  const int lg2 = lanes_log2(v4 ? C / 4 : C);
  const int grid = fwd_grid(P, lg2);
#define WG_PAIR_FWD(VEC, BCE) \
  pair_fwd_kernel<VEC, BCE><<<grid, kLinkThreads, 0, st>>>(xs, lds, n_src, xd, ldd, n_dst, C, isrc, idst, P, label, weight, score, \
                                                          coef, state, loss_out, mean, lg2)
  if (bce) {
    if (v4) WG_PAIR_FWD(4, true); else WG_PAIR_FWD(1, true);
  } else {
    if (v4) WG_PAIR_FWD(4, false); else WG_PAIR_FWD(1, false);
  }
#undef WG_PAIR_FWD
  WG_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace wgamd

extern "C" {

size_t wgamd_pair_bce_state_bytes(int64_t n_pairs)
{
  (void)n_pairs;   // (the grid is bounded: one size for every call, so one state serves them all)
  return sizeof(float) * (size_t)(4 + 2 * wgamd::kLinkMaxGrid) + 16;
}

wholememory_error_code_t wgamd_pair_dot_forward_f32(const float* x_src, int64_t ld_src, int64_t n_src, const float* x_dst,
                                                    int64_t ld_dst, int64_t n_dst, int n_cols, const int64_t* index_src,
                                                    const int64_t* index_dst, int64_t n_pairs, float* score, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pair_dot_forward_f32", [&] {
    WG_REQUIRE_INPUT(n_pairs >= 0 && n_src >= 0 && n_dst >= 0 && n_cols >= 1 && ld_src >= n_cols && ld_dst >= n_cols, "bad shape");
    if (n_pairs == 0) return;
    WG_REQUIRE_INPUT(index_src && index_dst && score && (x_src || n_src == 0) && (x_dst || n_dst == 0), "null pointer");
    pair_forward(false, x_src, ld_src, n_src, x_dst, ld_dst, n_dst, n_cols, index_src, index_dst, n_pairs, nullptr, nullptr, score,
                 nullptr, nullptr, nullptr, 0, static_cast<hipStream_t>(stream));
  });
}

wholememory_error_code_t wgamd_pair_bce_forward_f32(const float* x_src, int64_t ld_src, int64_t n_src, const float* x_dst,
                                                    int64_t ld_dst, int64_t n_dst, int n_cols, const int64_t* index_src,
                                                    const int64_t* index_dst, int64_t n_pairs, const float* label,
                                                    const float* pair_weight, int mean, float* score, float* coef, void* state,
                                                    int state_is_zeroed, float* loss_out, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pair_bce_forward_f32", [&] {
    WG_REQUIRE_INPUT(n_pairs >= 1 && n_src >= 0 && n_dst >= 0 && n_cols >= 1 && ld_src >= n_cols && ld_dst >= n_cols, "bad shape");
    WG_REQUIRE_INPUT(index_src && index_dst && label && coef && state && loss_out && (x_src || n_src == 0) && (x_dst || n_dst == 0),
                     "null pointer");
    auto st = static_cast<hipStream_t>(stream);
    if (!state_is_zeroed) WG_HIP_CHECK(hipMemsetAsync(state, 0, wgamd_pair_bce_state_bytes(n_pairs), st));
    pair_forward(true, x_src, ld_src, n_src, x_dst, ld_dst, n_dst, n_cols, index_src, index_dst, n_pairs, label, pair_weight, score,
                 coef, static_cast<float*>(state), loss_out, mean, st);
  });
}

size_t wgamd_pair_grad_workspace_bytes(int64_t n_pairs, int n_cols)
{
  using namespace wgamd;
  if (n_pairs < 0 || n_cols <= 0) return 0;
  const size_t ldp = ((size_t)n_cols + 3) / 4 * 4;
  return 256 + counter_bytes(n_pairs, n_cols) + 2 * (size_t)chunks_of(n_pairs) * ldp * sizeof(float) + 256;
}

wholememory_error_code_t wgamd_pair_grad_f32(const int* row_ptr, const int* pair, int64_t n_rows, int64_t n_pairs,
                                             const int64_t* index_row, const int64_t* index_other, const float* coef,
                                             const float* x_other, int64_t ld_other, int64_t n_other, int n_cols,
                                             const float* scale_num, const float* scale_den, const float* acc, int64_t ld_acc,
                                             float* out, int64_t ld_out, void* workspace, size_t workspace_bytes,
                                             int counters_are_zeroed, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pair_grad_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && n_pairs >= 0 && n_other >= 0 && n_cols >= 1 && ld_other >= n_cols && ld_out >= n_cols &&
                       (acc == nullptr || ld_acc >= n_cols) && n_pairs < ((int64_t)1 << 31) && n_rows < ((int64_t)1 << 31) &&
                       n_other < ((int64_t)1 << 31),
                     "bad shape");
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && out && (n_pairs == 0 || (pair && index_row && index_other && coef && workspace)) &&
                       (x_other || n_other == 0),
                     "null pointer");
    WG_REQUIRE_INPUT(n_pairs == 0 || workspace_bytes >= wgamd_pair_grad_workspace_bytes(n_pairs, n_cols), "workspace too small");
    auto st               = static_cast<hipStream_t>(stream);
    const int64_t ldp     = ((int64_t)n_cols + 3) / 4 * 4;
    const int64_t n_chunk = chunks_of(n_pairs);
    char* ws       = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
    int* counters  = reinterpret_cast<int*>(ws);
    float* partial = reinterpret_cast<float*>(ws + counter_bytes(n_pairs, n_cols));
    if (n_pairs > 0 && !counters_are_zeroed) WG_HIP_CHECK(hipMemsetAsync(counters, 0, counter_bytes(n_pairs, n_cols), st));
    const bool v4 = n_cols % 4 == 0 && ld_other % 4 == 0 && ld_out % 4 == 0 && (acc == nullptr || ld_acc % 4 == 0) &&
                    aligned16(x_other) && aligned16(out) && aligned16(acc);
    const int vec = v4 ? 4 : 1;
    const int lg2 = std::max(4, lanes_log2((n_cols + vec - 1) / vec));   // (at least 16 lanes a group: its LDS share)
    const int64_t per_block = kLinkThreads >> lg2;
    const int64_t want      = std::max<int64_t>((n_chunk + per_block - 1) / per_block, (n_rows + 8 * per_block - 1) / (8 * per_block));
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, kLinkMaxGrid)), (unsigned)col_blocks(n_cols, vec));
    if (v4)
      pair_grad_kernel<4><<<grid, kLinkThreads, 0, st>>>(row_ptr, pair, n_rows, n_pairs, index_row, index_other, coef, x_other, ld_other,
                                                        n_other, n_cols, scale_num, scale_den, acc, ld_acc, out, ld_out, partial, ldp,
                                                        counters, n_chunk, lg2);
    else
      pair_grad_kernel<1><<<grid, kLinkThreads, 0, st>>>(row_ptr, pair, n_rows, n_pairs, index_row, index_other, coef, x_other, ld_other,
                                                        n_other, n_cols, scale_num, scale_den, acc, ld_acc, out, ld_out, partial, ldp,
                                                        counters, n_chunk, lg2);
    WG_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
