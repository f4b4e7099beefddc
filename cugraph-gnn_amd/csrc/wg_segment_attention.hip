// Multi-head self-attention inside the segments of a row table (the global branch of torch_geometric.nn.GPSConv): the n rows
// of q / k / v ([n, H D] views, each with its own row stride, so a packed [n, 3C] in-projection is read in place) are cut into
// consecutive segments by ptr (int64 [n_seg + 1], PyG's Batch.ptr), and row i attends to exactly the rows of its segment:
//     S_ij = (q_i[h] . k_j[h]) scale,   P = softmax over j in the segment of i,   o_i[h] = sum_j P_ij v_j[h]
// A dense block-diagonal pattern: both products run on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
//
// Frame of all three kernels.  Grid = ceil(n / 64) x H; a workgroup of 4 waves owns 64 consecutive rows and one head, a wave
// 16 of them.  The workgroup finds the segments of its first and last row by binary search in ptr and streams 64-row tiles
// of the OTHER side over [start of the first row's segment, end of the last row's segment): two [64 x D16] operands per tile
// (D16 = D rounded up to 16, columns D.. zero), fetched as coalesced float4 into registers while the previous tile is
// multiplied, then put into LDS rows D16 + 4 floats apart (4 banks: both fragment reads below are conflict-free).  No tile
// table, no host read-back; several small graphs in a 16-row tile, a graph over many tiles and empty segments all take the
// same loop, cut by a mask per (row, other row) pair; a wave skips the 16-row sub-tiles outside its own rows' segments.
//
// The score tile is kept TRANSPOSED so that no probability goes through LDS.  With the MFMA's C/D map (col = lane & 15,
// row = 4 (lane >> 4) + reg):
//   * S^T = K Q^T — A = 16 tile rows of K (a float4 of row lane & 15 per 16 columns), B = the wave's own rows of Q, in
//     registers for the whole kernel with scale log2(e) folded in.  A lane then holds four keys (4 g + reg) of ONE query
//     (lane & 15): the softmax statistics m, l are one scalar per lane, reduced over its four registers and two cross-lane
//     steps (xor 16, 32), and the rescale of the output accumulators is one factor per lane.
//   * those registers ARE the B fragments of O^T += V^T P^T: step reg contracts keys 4 g + reg, A = V[key][d0 + (lane & 15)].
//     O^T is D16 / 16 x 4 registers; the epilogue is one float4 store per lane and 16-column block.
//   * segment_attention_bwd_q_kernel: the same frame; dP^T = V dO^T in the same layout, P = exp2(S - lse), dS^T = P (dP -
//     delta) in registers is the B operand of dQ^T += K^T dS^T.  Also writes delta_ih = do_ih . o_ih.
//   * segment_attention_bwd_kv_kernel: key-major, the wave's K and V rows in registers, tiles of Q and dO (and lse, delta)
//     streamed: S = Q K^T has queries on the register axis, P and dS are the B operands of dV^T += dO^T P, dK^T += Q^T dS.
// Every row of o, lse, delta, dq, dk, dv is written exactly once, by plain stores: no atomics, the same bits on every run.
// Every global load is predicated on its row index being below n.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kSegRows = 64;          // rows per workgroup, and rows of a streamed tile
constexpr int kSegMaxH = 8, kSegMaxD = 64, kSegMaxC = 256;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

struct seg_args {
  const float *q, *k, *v;
  int64_t ldq, ldk, ldv;
  const int64_t* ptr;
  int n_seg, n, H, D;
  float scale;
  float* out;                 // forward: written; bwd_q: the forward's o, read
  int64_t ldo;
  float* lse;                 // [n, ld_lse], H used; forward: nullable
  int64_t ld_lse;
  const float* dout;
  int64_t ld_do;
  float* delta;               // [n, ld_delta], H used: written by bwd_q, read by bwd_kv
  int64_t ld_delta;
  float *dq, *dk, *dv;
  int64_t ld_dq, ld_dk, ld_dv;
};

// [s, e): the segment holding row i, clamped to [0, n]; (0, 0) for a row outside [0, n) or outside [ptr[0], ptr[n_seg])
__device__ __forceinline__ void segment_of(const int64_t* ptr, int n_seg, int n, int i, int& s, int& e)
{
  s = e = 0;
  if (i < 0 || i >= n) return;
  int lo = 0, hi = n_seg + 1;                     // the first index of ptr[0 .. n_seg] whose value is above i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] > i) hi = mid; else lo = mid + 1;
  }
  if (lo == 0 || lo > n_seg) return;
  s = (int)std::max<int64_t>(ptr[lo - 1], 0);
  e = (int)std::min<int64_t>(ptr[lo], n);
}

__device__ __forceinline__ float group_max(float v)
{
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

__device__ __forceinline__ float group_sum(float v)
{
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// One thread's share of a streamed tile: NB float4 of each of the two operands, and one float of the row vectors (bwd_kv)
template <int NB>
struct seg_stage {
  f32x4 a[NB], b[NB];
  float x;
};

// rows [r0, r0 + 64) below r_end of the head's columns [col0, col0 + D) of A and B into registers: slot p = tid + 256 u is
// (row p / (4 NB), float4 p % (4 NB)); zeros from r_end on and from column D on
template <int NB>
__device__ __forceinline__ void seg_fetch(seg_stage<NB>& st, const float* A, int64_t lda, const float* B, int64_t ldb, int col0,
                                          int D, int r0, int r_end)
{
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int p = threadIdx.x + kThreads * u, row = p / (4 * NB), c = (p % (4 * NB)) * 4;
    st.a[u] = st.b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r0 + row < r_end && c < D) {
      st.a[u] = *reinterpret_cast<const f32x4*>(A + (int64_t)(r0 + row) * lda + col0 + c);
      st.b[u] = *reinterpret_cast<const f32x4*>(B + (int64_t)(r0 + row) * ldb + col0 + c);
    }
  }
}

template <int NB>
__device__ __forceinline__ void seg_put(const seg_stage<NB>& st, float* ta, float* tb)
{
  constexpr int SD = 16 * NB + 4;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int p = threadIdx.x + kThreads * u, row = p / (4 * NB), c = (p % (4 * NB)) * 4;
    *reinterpret_cast<f32x4*>(ta + row * SD + c) = st.a[u];
    *reinterpret_cast<f32x4*>(tb + row * SD + c) = st.b[u];
  }
}

// T[r0 .. r0 + 15][:] times b^T, contraction over the D16 columns: the result's row = tile row 4 g + reg, column = the lane's
// own row (lane & 15) whose float4s are b
template <int NB>
__device__ __forceinline__ f32x4 seg_rows_dot(const float* tile, int r0, const f32x4 (&b)[NB], int c, int g)
{
  constexpr int SD = 16 * NB + 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(tile + (r0 + c) * SD + 16 * blk + 4 * g);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], b[blk][kk], acc, 0, 0, 0);
  }
  return acc;
}

// acc[blk] += T^T[16 blk .. + 15][r0 .. r0 + 15] times p, contraction over the 16 tile rows: p[reg] belongs to tile row 4 g + reg
template <int NB>
__device__ __forceinline__ void seg_cols_acc(f32x4 (&acc)[NB], const float* tile, int r0, const f32x4& p, int c, int g)
{
  constexpr int SD = 16 * NB + 4;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      acc[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[(r0 + 4 * g + reg) * SD + 16 * blk + c], p[reg], acc[blk], 0, 0, 0);
  }
}

// the lane's own row i of a table, head columns, as NB float4 (block blk = columns 16 blk + 4 g ..): zeros past n and past D
template <int NB>
__device__ __forceinline__ void seg_own_row(f32x4 (&r)[NB], const float* t, int64_t ld, int i, int n, int col0, int D, int g,
                                            float factor)
{
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const int d = 16 * blk + 4 * g;
    r[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < n && d < D) r[blk] = *reinterpret_cast<const f32x4*>(t + (int64_t)i * ld + col0 + d) * factor;
  }
}

template <int NB>
__device__ __forceinline__ void seg_store_row(const f32x4 (&r)[NB], float* t, int64_t ld, int i, int n, int col0, int D, int g,
                                              float factor)
{
  if (i >= n) return;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const int d = 16 * blk + 4 * g;
    if (d < D) *reinterpret_cast<f32x4*>(t + (int64_t)i * ld + col0 + d) = r[blk] * factor;
  }
}

// What a wave knows about its 16 rows: the lane's row i (row lane & 15 of the wave) with its segment [s, e), and the span
// [wlo, whi) of the wave's segments (wave-uniform); [tlo, thi) is the workgroup's span, the range of the streamed tiles
struct seg_frame {
  int lane, c, g, h, col0, i, s, e, wlo, whi, tlo, thi;
};

__device__ __forceinline__ seg_frame seg_make_frame(const seg_args& a)
{
  seg_frame f;
  f.lane = threadIdx.x & 63, f.c = f.lane & 15, f.g = f.lane >> 4;
  f.h = blockIdx.y, f.col0 = f.h * a.D;
  const int row0 = blockIdx.x * kSegRows, last = std::min(row0 + kSegRows, a.n) - 1;
  int unused;
  segment_of(a.ptr, a.n_seg, a.n, row0, f.tlo, unused);
  segment_of(a.ptr, a.n_seg, a.n, last, unused, f.thi);
  f.i = row0 + 16 * (int)(threadIdx.x >> 6) + f.c;
  segment_of(a.ptr, a.n_seg, a.n, f.i, f.s, f.e);
  int hi = f.e;
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) hi = std::max(hi, __shfl_xor(hi, off));
  f.whi = __builtin_amdgcn_readfirstlane(hi);
  f.wlo = __builtin_amdgcn_readfirstlane(f.s);        // (lane 0: the wave's first row; rows ascend, so do their segments)
  return f;
}

template <int NB>
__global__ void __launch_bounds__(kThreads) segment_attention_kernel(seg_args a)
{
  constexpr int SD = 16 * NB + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *kt = lds, *vt = lds + kSegRows * SD;
  const seg_frame f = seg_make_frame(a);
  const int c = f.c, g = f.g;
  f32x4 qb[NB], o[NB];
  seg_own_row<NB>(qb, a.q, a.ldq, f.i, a.n, f.col0, a.D, g, a.scale * kLog2e);
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) o[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // of the lane's query, in base 2

  seg_stage<NB> st;
  if (f.tlo < f.thi) seg_fetch<NB>(st, a.k, a.ldk, a.v, a.ldv, f.col0, a.D, f.tlo, f.thi);
  for (int jt = f.tlo; jt < f.thi; jt += kSegRows) {
    __syncthreads();                                  // (the previous tile has been read)
    seg_put<NB>(st, kt, vt);
    __syncthreads();
    if (jt + kSegRows < f.thi) seg_fetch<NB>(st, a.k, a.ldk, a.v, a.ldv, f.col0, a.D, jt + kSegRows, f.thi);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int j0 = jt + 16 * sub;
      if (j0 + 16 <= f.wlo || j0 >= f.whi) continue;
      f32x4 s = seg_rows_dot<NB>(kt, 16 * sub, qb, c, g);
      float mx = -INFINITY;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int j = j0 + 4 * g + reg;
        s[reg] = (j >= f.s && j < f.e) ? s[reg] : -INFINITY;
        mx = fmaxf(mx, s[reg]);
      }
      const float mn = fmaxf(m, group_max(mx));
      const float ms = mn == -INFINITY ? 0.f : mn;    // (no key of the query's segment so far: exp2(-inf - 0) = 0, never inf - inf)
      const float rs = exp2f(m - ms);
      f32x4 p;
      float ps = 0.f;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        p[reg] = exp2f(s[reg] - ms);
        ps += p[reg];
      }
      l = l * rs + group_sum(ps);
      m = mn;
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) o[blk] *= rs;
      seg_cols_acc<NB>(o, vt, 16 * sub, p, c, g);
    }
  }
  seg_store_row<NB>(o, a.out, a.ldo, f.i, a.n, f.col0, a.D, g, l > 0.f ? 1.f / l : 0.f);
  if (a.lse && f.i < a.n && g == 0) a.lse[(int64_t)f.i * a.ld_lse + f.h] = l > 0.f ? (m + log2f(l)) * kLn2 : 0.f;
}

template <int NB>
__global__ void __launch_bounds__(kThreads) segment_attention_bwd_q_kernel(seg_args a)
{
  constexpr int SD = 16 * NB + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *kt = lds, *vt = lds + kSegRows * SD;
  const seg_frame f = seg_make_frame(a);
  const int c = f.c, g = f.g;
  f32x4 qb[NB], dob[NB], ob[NB], dq[NB];
  seg_own_row<NB>(qb, a.q, a.ldq, f.i, a.n, f.col0, a.D, g, a.scale * kLog2e);
  seg_own_row<NB>(dob, a.dout, a.ld_do, f.i, a.n, f.col0, a.D, g, 1.f);
  seg_own_row<NB>(ob, a.out, a.ldo, f.i, a.n, f.col0, a.D, g, 1.f);
  float dl = 0.f;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    dq[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) dl += dob[blk][t] * ob[blk][t];
  }
  dl = group_sum(dl);
  float lse2 = 0.f;
  if (f.i < a.n) {
    lse2 = a.lse[(int64_t)f.i * a.ld_lse + f.h] * kLog2e;
    if (g == 0) a.delta[(int64_t)f.i * a.ld_delta + f.h] = dl;
  }

  seg_stage<NB> st;
  if (f.tlo < f.thi) seg_fetch<NB>(st, a.k, a.ldk, a.v, a.ldv, f.col0, a.D, f.tlo, f.thi);
  for (int jt = f.tlo; jt < f.thi; jt += kSegRows) {
    __syncthreads();
    seg_put<NB>(st, kt, vt);
    __syncthreads();
    if (jt + kSegRows < f.thi) seg_fetch<NB>(st, a.k, a.ldk, a.v, a.ldv, f.col0, a.D, jt + kSegRows, f.thi);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int j0 = jt + 16 * sub;
      if (j0 + 16 <= f.wlo || j0 >= f.whi) continue;
      const f32x4 s = seg_rows_dot<NB>(kt, 16 * sub, qb, c, g);
      const f32x4 dp = seg_rows_dot<NB>(vt, 16 * sub, dob, c, g);
      f32x4 ds;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int j = j0 + 4 * g + reg;
        const float p = (j >= f.s && j < f.e) ? exp2f(s[reg] - lse2) : 0.f;
        ds[reg] = p * (dp[reg] - dl);
      }
      seg_cols_acc<NB>(dq, kt, 16 * sub, ds, c, g);
    }
  }
  seg_store_row<NB>(dq, a.dq, a.ld_dq, f.i, a.n, f.col0, a.D, g, a.scale);
}

template <int NB>
__global__ void __launch_bounds__(kThreads) segment_attention_bwd_kv_kernel(seg_args a)
{
  constexpr int SD = 16 * NB + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *qt = lds, *dot = lds + kSegRows * SD, *lse_t = lds + 2 * kSegRows * SD, *delta_t = lse_t + kSegRows;
  const seg_frame f = seg_make_frame(a);              // (the lane's row is a KEY here, the streamed rows are queries)
  const int c = f.c, g = f.g, tid = threadIdx.x;
  f32x4 kb[NB], vb[NB], dk[NB], dv[NB];
  seg_own_row<NB>(kb, a.k, a.ldk, f.i, a.n, f.col0, a.D, g, a.scale * kLog2e);
  seg_own_row<NB>(vb, a.v, a.ldv, f.i, a.n, f.col0, a.D, g, 1.f);
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) dk[blk] = dv[blk] = f32x4{0.f, 0.f, 0.f, 0.f};

  // threads 0 .. 63 carry the tile's lse (base 2), threads 64 .. 127 its delta
  auto fetch_vec = [&](int r0) {
    const int r = r0 + (tid & 63);
    float x = 0.f;
    if (tid < 2 * kSegRows && r < f.thi)
      x = tid < kSegRows ? a.lse[(int64_t)r * a.ld_lse + f.h] * kLog2e : a.delta[(int64_t)r * a.ld_delta + f.h];
    return x;
  };
  seg_stage<NB> st;
  if (f.tlo < f.thi) {
    seg_fetch<NB>(st, a.q, a.ldq, a.dout, a.ld_do, f.col0, a.D, f.tlo, f.thi);
    st.x = fetch_vec(f.tlo);
  }
  for (int it = f.tlo; it < f.thi; it += kSegRows) {
    __syncthreads();
    seg_put<NB>(st, qt, dot);
    if (tid < 2 * kSegRows) lse_t[tid] = st.x;       // (delta_t = lse_t + 64)
    __syncthreads();
    if (it + kSegRows < f.thi) {
      seg_fetch<NB>(st, a.q, a.ldq, a.dout, a.ld_do, f.col0, a.D, it + kSegRows, f.thi);
      st.x = fetch_vec(it + kSegRows);
    }
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int i0 = it + 16 * sub;
      if (i0 + 16 <= f.wlo || i0 >= f.whi) continue;
      const f32x4 s = seg_rows_dot<NB>(qt, 16 * sub, kb, c, g);
      const f32x4 dp = seg_rows_dot<NB>(dot, 16 * sub, vb, c, g);
      const f32x4 ls = *reinterpret_cast<const f32x4*>(lse_t + 16 * sub + 4 * g);
      const f32x4 dl = *reinterpret_cast<const f32x4*>(delta_t + 16 * sub + 4 * g);
      f32x4 p, ds;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + 4 * g + reg;
        p[reg] = (i >= f.s && i < f.e) ? exp2f(s[reg] - ls[reg]) : 0.f;
        ds[reg] = p[reg] * (dp[reg] - dl[reg]);
      }
      seg_cols_acc<NB>(dv, dot, 16 * sub, p, c, g);
      seg_cols_acc<NB>(dk, qt, 16 * sub, ds, c, g);
    }
  }
  seg_store_row<NB>(dk, a.dk, a.ld_dk, f.i, a.n, f.col0, a.D, g, a.scale);
  seg_store_row<NB>(dv, a.dv, a.ld_dv, f.i, a.n, f.col0, a.D, g, 1.f);
}

bool seg_shape_ok(int H, int D)
{
  return H >= 1 && H <= kSegMaxH && D >= 4 && D <= kSegMaxD && D % 4 == 0 && H * D <= kSegMaxC;
}

// the checks every entry point shares, and the operands every kernel reads; false: nothing to launch
bool seg_take(seg_args& a, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* ptr,
              int64_t n_seg, int64_t n, int H, int D, float scale)
{
  WG_REQUIRE_INPUT(n >= 0 && n_seg >= 0 && n <= INT32_MAX - 2 * kSegRows && n_seg < INT32_MAX, "bad sizes");
  if (!seg_shape_ok(H, D))
    throw logic_error(fmt("unsupported shape: H=%d (1 .. %d), D=%d (a multiple of 4, 4 .. %d), H D <= %d", H, kSegMaxH, D, kSegMaxD,
                          kSegMaxC));
  if (n == 0) return false;
  WG_REQUIRE_INPUT(q && k && v && ptr, "null pointer");
  WG_REQUIRE_INPUT(ldq >= H * D && ldk >= H * D && ldv >= H * D, "leading dimension too small");
  WG_REQUIRE_INPUT(scale == scale && scale - scale == 0.f, "scale must be finite");
  if (!aligned_rows(q, ldq) || !aligned_rows(k, ldk) || !aligned_rows(v, ldv)) throw logic_error("q / k / v rows must be 16-B aligned");
  a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv, a.ptr = ptr, a.n_seg = (int)n_seg, a.n = (int)n, a.H = H, a.D = D;
  a.scale = scale;
  return true;
}

// kern<NB>(a) over ceil(n / 64) x H workgroups, NB = D16 / 16; extra floats of LDS behind the two [64 x (D16 + 4)] tiles
#define WG_SEG_LAUNCH(kern, a, extra, stream)                                                          \
  do {                                                                                                 \
    const dim3 grid((unsigned)((a.n + kSegRows - 1) / kSegRows), (unsigned)a.H);                       \
    const int nb = (a.D + 15) / 16;                                                                    \
    const size_t lds = ((size_t)2 * kSegRows * (16 * nb + 4) + (extra)) * 4; /* at most 35.3 KB */      \
    auto st = static_cast<hipStream_t>(stream);                                                        \
    switch (nb) {                                                                                      \
      case 1: kern<1><<<grid, kThreads, lds, st>>>(a); break;                                          \
      case 2: kern<2><<<grid, kThreads, lds, st>>>(a); break;                                          \
      case 3: kern<3><<<grid, kThreads, lds, st>>>(a); break;                                          \
      default: kern<4><<<grid, kThreads, lds, st>>>(a); break;                                         \
    }                                                                                                  \
    WG_HIP_CHECK(hipGetLastError());                                                                   \
  } while (0)

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_segment_attention_supported(int H, int D) { return wgamd::seg_shape_ok(H, D); }

extern "C" wholememory_error_code_t wgamd_segment_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                                                int64_t ldv, const int64_t* ptr, int64_t n_seg, int64_t n, int H, int D,
                                                                float scale, float* out, int64_t ldo, float* lse_out, int64_t ld_lse,
                                                                void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_segment_attention_f32", [&] {
    seg_args a{};
    if (!seg_take(a, q, ldq, k, ldk, v, ldv, ptr, n_seg, n, H, D, scale)) return;
    WG_REQUIRE_INPUT(out, "null pointer");
    WG_REQUIRE_INPUT(ldo >= H * D && (lse_out == nullptr || ld_lse >= H), "leading dimension too small");
    if (!aligned_rows(out, ldo)) throw logic_error("out rows must be 16-B aligned");
    a.out = out, a.ldo = ldo, a.lse = lse_out, a.ld_lse = ld_lse;
    WG_SEG_LAUNCH(segment_attention_kernel, a, 0, stream);
  });
}

extern "C" wholememory_error_code_t wgamd_segment_attention_bwd_q_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                                                      const float* v, int64_t ldv, const int64_t* ptr, int64_t n_seg,
                                                                      int64_t n, int H, int D, float scale, const float* dout,
                                                                      int64_t ld_do, const float* out, int64_t ldo, const float* lse,
                                                                      int64_t ld_lse, float* dq, int64_t ld_dq, float* delta,
                                                                      int64_t ld_delta, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_segment_attention_bwd_q_f32", [&] {
    seg_args a{};
    if (!seg_take(a, q, ldq, k, ldk, v, ldv, ptr, n_seg, n, H, D, scale)) return;
    WG_REQUIRE_INPUT(dout && out && lse && dq && delta, "null pointer");
    WG_REQUIRE_INPUT(ld_do >= H * D && ldo >= H * D && ld_dq >= H * D && ld_lse >= H && ld_delta >= H, "leading dimension too small");
    if (!aligned_rows(dout, ld_do) || !aligned_rows(out, ldo) || !aligned_rows(dq, ld_dq))
      throw logic_error("dout / out / dq rows must be 16-B aligned");
    a.dout = dout, a.ld_do = ld_do, a.out = const_cast<float*>(out), a.ldo = ldo, a.lse = const_cast<float*>(lse), a.ld_lse = ld_lse;
    a.dq = dq, a.ld_dq = ld_dq, a.delta = delta, a.ld_delta = ld_delta;
    WG_SEG_LAUNCH(segment_attention_bwd_q_kernel, a, 0, stream);
  });
}

extern "C" wholememory_error_code_t wgamd_segment_attention_bwd_kv_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                                                       const float* v, int64_t ldv, const int64_t* ptr, int64_t n_seg,
                                                                       int64_t n, int H, int D, float scale, const float* dout,
                                                                       int64_t ld_do, const float* lse, int64_t ld_lse,
                                                                       const float* delta, int64_t ld_delta, float* dk, int64_t ld_dk,
                                                                       float* dv, int64_t ld_dv, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_segment_attention_bwd_kv_f32", [&] {
    seg_args a{};
    if (!seg_take(a, q, ldq, k, ldk, v, ldv, ptr, n_seg, n, H, D, scale)) return;
    WG_REQUIRE_INPUT(dout && lse && delta && dk && dv, "null pointer");
    WG_REQUIRE_INPUT(ld_do >= H * D && ld_dk >= H * D && ld_dv >= H * D && ld_lse >= H && ld_delta >= H, "leading dimension too small");
    if (!aligned_rows(dout, ld_do) || !aligned_rows(dk, ld_dk) || !aligned_rows(dv, ld_dv))
      throw logic_error("dout / dk / dv rows must be 16-B aligned");
    a.dout = dout, a.ld_do = ld_do, a.lse = const_cast<float*>(lse), a.ld_lse = ld_lse, a.delta = const_cast<float*>(delta);
    a.ld_delta = ld_delta, a.dk = dk, a.ld_dk = ld_dk, a.dv = dv, a.ld_dv = ld_dv;
    WG_SEG_LAUNCH(segment_attention_bwd_kv_kernel, a, 2 * kSegRows, stream);
  });
}
