// Grouped Linear: the dense products around the heterogeneous layers (one Linear per node type: PyG's HeteroLinear /
// HeteroDictLinear, pyg_lib.segment_matmul / grouped_matmul) — up to 16 segments in ONE launch:
//     out_s[place(i), :] = act( X_s[list(i), :] @ W_s + b_s + add_s[i, :] )      i < n_rows_s
// X_s read by row or through an int64 list, W_s through two element strides (ld_n, ld_k), one of them 1: torch.nn.Linear's
// [N, K], HeteroLinear's [K, N], and either one transposed (the dX product of the backward runs on the same kernel).
//
// Pieces:
//   * grouped_linear_kernel<NT> — a real GEMM frame, unlike the layer kernels' tile_times: a workgroup owns 64 rows of one
//     segment and a column block of 16 NT <= 256 columns; it finds (segment, row tile) by walking the descriptors' tile counts
//     (at most 16 uniform steps).  K is streamed in panels of 32: the [64 x 32] panel of X and the [16 NT x 32] panel of W go
//     into LDS ONCE per workgroup, both as rows of 32 k + 4 floats (the weight as [n][k] whichever way it lies in memory), and
//     the four waves share them; the next panel waits in registers while the current one is multiplied.  Wave w owns rows
//     16 w .. 16 w + 15 and all NT column tiles: NT f32x4 accumulators on v_mfma_f32_16x16x4_f32, one ds_read_b128 of X and NT
//     of W per 16 k and 4 NT MFMAs.  The epilogue (bias, add, ReLU, placed store) goes straight from the accumulator layout.
//     With act_out the value of X at (row, column) counts as 0 where act_out there is not > 0: the ReLU mask of the backward,
//     applied while staging.
//   * grouped_linear_wgrad_kernel — a work item is (segment, 64 x 64 block of the weight, row range): dW[k, n] = sum over the
//     range's rows of X[list(i), k] dY[place(i), n] (dY masked by act_out).  Panels of 64 rows of both operands in LDS (rows of
//     64 + 4 floats), read as TRANSPOSED fragments (the contraction runs over rows); wave w owns k rows 16 w .. 16 w + 15 of
//     the block, 4 accumulators.  The block's partial goes to a workspace; items of k block 0 add the column sums of the masked
//     dY (in registers while staging, then over the 16 row groups in group order through LDS).
//   * grouped_linear_reduce_kernel adds the partials in range order and writes dW through (ld_n, ld_k), db beside it.
// No atomics anywhere, and the split into row ranges depends on the shapes only: the same bits on every run.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kGlSegs = WGAMD_GROUPED_LINEAR_MAX_SEGMENTS;
constexpr int kGlRows = 64;              // rows per workgroup: 16 per wave
constexpr int kGlKP   = 32;              // k per panel
constexpr int kGlS    = kGlKP + 4;       // floats between two panel rows in LDS: (32 + 4) / 4 odd, see DESIGN 3.34
constexpr int kGlKV   = kGlKP / 4;       // float4 per panel row
constexpr int kGwRows = 64, kGwBlk = 64; // wgrad: rows per panel, block edge
constexpr int kGwS    = kGwBlk + 4;
constexpr int kGwV    = kGwRows * kGwBlk / 4 / kThreads;      // float4 per thread, panel and operand: 4
constexpr int kGwMaxRanges = 256;
constexpr int64_t kGwRangeRows = 1024;                      // rows per range at least (before the caps)
constexpr int64_t kGwSegBytes = int64_t(32) << 20;          // partial blocks of one segment at most

struct gl_seg {
  const float* x;
  const int64_t* ids;
  const float* w;
  const float* bias;
  const float* add;
  float* out;
  const int64_t* out_rows;
  const float* act;
  int64_t ldx, ld_n, ld_k, ld_add, ldo, ld_act, n_rows;
  int K, N;
};

struct gl_args {
  gl_seg s[kGlSegs];
  int n_segs, relu;
};

struct gw_seg {
  const float* x;
  const int64_t* ids;
  const float* g;
  const int64_t* g_rows;
  const float* act;
  float* dw;
  float* db;
  int64_t ldx, ldg, ld_act, ld_n, ld_k, n_rows;
  int K, N;
};

struct gw_args {
  gw_seg s[kGlSegs];
  int n_segs;
  float* ws;
};

// The row ranges of a segment's weight gradient: `ranges` ranges of `len` rows (a multiple of 64; the last may be short).  A
// function of the shapes only.
__host__ __device__ inline void wgrad_split(int64_t n_rows, int K, int N, int& ranges, int64_t& len)
{
  ranges = 0, len = 0;
  if (n_rows <= 0) return;
  int64_t cap = kGwSegBytes / ((int64_t)K * N * 4);
  cap = cap < 1 ? 1 : cap > kGwMaxRanges ? kGwMaxRanges : cap;
  int64_t r = (n_rows + kGwRangeRows - 1) / kGwRangeRows;
  r = r > cap ? cap : r;
  len = ((n_rows + r - 1) / r + kGwRows - 1) / kGwRows * kGwRows;
  ranges = (int)((n_rows + len - 1) / len);
}

__host__ __device__ inline int64_t wgrad_items(const gw_seg& s, int ranges)
{
  return s.dw == nullptr ? 0 : (int64_t)ranges * ((s.K + kGwBlk - 1) / kGwBlk) * ((s.N + kGwBlk - 1) / kGwBlk);
}

// floats of one range's partial: dW [K][N], then db [N]
__host__ __device__ inline int64_t wgrad_partial(int K, int N) { return (int64_t)K * N + N; }

__device__ __forceinline__ f32x4 relu_masked(f32x4 v, f32x4 y)
{
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!(y[e] > 0.f)) v[e] = 0.f;
  return v;
}

template <int NT>
__global__ void __launch_bounds__(kThreads) grouped_linear_kernel(gl_args a)
{
  constexpr int NB = 16 * NT;                                // columns of the block
  constexpr int XV = kGlRows * kGlKV / kThreads;             // float4 of X per thread and panel: 2
  constexpr int WV = NB * kGlKV / kThreads;                  // float4 of W per thread and panel: NT / 2
  __shared__ __attribute__((aligned(16))) float xs[kGlRows * kGlS];
  __shared__ __attribute__((aligned(16))) float ws[NB * kGlS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, g = lane >> 4;

  // (segment, row tile): the grid has exactly the segments' tiles; a workgroup past them all leaves
  int k = 0;
  int64_t t = blockIdx.x;
  for (; k < a.n_segs; ++k) {
    const int64_t tiles = (a.s[k].n_rows + kGlRows - 1) / kGlRows;
    if (t < tiles) break;
    t -= tiles;
  }
  if (k == a.n_segs) return;
  const gl_seg& s = a.s[k];
  const int K = s.K, N = s.N, n0 = blockIdx.y * NB;
  if (n0 >= N) return;
  const int64_t row0 = t * kGlRows;
  const int rows_here = (int)std::min<int64_t>(kGlRows, s.n_rows - row0);
  const int nct = std::min(NT, (N - n0 + 15) / 16);
  const bool w_by_k = s.ld_k == 1;                           // the weight's unit stride runs along k

  // the thread's rows of the X panel: float4 c4 of rows tid / 8 and tid / 8 + 32
  const int c4 = tid % kGlKV;
  const float* xrow[XV];
  const float* arow[XV];
#pragma unroll
  for (int v = 0; v < XV; ++v) {
    const int r = tid / kGlKV + v * (kThreads / kGlKV);
    xrow[v] = arow[v] = nullptr;
    if (r < rows_here) {
      const int64_t i = s.ids ? s.ids[row0 + r] : row0 + r;
      xrow[v] = s.x + i * s.ldx;
      if (s.act) arow[v] = s.act + i * s.ld_act;
    }
  }
  // ... and its float4s of the W panel.  Along k: float4 c4 of rows n = tid / 8 + 32 v.  Along n: k row (tid / 4) % 32, float4
  // tid % 4 + 4 (tid / 128) + 8 v of the block's n — 16 k rows x 4 float4 per wave, whose transposing LDS writes hit 64
  // different banks.
  const int wk = (tid / 4) % kGlKP, wn4 = tid % 4 + 4 * (tid / 128);

  f32x4 xr[XV], wr[WV];
  const auto load_panel = [&](int k0) {
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int kk = k0 + 4 * c4;
      xr[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (xrow[v] && kk < K) {
        xr[v] = *reinterpret_cast<const f32x4*>(xrow[v] + kk);
        if (arow[v]) xr[v] = relu_masked(xr[v], *reinterpret_cast<const f32x4*>(arow[v] + kk));
      }
    }
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      // Piece v holds the block's n 32 v .. 32 v + 31 either way: skipped (uniformly) past the last column tile in use.  Inside
      // that tile an n past N reads row N - 1 (or float4 N - 4) again: column n of the weight reaches column n of the product
      // only, and the epilogue stores no column past N — so the one predicate a lane keeps across the K loop is its kk < K.
      wr[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (32 * v >= 16 * nct) continue;
      if (w_by_k) {
        const int n = std::min(n0 + tid / kGlKV + v * (kThreads / kGlKV), N - 1), kk = k0 + 4 * c4;
        if (kk < K) wr[v] = *reinterpret_cast<const f32x4*>(s.w + (int64_t)n * s.ld_n + kk);
      } else {
        const int n = std::min(n0 + 4 * (wn4 + 8 * v), N - 4), kk = k0 + wk;
        if (kk < K) wr[v] = *reinterpret_cast<const f32x4*>(s.w + (int64_t)kk * s.ld_k + n);
      }
    }
  };
  const auto store_panel = [&]() {
#pragma unroll
    for (int v = 0; v < XV; ++v)
      *reinterpret_cast<f32x4*>(xs + (tid / kGlKV + v * (kThreads / kGlKV)) * kGlS + 4 * c4) = xr[v];
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      if (w_by_k) {
        *reinterpret_cast<f32x4*>(ws + (tid / kGlKV + v * (kThreads / kGlKV)) * kGlS + 4 * c4) = wr[v];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) ws[(4 * (wn4 + 8 * v) + e) * kGlS + wk] = wr[v][e];
      }
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool active = wave * 16 < rows_here;                 // the wave's 16 rows begin inside the segment
  load_panel(0);
  for (int k0 = 0; k0 < K; k0 += kGlKP) {
    store_panel();
    __syncthreads();
    if (k0 + kGlKP < K) load_panel(k0 + kGlKP);              // the next panel: in flight under the multiply
    if (active) {
#pragma unroll
      for (int kb = 0; kb < kGlKP; kb += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(xs + (wave * 16 + m) * kGlS + kb + 4 * g);
#pragma unroll
        for (int q = 0; q < NT; ++q) {
          if (q < nct) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(ws + (q * 16 + m) * kGlS + kb + 4 * g);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], bv[kk], acc[q], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;

  // C/D map of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg
  int64_t orow[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int r = wave * 16 + 4 * g + reg;
    orow[reg] = r < rows_here ? (s.out_rows ? s.out_rows[row0 + r] : row0 + r) : -1;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int n = n0 + q * 16 + m;
    if (q >= nct || n >= N) continue;
    const float b = s.bias ? s.bias[n] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      if (orow[reg] < 0) continue;
      float y = acc[q][reg] + b;
      if (s.add) y += s.add[(row0 + wave * 16 + 4 * g + reg) * s.ld_add + n];
      if (a.relu) y = fmaxf(y, 0.f);
      s.out[orow[reg] * s.ldo + n] = y;
    }
  }
}

__global__ void __launch_bounds__(kThreads) grouped_linear_wgrad_kernel(gw_args a)
{
  __shared__ __attribute__((aligned(16))) float xs[kGwRows * kGwS];
  __shared__ __attribute__((aligned(16))) float gs[kGwRows * kGwS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, g = lane >> 4;

  // (segment, item) and the segment's partials: the grid has exactly the segments' items; a workgroup past them all leaves
  int k = 0, ranges = 0;
  int64_t t = blockIdx.x, len = 0;
  float* part = a.ws;
  for (; k < a.n_segs; ++k) {
    wgrad_split(a.s[k].n_rows, a.s[k].K, a.s[k].N, ranges, len);
    const int64_t items = wgrad_items(a.s[k], ranges);
    if (t < items) break;
    t -= items;
    if (a.s[k].dw) part += ranges * wgrad_partial(a.s[k].K, a.s[k].N);
  }
  if (k == a.n_segs) return;
  const gw_seg& s = a.s[k];
  const int K = s.K, N = s.N;
  const int nb = (N + kGwBlk - 1) / kGwBlk, kbs = (K + kGwBlk - 1) / kGwBlk;
  const int n0 = (int)(t % nb) * kGwBlk, k0 = (int)(t / nb % kbs) * kGwBlk;
  const int64_t range = t / nb / kbs;
  const int64_t r0 = range * len, r1 = std::min(r0 + len, s.n_rows);
  part += range * wgrad_partial(K, N);

  // a thread stages float4 c4 of panel rows tid / 16 + 16 v of both operands
  const int c4 = tid % 16, pr = tid / 16;
  const bool x_in = k0 + 4 * c4 < K, g_in = n0 + 4 * c4 < N;
  f32x4 xr[kGwV], gr[kGwV], bsum = {0.f, 0.f, 0.f, 0.f};
  const auto load_panel = [&](int64_t rp) {
#pragma unroll
    for (int v = 0; v < kGwV; ++v) {
      const int64_t i = rp + pr + 16 * v;
      xr[v] = gr[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i >= r1) continue;
      if (x_in) xr[v] = *reinterpret_cast<const f32x4*>(s.x + (s.ids ? s.ids[i] : i) * s.ldx + k0 + 4 * c4);
      if (g_in) {
        const int64_t j = s.g_rows ? s.g_rows[i] : i;
        gr[v] = *reinterpret_cast<const f32x4*>(s.g + j * s.ldg + n0 + 4 * c4);
        if (s.act) gr[v] = relu_masked(gr[v], *reinterpret_cast<const f32x4*>(s.act + j * s.ld_act + n0 + 4 * c4));
      }
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool active = k0 + wave * 16 < K;                    // the wave's 16 k rows lie inside the weight
  const int nct = std::min(4, (N - n0 + 15) / 16);
  load_panel(r0);
  for (int64_t rp = r0; rp < r1; rp += kGwRows) {
#pragma unroll
    for (int v = 0; v < kGwV; ++v) {
      *reinterpret_cast<f32x4*>(xs + (pr + 16 * v) * kGwS + 4 * c4) = xr[v];
      *reinterpret_cast<f32x4*>(gs + (pr + 16 * v) * kGwS + 4 * c4) = gr[v];
      bsum += gr[v];
    }
    __syncthreads();
    if (rp + kGwRows < r1) load_panel(rp + kGwRows);
    if (active) {
      // an MFMA step contracts the four panel rows rb + 4 g + kk (g = 0 .. 3): lane (m, g) gives A[m][g] = X[row, k m] and
      // B[g][m] = dY[row, n m] — both read down a column of the panel, the transposed fragment
#pragma unroll 2
      for (int rb = 0; rb < kGwRows; rb += 16) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int row = rb + 4 * g + kk;
          const float av = xs[row * kGwS + wave * 16 + m];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < nct) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, gs[row * kGwS + q * 16 + m], acc[q], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + q * 16 + m;
      if (q >= nct || n >= N) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int kk = k0 + wave * 16 + 4 * g + reg;
        if (kk < K) part[(int64_t)kk * N + n] = acc[q][reg];
      }
    }
  }
  if (k0 != 0) return;                                       // (uniform in the workgroup)
  // the column sums of the masked dY: the 16 row groups' sums through LDS, added in group order
  *reinterpret_cast<f32x4*>(xs + pr * kGwS + 4 * c4) = bsum;
  __syncthreads();
  if (tid < kGwBlk && n0 + tid < N) {
    float sum = 0.f;
    for (int q = 0; q < 16; ++q) sum += xs[q * kGwS + tid];
    part[(int64_t)K * N + n0 + tid] = sum;
  }
}

struct gr_seg {
  const float* part;
  float* dw;
  float* db;
  int64_t ld_n, ld_k;
  int K, N, ranges;
};

struct gr_args {
  gr_seg s[kGlSegs];
};

// element e of the segment's partial (dW [K][N], then db [N]) summed over the ranges in order; grid (ceil(max elements / 256), n_segs)
__global__ void __launch_bounds__(kThreads) grouped_linear_reduce_kernel(gr_args a)
{
  const gr_seg& s = a.s[blockIdx.y];
  const int64_t kn = (int64_t)s.K * s.N, stride = wgrad_partial(s.K, s.N);
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s.dw == nullptr || e >= stride) return;
  float sum = 0.f;
  for (int r = 0; r < s.ranges; ++r) sum += s.part[r * stride + e];
  if (e < kn) s.dw[(e % s.N) * s.ld_n + (e / s.N) * s.ld_k] = sum;
  else if (s.db) s.db[e - kn] = sum;
}

inline bool vec_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void check_count(const wgamd_grouped_linear_segment* segs, int n_segs)
{
  WG_REQUIRE_INPUT(segs != nullptr && n_segs >= 1 && n_segs <= kGlSegs, "n_segs = %d: 1 .. %d segments per launch", n_segs, kGlSegs);
}

// the shape and the weight's strides of a segment, for a weight or a weight gradient at `w`
void check_weight(const wgamd_grouped_linear_segment& d, const float* w)
{
  WG_REQUIRE_INPUT(d.n_rows >= 0, "bad sizes");
  if (!wgamd_grouped_linear_supported(d.K, d.N))
    throw logic_error(fmt("unsupported shape: K=%d, N=%d (multiples of 4, 4 .. 1024)", d.K, d.N));
  const bool by_k = d.ld_k == 1 && d.ld_n >= d.K, by_n = d.ld_n == 1 && d.ld_k >= d.N;
  WG_REQUIRE_INPUT(by_k || by_n, "weight strides (ld_n=%lld, ld_k=%lld): one must be 1, the other at least the row's width",
                   (long long)d.ld_n, (long long)d.ld_k);
  if (!vec_ok(w) || (by_k ? d.ld_n : d.ld_k) % 4 != 0) throw logic_error("weight rows must be 16-B aligned");
}

// the weight-gradient launches' view of the segments; false = nothing to launch
bool make_wgrad_args(gw_args& a, const wgamd_grouped_linear_segment* segs, int n_segs, int64_t& items, int64_t& floats)
{
  check_count(segs, n_segs);
  a = gw_args{};
  a.n_segs = n_segs;
  items = floats = 0;
  for (int k = 0; k < n_segs; ++k) {
    const auto& d = segs[k];
    check_weight(d, d.dw);
    gw_seg& s = a.s[k];
    s.x = d.x, s.ids = d.ids, s.g = d.grad_out, s.g_rows = d.out_rows, s.act = d.act_out, s.dw = d.dw, s.db = d.db;
    s.ldx = d.ldx, s.ldg = d.ldg, s.ld_act = d.ld_act, s.ld_n = d.ld_n, s.ld_k = d.ld_k, s.n_rows = d.n_rows, s.K = d.K, s.N = d.N;
    if (d.dw == nullptr) {
      WG_REQUIRE_INPUT(d.db == nullptr, "db without dw");
      continue;
    }
    if (d.n_rows > 0) {
      WG_REQUIRE_INPUT(d.x && d.grad_out, "null pointer");
      WG_REQUIRE_INPUT(d.ldx >= d.K && d.ldg >= d.N && (d.act_out == nullptr || d.ld_act >= d.N), "leading dimension too small");
      if (!aligned_rows(d.x, d.ldx) || !aligned_rows(d.grad_out, d.ldg) || (d.act_out && !aligned_rows(d.act_out, d.ld_act)))
        throw logic_error("x / grad_out / act_out rows must be 16-B aligned (leading dimensions multiples of 4)");
    }
    int ranges;
    int64_t len;
    wgrad_split(d.n_rows, d.K, d.N, ranges, len);
    items += wgrad_items(s, ranges);
    floats += ranges * wgrad_partial(d.K, d.N);
  }
  return true;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_grouped_linear_supported(int K, int N)
{
  return K % 4 == 0 && K >= 4 && K <= 1024 && N % 4 == 0 && N >= 4 && N <= 1024;
}

extern "C" size_t wgamd_grouped_linear_wgrad_workspace_bytes(const wgamd_grouped_linear_segment* segs, int n_segs)
{
  using namespace wgamd;
  int64_t floats = 0;
  for (int k = 0; segs != nullptr && k < n_segs && k < kGlSegs; ++k) {
    if (segs[k].dw == nullptr || !wgamd_grouped_linear_supported(segs[k].K, segs[k].N)) continue;
    int ranges;
    int64_t len;
    wgrad_split(segs[k].n_rows, segs[k].K, segs[k].N, ranges, len);
    floats += ranges * wgrad_partial(segs[k].K, segs[k].N);
  }
  return (size_t)floats * sizeof(float);
}

extern "C" wholememory_error_code_t wgamd_grouped_linear_f32(const wgamd_grouped_linear_segment* segs, int n_segs, int relu,
                                                             void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_grouped_linear_f32", [&] {
    check_count(segs, n_segs);
    gl_args a{};
    a.n_segs = n_segs, a.relu = relu ? 1 : 0;
    int64_t tiles = 0;
    int max_n = 0;
    for (int k = 0; k < n_segs; ++k) {
      const auto& d = segs[k];
      check_weight(d, d.w);
      gl_seg& s = a.s[k];
      s.x = d.x, s.ids = d.ids, s.w = d.w, s.bias = d.bias, s.add = d.add, s.out = d.out, s.out_rows = d.out_rows, s.act = d.act_out;
      s.ldx = d.ldx, s.ld_n = d.ld_n, s.ld_k = d.ld_k, s.ld_add = d.ld_add, s.ldo = d.ldo, s.ld_act = d.ld_act;
      s.n_rows = d.n_rows, s.K = d.K, s.N = d.N;
      if (d.n_rows == 0) continue;
      WG_REQUIRE_INPUT(d.x && d.w && d.out, "null pointer");
      WG_REQUIRE_INPUT(d.ldx >= d.K && d.ldo >= d.N && (d.add == nullptr || d.ld_add >= d.N) && (d.act_out == nullptr || d.ld_act >= d.K),
                       "leading dimension too small");
      if (!aligned_rows(d.x, d.ldx) || !aligned_rows(d.out, d.ldo) || (d.add && !aligned_rows(d.add, d.ld_add)) ||
          (d.act_out && !aligned_rows(d.act_out, d.ld_act)))
        throw logic_error("x / out / add / act_out rows must be 16-B aligned (leading dimensions multiples of 4)");
      tiles += (d.n_rows + kGlRows - 1) / kGlRows;
      max_n = std::max(max_n, d.N);
    }
    if (tiles == 0) return;
    WG_REQUIRE_INPUT(tiles <= 0x7fffffff, "too many rows for one launch");
    auto st = static_cast<hipStream_t>(stream);
    if (max_n <= 64) grouped_linear_kernel<4><<<dim3((unsigned)tiles, 1), kThreads, 0, st>>>(a);
    else if (max_n <= 128) grouped_linear_kernel<8><<<dim3((unsigned)tiles, 1), kThreads, 0, st>>>(a);
    else grouped_linear_kernel<16><<<dim3((unsigned)tiles, (unsigned)((max_n + 255) / 256)), kThreads, 0, st>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_grouped_linear_wgrad_f32(const wgamd_grouped_linear_segment* segs, int n_segs,
                                                                   float* workspace, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_grouped_linear_wgrad_f32", [&] {
    gw_args a;
    int64_t items, floats;
    make_wgrad_args(a, segs, n_segs, items, floats);
    if (items == 0) return;
    WG_REQUIRE_INPUT(workspace != nullptr && items <= 0x7fffffff, "null workspace");
    if (!vec_ok(workspace)) throw logic_error("workspace must be 16-B aligned");
    a.ws = workspace;
    grouped_linear_wgrad_kernel<<<(unsigned)items, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_grouped_linear_wgrad_reduce_f32(const wgamd_grouped_linear_segment* segs, int n_segs,
                                                                          const float* workspace, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_grouped_linear_wgrad_reduce_f32", [&] {
    gw_args w;
    int64_t items, floats;
    make_wgrad_args(w, segs, n_segs, items, floats);
    WG_REQUIRE_INPUT(floats == 0 || workspace != nullptr, "null workspace");
    gr_args a{};
    int64_t at = 0, most = 0;
    for (int k = 0; k < n_segs; ++k) {
      const gw_seg& s = w.s[k];
      if (s.dw == nullptr) continue;      // (a.s[k].dw stays null: the workgroups of that segment leave)
      int64_t len;
      gr_seg& r = a.s[k];
      wgrad_split(s.n_rows, s.K, s.N, r.ranges, len);
      r.part = workspace + at, r.dw = s.dw, r.db = s.db, r.ld_n = s.ld_n, r.ld_k = s.ld_k, r.K = s.K, r.N = s.N;
      at += r.ranges * wgrad_partial(s.K, s.N);
      most = std::max(most, wgrad_partial(s.K, s.N));
    }
    if (most == 0) return;
    const dim3 grid((unsigned)((most + kThreads - 1) / kThreads), (unsigned)n_segs);
    grouped_linear_reduce_kernel<<<grid, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
