// PNA layer (torch_geometric.nn.PNAConv, flow source_to_target, towers = 1, pre_layers = post_layers = 1) over a sampled hop.  The
// message of edge j -> i is linear, m_ji = a_i + y_j with y = X W_j^T over the input rows and a = X_dst W_i^T + b over the
// destinations (both made before the launch), so the kernel reduces y alone:
//     stat[i]  = the A chosen of  sum, mean, min, max, var, std  of {a_i + y_j : j -> i}, per channel            (0 without edges)
//     Z[i, :]  = [x_i | s_1(deg_i) stat[i] | ... | s_S(deg_i) stat[i]] @ Wp^T + bp          (scaler-major, Wp = post_nns.0.0.weight)
//     out[i,:] = act(Z[i] @ Wl^T + bl)                                                       (Wl = lin.weight)
// Four scatter passes over an [E, F] message array and a [n, (1 + S A) F] concatenation in the torch-ops formulation; here
// neither exists.
//
//   * pna_layer_kernel — one launch per hop, a workgroup owns R = 16 M destination rows (M = 4, 2 or 1: the largest whose tile fits
//     the CU's 160 KB of LDS, pna_row_tiles).  Phase 1: a lane group of LG >= F / 4 lanes per destination row, a lane = one float4
//     of the row, eight edges in flight in CSR order.  Per channel in registers: the sum, the sum and the sum of squares of the
//     DEVIATIONS from the row's first message (var = d2 / deg - (d1 / deg)^2: mean(y^2) - mean(y)^2 cancels in float32 and the
//     sqrt(. + 1e-5) of std amplifies that 158-fold near zero; a row of degree 1 or of one repeated source gives d1 = d2 = 0 and
//     std = sqrt(1e-5) exactly), the minimum and the maximum with their CSR edge slots (strict compares: the lowest slot wins a
//     tie, as in wg_sage_max.hip).  a_i joins sum (x deg), mean, min and max; var and std do not see it.  The row's
//     [x_i | stat_1 .. stat_A] goes to LDS UNSCALED, (1 + A) F floats, and the row's S scaler values beside it.
//     Phase 2: the tile times Wp^T on v_mfma_f32_16x16x4_f32, Wp read in its own [N, (1 + S A) F] layout.  The A operand of
//     block (scaler s, aggregator a) is the LDS value of aggregator a times s(deg_row), formed in registers as the fragment is
//     loaded; every weight fragment a wave loads meets all M row tiles before the next is fetched (M x fewer weight bytes per
//     destination row than a 16-row workgroup reads).  Phase 3: Z (+ bp) is staged in LDS over the finished tile and each 16-row
//     sub-tile goes through tile_times_wt with Wl, bl and the ReLU.  With a null Wp the kernel ends after phase 1 and the
//     statistics are the output (towers, deeper post_nns: the rest runs outside).
//   * pna_bwd_src_kernel — over the hop's transpose, a lane group per SOURCE row holding y_j; entry (j -> i, CSR slot e) adds
//         c0_i + (y_j - meany_i) c1_i + [argmax_i = e] dmax_i + [argmin_i = e] dmin_i
//     with c0 = dsum + dmean / deg and c1 = (2 dvar + dstd / std) / deg made per destination by the host.  gen_bwd_src_kernel's
//     frame: a bounded grid over 16-row tiles at a fixed stride, rows of more than 64 entries cut into 64-entry pieces that the
//     lane groups take round-robin and that are added in group order from LDS.  No atomics: the same bits from run to run.
#include <cfloat>
#include <cmath>

#include "wg_gin_parts.hpp"

namespace wgamd {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int kPnaMaxAggr    = 6;
constexpr int kPnaMaxScalers = 5;
constexpr int kPnaLdsBytes   = 160 * 1024;   // the LDS of one gfx950 CU, all of it one workgroup's at most
constexpr int kPnaWgCu       = 4;            // workgroups per CU of the backward
constexpr int kPnaPiece      = 64;           // entries per piece of a long transposed row
constexpr int kPnaBwdUnroll  = 2;            // entries of a source row in flight (up to seven destination rows each)
constexpr float kPnaStdEps   = 1e-5f;

struct pna_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* y;             // [n_src, ldy], read by row or through src_ids
  int64_t ldy;
  int F;
  const void* src_ids;
  const float* a;             // nullable (0): [n_rows, lda]
  int64_t lda;
  const float* xd;            // [n_rows, ldxd]: the destinations' own rows (not read without wp)
  int64_t ldxd;
  int A;
  int aggr[kPnaMaxAggr];      // WGAMD_PNA_SUM ..
  int S;
  int scaler[kPnaMaxScalers]; // WGAMD_PNA_IDENTITY ..
  float avg_lin, avg_log;
  const float* wp;            // nullable: [N, ldwp], (1 + S A) F columns
  int64_t ldwp;
  int N;
  const float* bp;
  const float* wl;            // [NO, ldwl]
  int64_t ldwl;
  int NO;
  const float* bl;
  int relu;
  float* out;                 // [n_rows, NO]; without wp: the statistics [n_rows, A F]
  int64_t ldo;
  float* stats_out;           // nullable: [n_rows, A F]
  int64_t ld_stats;
  float* mean_out;            // nullable: the mean of y [n_rows, F]
  int64_t ld_mean;
  int* argmin_out;            // nullable: CSR edge slots [n_rows, ld_arg], -1 without edges
  int* argmax_out;
  int64_t ld_arg;
  float* z_out;               // nullable: [n_rows, N]
  int64_t ld_z;
  int M, SD, N16, SN;         // row tiles per workgroup; floats per LDS row of the statistics tile; N up to 16; of the Z tile
};

__device__ __forceinline__ float pna_scale(int code, int deg, float avg_lin, float avg_log)
{
  const float d = (float)(deg > 1 ? deg : 1);
  const float lg = logf(d + 1.f);
  switch (code) {
    case WGAMD_PNA_AMPLIFICATION: return lg / avg_log;
    case WGAMD_PNA_ATTENUATION: return avg_log / lg;
    case WGAMD_PNA_LINEAR: return d / avg_lin;
    case WGAMD_PNA_INVERSE_LINEAR: return avg_lin / d;
    default: return 1.f;
  }
}

// what a lane keeps of one destination row, channels [4 c, 4 c + 4)
struct pna_row {
  f32x4 sum, d1, d2, mn, mx;
  i32x4 amn, amx;
};

template <int KIND>
__device__ __forceinline__ void pna_walk(const pna_args& p, int s, int t, int c, bool active, pna_row& r)
{
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  r.sum = r.d1 = r.d2 = zero;
  r.mn = f32x4{INFINITY, INFINITY, INFINITY, INFINITY};
  r.mx = -r.mn;
  r.amn = r.amx = i32x4{-1, -1, -1, -1};
  f32x4 first = zero;
  if (t > s && active) first = reinterpret_cast<const f32x4*>(x_row<KIND>(p.y, p.ldy, p.src_ids, p.col[s]))[c];
  for (int e = s; e < t; e += kGinUnroll) {
    int j[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) j[u] = e + u < t ? p.col[e + u] : -1;
    f32x4 v[kGinUnroll];
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      v[u] = zero;
      if (j[u] >= 0 && active) v[u] = reinterpret_cast<const f32x4*>(x_row<KIND>(p.y, p.ldy, p.src_ids, j[u]))[c];
    }
#pragma unroll
    for (int u = 0; u < kGinUnroll; ++u) {
      if (j[u] >= 0) {                                     // (the same for a whole lane group)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float val = v[u][k], d = val - first[k];
          r.sum[k] += val;
          r.d1[k] += d;
          r.d2[k] = __builtin_fmaf(d, d, r.d2[k]);
          const bool lo = val < r.mn[k], hi = val > r.mx[k];
          r.mn[k] = lo ? val : r.mn[k];
          r.amn[k] = lo ? e + u : r.amn[k];
          r.mx[k] = hi ? val : r.mx[k];
          r.amx[k] = hi ? e + u : r.amx[k];
        }
      }
    }
  }
}

// the statistic `code` of a row of deg > 0 edges from what the walk kept; av = a_i
__device__ __forceinline__ f32x4 pna_stat(int code, const pna_row& r, f32x4 meany, f32x4 var, f32x4 av, float deg)
{
  f32x4 st;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    switch (code) {
      case WGAMD_PNA_SUM: st[k] = __builtin_fmaf(deg, av[k], r.sum[k]); break;
      case WGAMD_PNA_MEAN: st[k] = meany[k] + av[k]; break;
      case WGAMD_PNA_MIN: st[k] = r.mn[k] + av[k]; break;
      case WGAMD_PNA_MAX: st[k] = r.mx[k] + av[k]; break;
      case WGAMD_PNA_VAR: st[k] = var[k]; break;
      default: st[k] = sqrtf(fmaxf(var[k], 0.f) + kPnaStdEps); break;
    }
  }
  return st;
}

// phases 2 and 3 over the finished statistics tile (behind the barrier that ends phase 1)
template <int M>
__device__ __forceinline__ void pna_products(const pna_args& p, float* tile, const float* scal, int64_t row0)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, g = lane >> 4;
  const int n_ct = (p.N + 15) / 16, F = p.F;
  f32x4 acc[4][M];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int mt = 0; mt < M; ++mt) acc[q][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- phase 2: [16 M x (1 + S A) F] (never stored: block b of it is LDS block 0, or 1 + (b - 1) % A times a scaler) @ Wp^T ----
  if (wave < n_ct) {
    const int n_blk = 1 + p.S * p.A;
    for (int b = 0; b < n_blk; ++b) {
      const int lb = b == 0 ? 0 : 1 + (b - 1) % p.A;
      float sc[M];
#pragma unroll
      for (int mt = 0; mt < M; ++mt) sc[mt] = b == 0 ? 1.f : scal[(mt * 16 + m) * kPnaMaxScalers + (b - 1) / p.A];
      const float* wb = p.wp + (int64_t)b * F;
      const float* tb = tile + m * p.SD + lb * F;
      for (int kb = 0; kb < F; kb += 16) {
        const int k = kb + 4 * g;
        const bool kin = k < F;                           // (F % 16 != 0: the last k-step's upper lanes carry zeros)
        f32x4 av[M];
#pragma unroll
        for (int mt = 0; mt < M; ++mt) {
          av[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (kin) av[mt] = *reinterpret_cast<const f32x4*>(tb + mt * 16 * p.SD + k) * sc[mt];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ct = wave + 4 * q;
          if (ct < n_ct) {
            const int n = ct * 16 + m;
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (n < p.N && kin) bv = *reinterpret_cast<const f32x4*>(wb + (int64_t)n * p.ldwp + k);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
              for (int mt = 0; mt < M; ++mt)              // one weight fragment, all M row tiles
                acc[q][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][kk], bv[kk], acc[q][mt], 0, 0, 0);
          }
        }
      }
    }
  }
  __syncthreads();                                        // the statistics tile has been read: Z goes over it

  // C/D map of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg; columns [N, N16) of the Z tile are zero
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = (wave + 4 * q) * 16 + m;
    if (wave + 4 * q >= n_ct) continue;
    const float b = n < p.N && p.bp ? p.bp[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < M; ++mt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) tile[(mt * 16 + 4 * g + reg) * p.SN + n] = n < p.N ? acc[q][mt][reg] + b : 0.f;
  }
  __syncthreads();
  if (p.z_out) {
    const int N4 = p.N / 4;                               // (N % 4 == 0 with kept rows: checked by the host)
    for (int idx = threadIdx.x; idx < 16 * M * N4; idx += kThreads) {
      const int r = idx / N4, q = idx % N4;
      if (row0 + r < p.n_rows)
        reinterpret_cast<f32x4*>(p.z_out + (row0 + r) * p.ld_z)[q] = reinterpret_cast<const f32x4*>(tile + r * p.SN)[q];
    }
  }

  // ---- phase 3: every 16-row sub-tile of Z @ Wl^T ----
#pragma unroll
  for (int mt = 0; mt < M; ++mt)
    if (row0 + 16 * mt < p.n_rows)
      tile_times_wt(tile + mt * 16 * p.SN, p.SN, p.N, p.N16, p.wl, p.ldwl, p.NO, p.bl, p.relu, p.out, p.ldo, row0 + 16 * mt, p.n_rows);
}

template <int KIND, int LG>
__global__ void __launch_bounds__(kThreads) pna_layer_kernel(pna_args p)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int kGroups = kThreads / LG;
  const int tid = threadIdx.x;
  const int R = kTileRows * p.M;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int grp = tid / LG, c = tid % LG;
  const int F = p.F, C4 = F / 4;
  const bool active = c < C4;
  float* scal = tile + R * (p.SD > p.SN ? p.SD : p.SN);   // [R][kPnaMaxScalers]
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // ---- phase 1: [x_i | stat_1 .. stat_A] of the workgroup's rows -> LDS (and the kept rows) ----
  for (int r = grp; r < R; r += kGroups) {
    const int64_t i = row0 + r;
    const bool row = i < p.n_rows;
    int s = 0, t = 0;
    if (row) s = p.row_ptr[i], t = p.row_ptr[i + 1];
    pna_row w;
    pna_walk<KIND>(p, s, t, c, active, w);
    const int deg = t - s;
    const float fdeg = (float)deg;
    f32x4 av = zero, meany = zero, var = zero;
    if (deg > 0) {
      if (p.a && active) av = reinterpret_cast<const f32x4*>(p.a + i * p.lda)[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        meany[k] = w.sum[k] / fdeg;
        const float dev = w.d1[k] / fdeg;
        var[k] = w.d2[k] / fdeg - dev * dev;
      }
    }
    if (p.wp) {
      if (active) {
        reinterpret_cast<f32x4*>(tile + r * p.SD)[c] = row ? reinterpret_cast<const f32x4*>(p.xd + i * p.ldxd)[c] : zero;
      }
      for (int k = c; k < p.S; k += LG) scal[r * kPnaMaxScalers + k] = pna_scale(p.scaler[k], deg, p.avg_lin, p.avg_log);
    }
    for (int ai = 0; ai < p.A; ++ai) {
      const f32x4 st = deg > 0 ? pna_stat(p.aggr[ai], w, meany, var, av, fdeg) : zero;
      if (!active) continue;
      if (p.wp) reinterpret_cast<f32x4*>(tile + r * p.SD + (1 + ai) * F)[c] = st;
      if (row && p.stats_out) reinterpret_cast<f32x4*>(p.stats_out + i * p.ld_stats + ai * F)[c] = st;
    }
    if (row && active) {
      if (p.mean_out) reinterpret_cast<f32x4*>(p.mean_out + i * p.ld_mean)[c] = meany;
      if (p.argmin_out) reinterpret_cast<i32x4*>(p.argmin_out + i * p.ld_arg)[c] = w.amn;
      if (p.argmax_out) reinterpret_cast<i32x4*>(p.argmax_out + i * p.ld_arg)[c] = w.amx;
    }
  }
  if (p.wp == nullptr) return;                            // (uniform) the statistics alone
  __syncthreads();
  if (p.M == 4) pna_products<4>(p, tile, scal, row0);
  else if (p.M == 2) pna_products<2>(p, tile, scal, row0);
  else pna_products<1>(p, tile, scal, row0);
}

// bytes of LDS of a workgroup of M row tiles: the statistics tile and the Z tile share the space, the scaler values follow
size_t pna_lds_bytes(int M, int SD, int SN) { return (size_t)kTileRows * M * (std::max(SD, SN) + kPnaMaxScalers) * 4; }

// M = 4, 2 or 1: the most row tiles whose workgroup fits the CU's LDS (F <= 64 with six aggregators: 4; F = 256: 1)
int pna_row_tiles(int SD, int SN)
{
  for (int M = 4; M > 1; M /= 2)
    if (pna_lds_bytes(M, SD, SN) <= (size_t)kPnaLdsBytes) return M;
  return 1;
}

template <int KIND, int LG>
void launch_one(const pna_args& p, hipStream_t st)
{
  auto kern = pna_layer_kernel<KIND, LG>;
  const int R = kTileRows * p.M;
  const dim3 grid((unsigned)((p.n_rows + R - 1) / R));
  const size_t lds = p.wp ? pna_lds_bytes(p.M, p.SD, p.SN) : 0;
  if (lds > 48 * 1024)
    WG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, kThreads, lds, st>>>(p);
}

// ---- source-major backward: the gradient of y ---------------------------------------------------------------------------------
struct pna_src_args {
  const int* row_ptr_t;       // the hop's transpose: rows = input rows
  const int* col_t;           // destination row of every entry
  const int* perm;            // the hop's CSR edge slot of every entry (read with dmax / dmin)
  int64_t n_src;
  int n_tiles;
  const float* y;
  int64_t ldy;
  const void* src_ids;
  int F;
  const float* c0;            // nullable: [n_dst, ld_c]
  const float* c1;            // nullable, with meany
  int64_t ld_c;
  const float* meany;
  int64_t ld_mean;
  const float* dmax;          // nullable, with amax
  const float* dmin;          // nullable, with amin
  int64_t ld_d;
  const int* amax;
  const int* amin;
  int64_t ld_arg;
  float* gy;                  // [n_src, ldgy], every row written
  int64_t ldgy;
  int lg_shift;
};

// the sum over the entries [s, t) of source row j, channels [4 c, 4 c + 4), in entry order
__device__ __forceinline__ f32x4 pna_entries(const pna_src_args& a, int s, int t, int c, f32x4 yv)
{
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int e = s; e < t; e += kPnaBwdUnroll) {
    int d[kPnaBwdUnroll], slot[kPnaBwdUnroll];
#pragma unroll
    for (int u = 0; u < kPnaBwdUnroll; ++u) {
      d[u] = e + u < t ? a.col_t[e + u] : -1;
      slot[u] = e + u < t && a.perm ? a.perm[e + u] : -2;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 g0[kPnaBwdUnroll], g1[kPnaBwdUnroll], mu[kPnaBwdUnroll], gx[kPnaBwdUnroll], gn[kPnaBwdUnroll];
    i32x4 ax[kPnaBwdUnroll], an[kPnaBwdUnroll];
#pragma unroll
    for (int u = 0; u < kPnaBwdUnroll; ++u) {
      g0[u] = g1[u] = mu[u] = gx[u] = gn[u] = zero;
      ax[u] = an[u] = i32x4{-1, -1, -1, -1};
      if (d[u] < 0) continue;
      const int64_t i = d[u];
      if (a.c0) g0[u] = reinterpret_cast<const f32x4*>(a.c0 + i * a.ld_c)[c];
      if (a.c1) {
        g1[u] = reinterpret_cast<const f32x4*>(a.c1 + i * a.ld_c)[c];
        mu[u] = reinterpret_cast<const f32x4*>(a.meany + i * a.ld_mean)[c];
      }
      if (a.dmax) {
        gx[u] = reinterpret_cast<const f32x4*>(a.dmax + i * a.ld_d)[c];
        ax[u] = reinterpret_cast<const i32x4*>(a.amax + i * a.ld_arg)[c];
      }
      if (a.dmin) {
        gn[u] = reinterpret_cast<const f32x4*>(a.dmin + i * a.ld_d)[c];
        an[u] = reinterpret_cast<const i32x4*>(a.amin + i * a.ld_arg)[c];
      }
    }
#pragma unroll
    for (int u = 0; u < kPnaBwdUnroll; ++u) {
      if (d[u] < 0) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v = __builtin_fmaf(yv[k] - mu[u][k], g1[u][k], g0[u][k]);
        v += ax[u][k] == slot[u] ? gx[u][k] : 0.f;
        v += an[u][k] == slot[u] ? gn[u][k] : 0.f;
        acc[k] += v;
      }
    }
  }
  return acc;
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) pna_bwd_src_kernel(pna_src_args a)
{
  __shared__ f32x4 part[kThreads];
  const int tid = threadIdx.x;
  const int LG = 1 << a.lg_shift, groups = kThreads >> a.lg_shift;
  const int grp = tid >> a.lg_shift, c = tid & (LG - 1);
  const bool active = c < a.F / 4;

  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {            // (a fixed stride: the same sums every run)
    const int64_t row0 = (int64_t)tile * kTileRows;
    // rows of at most kPnaPiece entries: one lane group each
    for (int r = grp; r < kTileRows; r += groups) {
      const int64_t j = row0 + r;
      if (j >= a.n_src) break;
      const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
      if (t - s > kPnaPiece || !active) continue;
      f32x4 yv = {0.f, 0.f, 0.f, 0.f};
      if (t > s) yv = reinterpret_cast<const f32x4*>(x_row<KIND>(a.y, a.ldy, a.src_ids, j))[c];
      reinterpret_cast<f32x4*>(a.gy + j * a.ldgy)[c] = pna_entries(a, s, t, c, yv);
    }

    // longer rows: every lane group takes pieces round-robin (r, s, t are the same in every thread: the barriers are uniform)
    for (int r = 0; r < kTileRows; ++r) {
      const int64_t j = row0 + r;
      if (j >= a.n_src) break;
      const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
      if (t - s <= kPnaPiece) continue;
      f32x4 yv = {0.f, 0.f, 0.f, 0.f}, acc = yv;
      if (active) {
        yv = reinterpret_cast<const f32x4*>(x_row<KIND>(a.y, a.ldy, a.src_ids, j))[c];
        for (int p0 = s + grp * kPnaPiece; p0 < t; p0 += groups * kPnaPiece) acc += pna_entries(a, p0, std::min(t, p0 + kPnaPiece), c, yv);
      }
      __syncthreads();      // (the previous long row's sums have been read)
      part[tid] = acc;
      __syncthreads();
      if (grp == 0 && active) {
        f32x4 total = part[c];
        for (int g = 1; g < groups; ++g) total += part[g * LG + c];
        reinterpret_cast<f32x4*>(a.gy + j * a.ldgy)[c] = total;
      }
    }
  }
}

bool pna_shape_ok(int F, int N) { return F >= 4 && F <= 256 && F % 4 == 0 && N >= 0 && N <= 256; }

int64_t pna_tiles(int64_t n_rows) { return n_rows <= 0 ? 0 : (n_rows + kTileRows - 1) / kTileRows; }

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_pna_layer_supported(int F, int N) { return wgamd::pna_shape_ok(F, N); }

extern "C" int wgamd_pna_row_tiles(int F, int n_aggr, int N)
{
  if (!wgamd::pna_shape_ok(F, N) || N == 0 || n_aggr < 1 || n_aggr > wgamd::kPnaMaxAggr) return 0;
  return wgamd::pna_row_tiles((1 + n_aggr) * F + 4, (N + 15) / 16 * 16 + 4);
}

extern "C" int64_t wgamd_pna_bwd_blocks(int64_t n_src, int max_blocks)
{
  const int64_t cap = max_blocks > 0 ? max_blocks : (int64_t)wgamd::kPnaWgCu * wgamd::stream_cu_count(nullptr);
  return std::min<int64_t>(wgamd::pna_tiles(n_src), cap);
}

extern "C" wholememory_error_code_t wgamd_pna_layer_f32_train(
    const int* row_ptr, const int* col, int64_t n_rows, const float* y, int64_t ldy, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const float* a, int64_t lda, const float* x_dst, int64_t ldx_dst, const int* aggregators,
    int n_aggr, const int* scalers, int n_scalers, float avg_lin, float avg_log, const float* w_post, int64_t ldw_post, int N,
    const float* b_post, const float* w_lin, int64_t ldw_lin, int N_out, const float* b_lin, int flags, float* out, int64_t ldo,
    float* stats_out, int64_t ld_stats, float* mean_out, int64_t ld_mean, int* argmin_out, int* argmax_out, int64_t ld_arg,
    float* z_out, int64_t ld_z, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pna_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    WG_REQUIRE_INPUT(aggregators && n_aggr >= 1 && n_aggr <= kPnaMaxAggr, "1 .. 6 aggregators");
    for (int k = 0; k < n_aggr; ++k) WG_REQUIRE_INPUT(aggregators[k] >= WGAMD_PNA_SUM && aggregators[k] <= WGAMD_PNA_STD, "bad aggregator");
    WG_REQUIRE_INPUT((w_post == nullptr) == (N == 0) && (w_post == nullptr) == (w_lin == nullptr) && (w_lin == nullptr) == (N_out == 0),
                     "w_post, w_lin, N and N_out come together, or none (the statistics alone)");
    if (!pna_shape_ok(F, N) || !pna_shape_ok(F, N_out))
      throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, <= 256), N=%d, N_out=%d (<= 256)", F, N, N_out));
    const int width = w_post ? N_out : n_aggr * F;
    if (w_post) {
      WG_REQUIRE_INPUT(scalers && n_scalers >= 1 && n_scalers <= kPnaMaxScalers, "1 .. 5 scalers");
      for (int k = 0; k < n_scalers; ++k)
        WG_REQUIRE_INPUT(scalers[k] >= WGAMD_PNA_IDENTITY && scalers[k] <= WGAMD_PNA_INVERSE_LINEAR, "bad scaler");
      WG_REQUIRE_INPUT(avg_lin > 0.f && avg_log > 0.f, "the degree averages must be positive");
    }
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && y && out && (w_post == nullptr || x_dst), "null pointer");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT((kind == 3 || ldy >= F) && (a == nullptr || lda >= F) && ldo >= width, "leading dimension too small");
    WG_REQUIRE_INPUT(w_post == nullptr || (ldx_dst >= F && ldw_post >= (int64_t)(1 + n_scalers * n_aggr) * F && ldw_lin >= N),
                     "leading dimension too small");
    WG_REQUIRE_INPUT((stats_out == nullptr || ld_stats >= n_aggr * F) && (mean_out == nullptr || ld_mean >= F) &&
                       ((argmin_out == nullptr && argmax_out == nullptr) || ld_arg >= F) && (z_out == nullptr || (ld_z >= N && N % 4 == 0)),
                     "kept rows: leading dimension too small (z_out: N a multiple of 4)");
    if (!aligned_rows(y, kind == 3 ? 0 : ldy) || (a && !aligned_rows(a, lda)) ||
        (w_post && (!aligned_rows(x_dst, ldx_dst) || !aligned_rows(w_post, ldw_post) || !aligned_rows(w_lin, ldw_lin))) ||
        (w_post == nullptr && !aligned_rows(out, ldo)) || (stats_out && !aligned_rows(stats_out, ld_stats)) ||
        (mean_out && !aligned_rows(mean_out, ld_mean)) || (argmin_out && !aligned_rows(argmin_out, ld_arg)) ||
        (argmax_out && !aligned_rows(argmax_out, ld_arg)) || (z_out && !aligned_rows(z_out, ld_z)))
      throw logic_error("y / a / x_dst / w_post / w_lin / kept rows must be 16-B aligned");
    pna_args p{};
    p.row_ptr = row_ptr, p.col = col, p.n_rows = n_rows, p.y = y, p.ldy = ldy, p.F = F, p.src_ids = src_ids;
    p.a = a, p.lda = lda, p.xd = x_dst, p.ldxd = ldx_dst, p.A = n_aggr, p.S = w_post ? n_scalers : 0;
    for (int k = 0; k < n_aggr; ++k) p.aggr[k] = aggregators[k];
    for (int k = 0; k < p.S; ++k) p.scaler[k] = scalers[k];
    p.avg_lin = avg_lin, p.avg_log = avg_log;
    p.wp = w_post, p.ldwp = ldw_post, p.N = N, p.bp = b_post, p.wl = w_lin, p.ldwl = ldw_lin, p.NO = N_out, p.bl = b_lin;
    p.relu = (flags & WGAMD_GIN_RELU_OUT) != 0;
    p.out = out, p.ldo = ldo, p.stats_out = w_post ? stats_out : out, p.ld_stats = w_post ? ld_stats : ldo;
    p.mean_out = mean_out, p.ld_mean = ld_mean, p.argmin_out = argmin_out, p.argmax_out = argmax_out, p.ld_arg = ld_arg;
    p.z_out = w_post ? z_out : nullptr, p.ld_z = ld_z;
    p.SD = (1 + n_aggr) * F + 4;
    tile_geometry(w_post ? N : 1, p.N16, p.SN);
    p.M = w_post ? pna_row_tiles(p.SD, p.SN) : 1;
    auto st = static_cast<hipStream_t>(stream);
    with_kind(kind, [&](auto k) {
      with_lane_group(F, [&](auto lg) { launch_one<decltype(k)::value, decltype(lg)::value>(p, st); });
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_pna_layer_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* y, int64_t ldy, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const float* a, int64_t lda, const float* x_dst, int64_t ldx_dst, const int* aggregators,
    int n_aggr, const int* scalers, int n_scalers, float avg_lin, float avg_log, const float* w_post, int64_t ldw_post, int N,
    const float* b_post, const float* w_lin, int64_t ldw_lin, int N_out, const float* b_lin, int flags, float* out, int64_t ldo,
    void* stream)
{
  return wgamd_pna_layer_f32_train(row_ptr, col, n_rows, y, ldy, F, src_ids, src_ids_dtype, a, lda, x_dst, ldx_dst, aggregators, n_aggr,
                                   scalers, n_scalers, avg_lin, avg_log, w_post, ldw_post, N, b_post, w_lin, ldw_lin, N_out, b_lin, flags,
                                   out, ldo, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, stream);
}

extern "C" wholememory_error_code_t wgamd_pna_bwd_src_f32(
    const int* row_ptr_t, const int* col_t, const int* perm, int64_t n_src, const float* y, int64_t ldy, int F, const void* src_ids,
    wholememory_dtype_t src_ids_dtype, const float* c0, const float* c1, int64_t ld_c, const float* meany, int64_t ld_mean,
    const float* dmax, const float* dmin, int64_t ld_d, const int* amax, const int* amin, int64_t ld_arg, float* gy, int64_t ldgy,
    int64_t n_blocks, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_pna_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    if (!pna_shape_ok(F, 0)) throw logic_error(fmt("unsupported shape: F=%d (multiple of 4, <= 256)", F));
    if (n_src == 0) return;
    const int64_t tiles = pna_tiles(n_src);
    WG_REQUIRE_INPUT(n_blocks >= 1 && n_blocks <= tiles && tiles <= INT32_MAX, "n_blocks: 1 .. the input rows' tiles of 16 rows");
    WG_REQUIRE_INPUT(row_ptr_t && col_t && y && gy, "null pointer");
    WG_REQUIRE_INPUT((c1 == nullptr) == (meany == nullptr) && (dmax == nullptr) == (amax == nullptr) && (dmin == nullptr) == (amin == nullptr),
                     "c1 comes with meany, dmax with amax, dmin with amin");
    WG_REQUIRE_INPUT(perm || (dmax == nullptr && dmin == nullptr), "dmax / dmin need perm");
    const int kind = ids_kind(src_ids, src_ids_dtype);
    WG_REQUIRE_INPUT((kind == 3 || ldy >= F) && ldgy >= F && ((c0 == nullptr && c1 == nullptr) || ld_c >= F) && (c1 == nullptr || ld_mean >= F) &&
                       ((dmax == nullptr && dmin == nullptr) || (ld_d >= F && ld_arg >= F)), "leading dimension too small");
    if (!aligned_rows(y, kind == 3 ? 0 : ldy) || !aligned_rows(gy, ldgy) || (c0 && !aligned_rows(c0, ld_c)) ||
        (c1 && (!aligned_rows(c1, ld_c) || !aligned_rows(meany, ld_mean))) || (dmax && (!aligned_rows(dmax, ld_d) || !aligned_rows(amax, ld_arg))) ||
        (dmin && (!aligned_rows(dmin, ld_d) || !aligned_rows(amin, ld_arg))))
      throw logic_error("y / gy / c0 / c1 / meany / dmax / dmin / amax / amin rows must be 16-B aligned");
    pna_src_args a{};
    a.row_ptr_t = row_ptr_t, a.col_t = col_t, a.perm = (dmax || dmin) ? perm : nullptr, a.n_src = n_src, a.n_tiles = (int)tiles;
    a.y = y, a.ldy = ldy, a.src_ids = src_ids, a.F = F, a.c0 = c0, a.c1 = c1, a.ld_c = ld_c, a.meany = meany, a.ld_mean = ld_mean;
    a.dmax = dmax, a.dmin = dmin, a.ld_d = ld_d, a.amax = amax, a.amin = amin, a.ld_arg = ld_arg, a.gy = gy, a.ldgy = ldgy;
    a.lg_shift = 2;
    while ((1 << a.lg_shift) < F / 4) ++a.lg_shift;
    const dim3 grid((unsigned)n_blocks);
    auto st = static_cast<hipStream_t>(stream);
    with_kind(kind, [&](auto k) { pna_bwd_src_kernel<decltype(k)::value><<<grid, kThreads, 0, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}
