// The row-wise block between two message-passing layers, for all node types of a layer in ONE launch:
//     z   = x (+ residual)
//     y   = LayerNorm(z; weight, bias, eps)        (NORM; torch.nn.LayerNorm: biased variance, rstd = 1 / sqrt(var + eps))
//     y   = keep ? y / (1 - p) : 0                 (p > 0)
//     out = relu(y)                                (RELU)
// the order of the reference's mag_lp_mnmg.py encoder (norm -> dropout -> relu); ReLU and dropout commute (the scale is >= 0), so
// it is also gnn_model.py's relu -> dropout with NORM off.
//
// Pieces:
//   * norm_act_fwd_kernel / norm_act_bwd_kernel — a segment (one node type's [n_rows, C] problem) owns a run of workgroups, found
//     through the prefix of the segments' workgroup counts; a workgroup walks its segment's row tiles with a fixed stride.  A
//     row is held in registers by a group of LG = 4 .. 64 lanes (one float4 per lane up to C = 256, then 2 .. 4 per lane of a whole
//     wave), so a 256-thread workgroup works on 256 / LG rows at a time; the segment's class (LG, float4s per lane) is uniform in
//     the workgroup and picked by a switch.  Row sums are xor shuffles inside the group: the mean, then the centred sum of
//     squares over the registers (never E[z^2] - mean^2).
//   * the keep mask is stateless: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) keyed with
//     the segment's seed, counter = (float4 column, row low, row high, 0), one call per float4 of columns.  keep(r, c) depends on
//     (segment seed, row in the segment, c) only; the backward draws it again and reads neither `out` nor a stored mask.
//   * the backward recomputes z, x^ (from the saved mean, rstd), y, the ReLU sign and the mask with the forward's own inline
//     functions, writes dz once (the gradient of x AND of the residual) and sums gy x^ and gy over the rows of the workgroup in
//     registers, then over its row groups through LDS in group order -> partials[workgroup][2][C].
//   * norm_act_wgrad_kernel adds the partial rows in workgroup order.  No atomics anywhere: the same bits on every run.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kNaThreads = 256;
constexpr int kNaFwdBlocks = 2048;   // workgroups per segment at most (forward): 8 per CU
constexpr int kNaBwdBlocks = 1024;   // (backward): the partial rows the weight-gradient launch adds up
constexpr int kWgCols = 64, kWgLanes = 16;      // norm_act_wgrad_kernel: 64 columns x 16 partial-row lanes per workgroup

struct na_seg {
  const float* x;
  const float* res;
  float* out;
  const float* w;
  const float* b;
  float* stats;
  const float* g;
  float* gi;
  float* part;
  float* dw;
  float* db;
  int64_t ldx, ld_res, ldo, ldg, ld_gi, n_rows;
  uint32_t key0, key1;
  int C, cls, blocks;
};

struct na_args {
  na_seg s[WGAMD_NORM_ACT_MAX_SEGMENTS];
  int first[WGAMD_NORM_ACT_MAX_SEGMENTS + 1];   // prefix of the segments' workgroup counts
  int n_segs;
  float eps, scale;
  uint32_t thr;        // keep <=> u32 >= thr
  int drop;            // 0: no dropout, 1: by thr, 2: p = 1 (nothing is kept)
  int norm, relu, save;
};

inline uint64_t mix64(uint64_t z)      // the splitmix64 output function (Steele, Lea, Flood 2014)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

inline int lanes_class(int C)          // 0..4: 4/8/16/32/64 lanes, one float4 each; 5..7: a wave, 2/3/4 float4 per lane
{
  const int c4 = C / 4;
  if (c4 <= 4) return 0;
  if (c4 <= 8) return 1;
  if (c4 <= 16) return 2;
  if (c4 <= 32) return 3;
  return 4 + (c4 - 1) / 64;
}
inline int lanes_of(int cls) { return cls >= 4 ? 64 : 4 << cls; }

inline int seg_blocks(int64_t n_rows, int C, int cap)
{
  const int rp = kNaThreads / lanes_of(lanes_class(C));
  const int64_t tiles = (n_rows + rp - 1) / rp;
  return (int)std::min<int64_t>(tiles, cap);
}

// ---- device pieces shared by the forward and the backward -------------------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1, c[3] = (uint32_t)p0, c[0] = n0, c[2] = n2;
}

// Philox4x32-10: four words for columns [4 c4, 4 c4 + 4) of row r
__device__ __forceinline__ void philox4(uint32_t k0, uint32_t k1, int64_t r, int c4, uint32_t (&u)[4])
{
  u[0] = (uint32_t)c4, u[1] = (uint32_t)(uint64_t)r, u[2] = (uint32_t)((uint64_t)r >> 32), u[3] = 0u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(u, k0, k1);
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

template <int LG>
__device__ __forceinline__ float group_sum(float v)
{
#pragma unroll
  for (int m = LG / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

template <int LG, int NV>
__device__ __forceinline__ void load_vec(const float* p, int c, int C4, bool ok, float fill, f32x4 (&v)[NV])
{
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    v[k] = f32x4{fill, fill, fill, fill};
    if (ok && p && c + k * LG < C4) v[k] = reinterpret_cast<const f32x4*>(p)[c + k * LG];
  }
}

// z = x (+ residual) of row r: zeros in lanes past the row's end and in rows past the segment's
template <int LG, int NV>
__device__ __forceinline__ void load_z(const na_seg& s, int64_t r, int c, int C4, bool ok, f32x4 (&z)[NV])
{
  load_vec<LG, NV>(s.x + r * s.ldx, c, C4, ok, 0.f, z);
  if (s.res) {
    f32x4 t[NV];
    load_vec<LG, NV>(s.res + r * s.ld_res, c, C4, ok, 0.f, t);
#pragma unroll
    for (int k = 0; k < NV; ++k) z[k] += t[k];
  }
}

// y = x^ w + b, one fused multiply-add per element (the backward's ReLU sign is the forward's)
template <int NV>
__device__ __forceinline__ void affine(const f32x4 (&xh)[NV], const f32x4 (&w)[NV], const f32x4 (&b)[NV], f32x4 (&y)[NV])
{
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) y[k][e] = __builtin_fmaf(xh[k][e], w[k][e], b[k][e]);
}

// the factor of element e of the float4 at column c4: keep / (1 - p), then the ReLU gate of y
__device__ __forceinline__ float gate(const na_args& a, const uint32_t (&u)[4], int e, float y)
{
  float f = 1.f;
  if (a.drop) f = (a.drop == 1 && u[e] >= a.thr) ? a.scale : 0.f;
  if (a.relu && y <= 0.f) f = 0.f;
  return f;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int LG, int NV>
__device__ __forceinline__ void fwd_rows(const na_args& a, const na_seg& s, int blk)
{
  constexpr int RP = kNaThreads / LG;
  const int grp = threadIdx.x / LG, c = threadIdx.x % LG, C4 = s.C / 4;
  const int64_t tiles = (s.n_rows + RP - 1) / RP;
  const float fc = (float)s.C;
  f32x4 w[NV], b[NV];
  load_vec<LG, NV>(s.w, c, C4, true, 1.f, w);
  load_vec<LG, NV>(s.b, c, C4, true, 0.f, b);
  for (int64_t t = blk; t < tiles; t += s.blocks) {
    const int64_t r = t * RP + grp;
    const bool ok = r < s.n_rows;
    f32x4 z[NV], y[NV];
    load_z<LG, NV>(s, r, c, C4, ok, z);
    if (a.norm) {
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) sum += sum4(z[k]);
      const float mean = group_sum<LG>(sum) / fc;
      float sq = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        z[k] = c + k * LG < C4 ? z[k] - mean : f32x4{0.f, 0.f, 0.f, 0.f};
        sq += sum4(z[k] * z[k]);
      }
      const float rstd = 1.f / sqrtf(group_sum<LG>(sq) / fc + a.eps);
#pragma unroll
      for (int k = 0; k < NV; ++k) z[k] *= rstd;
      affine<NV>(z, w, b, y);
      if (a.save && ok && c == 0) reinterpret_cast<float2*>(s.stats)[r] = make_float2(mean, rstd);
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) y[k] = z[k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c4 = c + k * LG;
      if (!ok || c4 >= C4) continue;
      uint32_t u[4] = {0u, 0u, 0u, 0u};
      if (a.drop == 1) philox4(s.key0, s.key1, r, c4, u);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = gate(a, u, e, y[k][e]);
        o[e] = f != 0.f ? y[k][e] * f : 0.f;
      }
      reinterpret_cast<f32x4*>(s.out + r * s.ldo)[c4] = o;
    }
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
template <int LG, int NV>
__device__ __forceinline__ void bwd_rows(const na_args& a, const na_seg& s, int blk, float* lds)
{
  constexpr int RP = kNaThreads / LG;
  const int grp = threadIdx.x / LG, c = threadIdx.x % LG, C4 = s.C / 4;
  const int64_t tiles = (s.n_rows + RP - 1) / RP;
  const float fc = (float)s.C;
  const bool sums = a.norm && s.part != nullptr;
  f32x4 w[NV], b[NV], dw[NV], db[NV];
  load_vec<LG, NV>(s.w, c, C4, true, 1.f, w);
  load_vec<LG, NV>(s.b, c, C4, true, 0.f, b);
#pragma unroll
  for (int k = 0; k < NV; ++k) dw[k] = db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t t = blk; t < tiles; t += s.blocks) {
    const int64_t r = t * RP + grp;
    const bool ok = r < s.n_rows;
    f32x4 z[NV], y[NV], gy[NV];
    load_z<LG, NV>(s, r, c, C4, ok, z);
    load_vec<LG, NV>(s.g + r * s.ldg, c, C4, ok, 0.f, gy);
    float mean = 0.f, rstd = 0.f;
    if (a.norm) {
      if (ok) {
        const float2 st = reinterpret_cast<const float2*>(s.stats)[r];
        mean = st.x, rstd = st.y;
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) z[k] = c + k * LG < C4 ? (z[k] - mean) * rstd : f32x4{0.f, 0.f, 0.f, 0.f};
      affine<NV>(z, w, b, y);
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) y[k] = z[k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c4 = c + k * LG;
      uint32_t u[4] = {0u, 0u, 0u, 0u};
      if (a.drop == 1 && ok && c4 < C4) philox4(s.key0, s.key1, r, c4, u);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = gate(a, u, e, y[k][e]);
        gy[k][e] = f != 0.f ? gy[k][e] * f : 0.f;
      }
    }
    if (a.norm) {
      // dz = rstd (w gy - mean_c(w gy) - x^ mean_c(w gy x^))      (z holds x^; gy = 0 past the row's end)
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        dw[k] += gy[k] * z[k], db[k] += gy[k];
        gy[k] *= w[k];
        s1 += sum4(gy[k]), s2 += sum4(gy[k] * z[k]);
      }
      const float m1 = group_sum<LG>(s1) / fc, m2 = group_sum<LG>(s2) / fc;
#pragma unroll
      for (int k = 0; k < NV; ++k) gy[k] = (gy[k] - m1 - z[k] * m2) * rstd;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (ok && c + k * LG < C4) reinterpret_cast<f32x4*>(s.gi + r * s.ld_gi)[c + k * LG] = gy[k];
  }
  if (!sums) return;
  // the row groups' sums through LDS, added in group order: partials[workgroup][0][:] = sum gy x^, [1][:] = sum gy
  const int C2 = 2 * s.C;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (c + k * LG < C4) {
      reinterpret_cast<f32x4*>(lds + grp * C2)[c + k * LG] = dw[k];
      reinterpret_cast<f32x4*>(lds + grp * C2 + s.C)[c + k * LG] = db[k];
    }
  __syncthreads();
  for (int i = threadIdx.x; i < C2; i += kNaThreads) {
    float acc = 0.f;
    for (int q = 0; q < RP; ++q) acc += lds[q * C2 + i];
    s.part[(int64_t)blk * C2 + i] = acc;
  }
}

__device__ __forceinline__ int segment_of(const na_args& a, int block)
{
  int k = 0;
  while (k + 1 < a.n_segs && block >= a.first[k + 1]) ++k;
  return k;
}

// WIDE = false: every segment of the launch holds a row in one float4 per lane (C <= 256, the common hidden widths) — the
// kernel then carries the registers of that form only
#define WG_NA_CLASSES(CALL)                      \
  switch (s.cls) {                               \
    case 0: CALL(4, 1);                          \
    case 1: CALL(8, 1);                          \
    case 2: CALL(16, 1);                         \
    case 3: CALL(32, 1);                         \
    case 4: CALL(64, 1);                         \
    default:                                     \
      if constexpr (WIDE) {                      \
        if (s.cls == 5) { CALL(64, 2); }         \
        if (s.cls == 6) { CALL(64, 3); }         \
        CALL(64, 4);                             \
      }                                          \
  }

template <bool WIDE>
__global__ void __launch_bounds__(kNaThreads) norm_act_fwd_kernel(na_args a)
{
  const int k = segment_of(a, blockIdx.x);
  const na_seg& s = a.s[k];
  const int blk = blockIdx.x - a.first[k];
#define WG_NA_FWD(LG, NV) fwd_rows<LG, NV>(a, s, blk); return
  WG_NA_CLASSES(WG_NA_FWD)
#undef WG_NA_FWD
}

template <bool WIDE>
__global__ void __launch_bounds__(kNaThreads) norm_act_bwd_kernel(na_args a)
{
  extern __shared__ __attribute__((aligned(16))) float na_lds[];
  const int k = segment_of(a, blockIdx.x);
  const na_seg& s = a.s[k];
  const int blk = blockIdx.x - a.first[k];
#define WG_NA_BWD(LG, NV) bwd_rows<LG, NV>(a, s, blk, na_lds); return
  WG_NA_CLASSES(WG_NA_BWD)
#undef WG_NA_BWD
}

// dweight[c] = sum over the partial rows of part[b][0][c], dbias[c] = ... part[b][1][c]: lane q of 16 adds rows q, q + 16, ...
// in order, then the 16 lane sums are added in lane order.  grid (ceil(2 C / 64), n_segs)
__global__ void __launch_bounds__(kWgCols* kWgLanes) norm_act_wgrad_kernel(na_args a)
{
  __shared__ float t[kWgLanes][kWgCols];
  const na_seg& s = a.s[blockIdx.y];
  const int C2 = 2 * s.C, col = threadIdx.x % kWgCols, q = threadIdx.x / kWgCols;
  const int i = blockIdx.x * kWgCols + col;
  if (blockIdx.x * kWgCols >= C2 || (s.dw == nullptr && s.db == nullptr)) return;      // (uniform in the workgroup)
  float acc = 0.f;
  if (i < C2 && s.part)
    for (int b = q; b < s.blocks; b += kWgLanes) acc += s.part[(int64_t)b * C2 + i];
  t[q][col] = acc;
  __syncthreads();
  if (q != 0 || i >= C2) return;
  acc = 0.f;
  for (int k = 0; k < kWgLanes; ++k) acc += t[k][col];
  if (i < s.C) {
    if (s.dw) s.dw[i] = acc;
  } else if (s.db) {
    s.db[i - s.C] = acc;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline bool vec_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// checks the segments (`bwd`: the gradient fields too) and fills the launch's table; false when every segment is empty
bool make_args(na_args& a, const wgamd_norm_act_segment* segs, int n_segs, float eps, float p, uint64_t seed, int flags, bool bwd,
               int cap)
{
  WG_REQUIRE_INPUT(n_segs >= 1 && n_segs <= WGAMD_NORM_ACT_MAX_SEGMENTS, "n_segs = %d: 1 .. %d segments per launch", n_segs,
                   WGAMD_NORM_ACT_MAX_SEGMENTS);
  WG_REQUIRE_INPUT(segs != nullptr, "null segment table");
  WG_REQUIRE_INPUT(p >= 0.f && p <= 1.f && eps >= 0.f, "p must be in [0, 1] and eps >= 0");
  a = na_args{};
  a.n_segs = n_segs, a.eps = eps;
  a.norm = (flags & WGAMD_NORM_ACT_NORM) != 0, a.relu = (flags & WGAMD_NORM_ACT_RELU) != 0;
  a.save = (flags & WGAMD_NORM_ACT_SAVE_STATS) != 0;
  a.drop = p <= 0.f ? 0 : p >= 1.f ? 2 : 1;
  a.thr = a.drop == 1 ? (uint32_t)std::min<uint64_t>((uint64_t)((double)p * 4294967296.0), 0xFFFFFFFFull) : 0u;
  a.scale = a.drop == 1 ? 1.f / (1.f - p) : 0.f;
  int64_t total = 0;
  for (int k = 0; k < n_segs; ++k) {
    const wgamd_norm_act_segment& g = segs[k];
    na_seg& s = a.s[k];
    WG_REQUIRE_INPUT(g.n_rows >= 0, "segment %d: n_rows < 0", k);
    if (!wgamd_norm_act_supported(g.C)) throw logic_error(fmt("segment %d: unsupported width C=%d (multiple of 4, 4 .. 1024)", k, g.C));
    a.first[k] = (int)total;
    s.C = g.C, s.cls = lanes_class(g.C), s.n_rows = g.n_rows;
    if (g.n_rows == 0) continue;
    WG_REQUIRE_INPUT(g.x != nullptr && (bwd ? g.grad_out && g.grad_in : g.out != nullptr), "segment %d: null pointer", k);
    WG_REQUIRE_INPUT(g.ldx >= g.C && (g.residual == nullptr || g.ld_res >= g.C), "segment %d: leading dimension too small", k);
    WG_REQUIRE_INPUT(bwd ? g.ldg >= g.C && g.ld_gi >= g.C : g.ldo >= g.C, "segment %d: leading dimension too small", k);
    WG_REQUIRE_INPUT(!(a.norm && (bwd || a.save)) || g.stats != nullptr, "segment %d: null stats", k);
    if (!aligned_rows(g.x, g.ldx) || (g.residual && !aligned_rows(g.residual, g.ld_res)) ||
        (bwd ? !aligned_rows(g.grad_out, g.ldg) || !aligned_rows(g.grad_in, g.ld_gi) : !aligned_rows(g.out, g.ldo)) ||
        !vec_ok(g.weight) || !vec_ok(g.bias) || (reinterpret_cast<uintptr_t>(g.stats) & 7) || !vec_ok(g.partials))
      throw logic_error(fmt("segment %d: x / residual / out / grad rows, weight, bias and partials must be 16-B aligned "
                            "(leading dimensions multiples of 4), stats 8-B aligned", k));
    s.x = g.x, s.ldx = g.ldx, s.res = g.residual, s.ld_res = g.ld_res, s.out = g.out, s.ldo = g.ldo;
    s.w = a.norm ? g.weight : nullptr, s.b = a.norm ? g.bias : nullptr, s.stats = g.stats;
    if (bwd) s.g = g.grad_out, s.ldg = g.ldg, s.gi = g.grad_in, s.ld_gi = g.ld_gi, s.part = g.partials;
    const uint64_t key = g.seed_index < 0 ? seed : wgamd_norm_act_segment_seed(seed, g.seed_index);
    s.key0 = (uint32_t)key, s.key1 = (uint32_t)(key >> 32);
    s.blocks = seg_blocks(g.n_rows, g.C, cap);
    total += s.blocks;
  }
  a.first[n_segs] = (int)total;
  return total > 0;
}

bool wide_launch(const na_args& a)
{
  for (int k = 0; k < a.n_segs; ++k)
    if (a.s[k].blocks > 0 && a.s[k].cls > 4) return true;
  return false;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_norm_act_supported(int C) { return C % 4 == 0 && C >= 4 && C <= 1024; }

extern "C" uint64_t wgamd_norm_act_segment_seed(uint64_t seed, int k)
{
  return wgamd::mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)(int64_t)k + 1));
}

extern "C" int64_t wgamd_norm_act_bwd_blocks(int64_t n_rows, int C)
{
  if (n_rows <= 0 || !wgamd_norm_act_supported(C)) return 0;
  return wgamd::seg_blocks(n_rows, C, wgamd::kNaBwdBlocks);
}

extern "C" wholememory_error_code_t wgamd_norm_act_f32(const wgamd_norm_act_segment* segs, int n_segs, float eps, float p,
                                                       uint64_t seed, int flags, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_norm_act_f32", [&] {
    na_args a;
    if (!make_args(a, segs, n_segs, eps, p, seed, flags, false, kNaFwdBlocks)) return;
    auto kern = wide_launch(a) ? norm_act_fwd_kernel<true> : norm_act_fwd_kernel<false>;
    kern<<<(unsigned)a.first[n_segs], kNaThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_norm_act_bwd_f32(const wgamd_norm_act_segment* segs, int n_segs, float eps, float p,
                                                           uint64_t seed, int flags, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_norm_act_bwd_f32", [&] {
    na_args a;
    if (!make_args(a, segs, n_segs, eps, p, seed, flags, true, kNaBwdBlocks)) return;
    size_t lds = 0;      // (256 / LG) row groups x 2 C floats: 8 KB up to C = 256, 32 KB at C = 1024
    for (int k = 0; k < n_segs; ++k)
      if (a.norm && a.s[k].part) lds = std::max(lds, (size_t)(kNaThreads / lanes_of(a.s[k].cls)) * 2 * a.s[k].C * sizeof(float));
    auto kern = wide_launch(a) ? norm_act_bwd_kernel<true> : norm_act_bwd_kernel<false>;
    kern<<<(unsigned)a.first[n_segs], kNaThreads, lds, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_norm_act_wgrad_f32(const wgamd_norm_act_segment* segs, int n_segs, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_norm_act_wgrad_f32", [&] {
    WG_REQUIRE_INPUT(n_segs >= 1 && n_segs <= WGAMD_NORM_ACT_MAX_SEGMENTS && segs != nullptr, "n_segs = %d: 1 .. %d segments per launch",
                     n_segs, WGAMD_NORM_ACT_MAX_SEGMENTS);
    na_args a{};
    a.n_segs = n_segs;
    int max_c = 0;
    for (int k = 0; k < n_segs; ++k) {
      const wgamd_norm_act_segment& g = segs[k];
      if (!wgamd_norm_act_supported(g.C)) throw logic_error(fmt("segment %d: unsupported width C=%d (multiple of 4, 4 .. 1024)", k, g.C));
      const bool wanted = g.dweight != nullptr || g.dbias != nullptr;      // (a segment with neither is skipped: no partials needed)
      WG_REQUIRE_INPUT(g.n_rows >= 0 && (!wanted || g.n_rows == 0 || g.partials != nullptr), "segment %d: null partials", k);
      a.s[k].C = g.C, a.s[k].part = g.partials, a.s[k].dw = g.dweight, a.s[k].db = g.dbias;
      a.s[k].blocks = (int)wgamd_norm_act_bwd_blocks(g.n_rows, g.C);      // no partial rows: zeros
      if (g.dweight || g.dbias) max_c = std::max(max_c, g.C);
    }
    if (max_c == 0) return;
    const dim3 grid((unsigned)((2 * max_c + kWgCols - 1) / kWgCols), (unsigned)n_segs);
    norm_act_wgrad_kernel<<<grid, kWgCols * kWgLanes, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
