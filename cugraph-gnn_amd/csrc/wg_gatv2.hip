// GATv2 attention (torch_geometric.nn.GATv2Conv, flow source_to_target) over a sampled hop, on TRANSFORMED rows:
//     s_ij    = XL[j] + XR[i]                                   (XL = lin_l(x_src), XR = lin_r(x_dst): library GEMMs of the caller)
//     e_ijh   = sum_c att[h, c] LeakyReLU(s_ij[h, c])
//     alpha   = softmax_j(e_ijh)                                (per destination row and head)
//     agg_ih  = sum_j alpha_ijh XL[j, h, :]
//     out_i   = act( concat_h agg_ih  or  mean_h agg_ih,  + bias )
// The nonlinearity sits between the sum of the two rows and the dot product with att, so the logit is not linear in the raw
// neighbour row and the aggregate-first form of wg_transformer.hip / wg_gat_fused.hip does not exist: the transformed neighbour
// row is read per edge — once, the registers that scored it accumulate it.  Self loops are ordinary leading entries of the CSR
// (HopGraph.with_self_loops).
//
// Pieces (all: one wave per row, lane = one float4 of the H C <= 256 wide row, so a lane's four columns lie in ONE head as
// C % 4 == 0, and a lane keeps the softmax state of its own head only):
//   * gatv2_attention_kernel — the whole attention of a hop in one launch.  The row's edges go by in groups of 4 (4 neighbour
//     rows in flight); a head's logit is the sum over the head's C / 4 lanes: xor butterflies inside the head's lanes when C / 4
//     is a power of two, else H masked wave sums — either way every lane of a head ends with the same bits.  Online softmax as
//     in tconv_row_walk (running max and sum, accumulators rescaled once per group, a group's terms summed before they join
//     them).  Bias, ReLU, the head mean of concat=False and the output row offset (out / ldo) are fused.  When training the
//     logits go to alpha [E, H] as they are made and become alpha in a second pass over the row; agg [n_rows, H C] is kept.
//   * gatv2_bwd_dst_kernel — destination-major, given G = dL/d agg: dalpha = G_ih . XL[j, h], de = alpha (dalpha - G_ih . agg_ih),
//     dXR[i] = sum_j de att * LeakyReLU'(s_ij), de written [E, H]; datt = sum_ij de LeakyReLU(s_ij) leaves as ONE partial row
//     per workgroup of 16 rows (the four waves' sums added in wave order), summed by the caller in a fixed order.
//   * gatv2_bwd_src_kernel — source-major over the hop's transpose (HopGraph.transposed with the edge permutation):
//     dXL[j] = sum_e (alpha_e G_i + de_e att * LeakyReLU'(XL[j] + XR[i])), entries added in transposed-CSR order (a hub source
//     is one wave's sequential walk, four entries in flight).
// No atomics anywhere: the same bits from run to run.
#include "wg_transformer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kGatv2MaxHC   = 256;    // one float4 of the row per lane
constexpr int kGatv2BwdRows = 16;     // destination rows per workgroup of the destination-major backward (4 per wave)

// the sum of v over the lanes of head hd; LPH = lanes per head when that is a power of two (butterflies inside the head's lanes:
// the idle lanes behind the row form groups of their own, H LPH being a multiple of LPH), 0 = any C / 4 (H masked wave sums)
template <int LPH>
__device__ __forceinline__ float head_sum(float v, int hd, int H)
{
  if constexpr (LPH > 0) {
#pragma unroll
    for (int o = LPH / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  } else {
    float mine = 0.f;
    for (int h = 0; h < H; ++h) {
      const float s = wave_sum(hd == h ? v : 0.f);
      if (hd == h) mine = s;
    }
    return mine;
  }
}

// launch(std::integral_constant<int, LPH>{}) for C channels per head
template <typename Launch>
void with_head_lanes(int C, Launch&& launch)
{
  switch (C / 4) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    case 16: launch(std::integral_constant<int, 16>{}); break;
    case 32: launch(std::integral_constant<int, 32>{}); break;
    case 64: launch(std::integral_constant<int, 64>{}); break;
    default: launch(std::integral_constant<int, 0>{}); break;
  }
}

struct gatv2_args {
  const int* row_ptr;
  const int* col;             // rows of xl
  int64_t n_rows;
  const float* xl;            // [n_src, ldxl]
  int64_t ldxl;
  const float* xr;            // XR[i] = xr[xr_rows ? xr_rows[i] : i]
  int64_t ldxr;
  const int64_t* xr_rows;
  const float* att;           // [H C]
  int H, C;
  float slope;
  const float* bias;          // [H C], or [C] with mean; nullable
  int relu, mean;
  float* out;                 // [n_rows, ldo]: H C wide, C with mean
  int64_t ldo;
  float* alpha;               // [E, H] or null
  float* agg;                 // [n_rows, H C] or null
};

template <int LPH>
__global__ void __launch_bounds__(256) gatv2_attention_kernel(gatv2_args a)
{
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_rows) return;                      // (wave-uniform; the kernel has no barrier)
  const int H = a.H, lph = a.C / 4, HC = H * a.C;
  const bool on = lane < H * lph;
  const int hd = on ? lane / lph : H;             // (H: no head — an idle lane)
  const bool lead = on && lane == hd * lph;       // the lane that writes its head's logits
  const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
  f32x4 att4 = {0.f, 0.f, 0.f, 0.f}, xr4 = att4, acc = att4;
  float m = -INFINITY, l = 0.f;
  if (on && s < t) {
    att4 = reinterpret_cast<const f32x4*>(a.att)[lane];
    xr4  = reinterpret_cast<const f32x4*>(a.xr + (a.xr_rows ? a.xr_rows[i] : i) * a.ldxr)[lane];
  }
  for (int e0 = s; e0 < t; e0 += 4) {
    f32x4 xv[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e0 + v < t && on) xv[v] = reinterpret_cast<const f32x4*>(a.xl + (int64_t)a.col[e0 + v] * a.ldxl)[lane];
    }
    float sc[4];
    float mx = m;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      f32x4 z = xv[v] + xr4;
#pragma unroll
      for (int k = 0; k < 4; ++k) z[k] = z[k] > 0.f ? z[k] : a.slope * z[k];
      sc[v] = head_sum<LPH>(dot4(att4, z), hd, H);
      if (e0 + v < t) mx = fmaxf(mx, sc[v]);
    }
    const float r = expf(m - mx);                 // (m = -inf before the first group: r = 0)
    acc *= r;
    l *= r;
    f32x4 ga = {0.f, 0.f, 0.f, 0.f};              // the group's terms join the running sums as ONE term (tconv_row_walk)
    float gl = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (e0 + v < t) {
        const float p = expf(sc[v] - mx);
        ga += p * xv[v];
        gl += p;
        if (a.alpha && lead) a.alpha[(int64_t)(e0 + v) * H + hd] = sc[v];     // the logit; alpha after the row
      }
    }
    acc += ga;
    l += gl;
    m = mx;
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;      // (no edges: acc = 0 and inv = 0 — the aggregate is exactly zero)
  const f32x4 o = acc * inv;
  if (a.agg && on) reinterpret_cast<f32x4*>(a.agg + i * HC)[lane] = o;
  if (!a.mean) {
    if (on) {
      f32x4 y = o;
      if (a.bias) y += reinterpret_cast<const f32x4*>(a.bias)[lane];
      if (a.relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fmaxf(y[k], 0.f);
      }
      reinterpret_cast<f32x4*>(a.out + i * a.ldo)[lane] = y;
    }
  } else {
    // the head mean: lane q < C / 4 adds the H lanes that hold its columns, in head order (every lane takes part in the reads)
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    const int q = lane % lph;
    for (int h = 0; h < H; ++h) {
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] += __shfl(o[k], h * lph + q, 64);
    }
    if (lane < lph) {
      y *= 1.f / (float)H;
      if (a.bias) y += reinterpret_cast<const f32x4*>(a.bias)[lane];
      if (a.relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fmaxf(y[k], 0.f);
      }
      reinterpret_cast<f32x4*>(a.out + i * a.ldo)[lane] = y;
    }
  }
  if (a.alpha && s < t) {
    __threadfence_block();                        // the logits this wave wrote, read back by other lanes
    float* base = a.alpha + (int64_t)s * H;
    const int n = (t - s) * H;
    for (int b = 0; b < n; b += 64) {             // (a uniform trip count: every lane is a source of the two reads)
      const int idx = b + lane;
      const int src = (idx % H) * lph;            // the first lane of the entry's head
      const float mh = __shfl(m, src, 64), lh = __shfl(inv, src, 64);
      if (idx < n) base[idx] = expf(base[idx] - mh) * lh;
    }
  }
}

// ---- destination-major backward -------------------------------------------------------------------------------------------
struct gatv2_bwd_args {
  const int* row_ptr;
  const int* col;
  int64_t n_rows;
  const float* xl;
  int64_t ldxl;
  const float* xr;
  int64_t ldxr;
  const int64_t* xr_rows;
  const float* att;
  int H, C;
  float slope;
  const float* alpha;         // [E, H]
  const float* g;             // [n_rows, ldg] = dL/d agg
  int64_t ldg;
  const float* agg;           // [n_rows, H C]
  float* dxr;                 // [n_rows, H C]
  float* de;                  // [E, H]
  float* datt_part;           // [n_blocks, H C]
};

template <int LPH>
__global__ void __launch_bounds__(256) gatv2_bwd_dst_kernel(gatv2_bwd_args a)
{
  __shared__ f32x4 part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kGatv2BwdRows;
  const int H = a.H, lph = a.C / 4, HC = H * a.C;
  const bool on = lane < H * lph;
  const int hd = on ? lane / lph : H;
  const bool lead = on && lane == hd * lph;
  f32x4 att4 = {0.f, 0.f, 0.f, 0.f}, da = att4;
  if (on) att4 = reinterpret_cast<const f32x4*>(a.att)[lane];
  for (int r = wave; r < kGatv2BwdRows; r += 4) {
    const int64_t i = row0 + r;
    if (i >= a.n_rows) break;                     // (wave-uniform)
    const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
    f32x4 g4 = {0.f, 0.f, 0.f, 0.f}, xr4 = g4, ag = g4, dx = g4;
    if (on) {
      g4 = reinterpret_cast<const f32x4*>(a.g + i * a.ldg)[lane];
      ag = reinterpret_cast<const f32x4*>(a.agg + i * HC)[lane];
      if (s < t) xr4 = reinterpret_cast<const f32x4*>(a.xr + (a.xr_rows ? a.xr_rows[i] : i) * a.ldxr)[lane];
    }
    const float rdot = head_sum<LPH>(dot4(g4, ag), hd, H);        // sum_j alpha dalpha = G_ih . agg_ih
    for (int e0 = s; e0 < t; e0 += 4) {
      f32x4 xv[4];
      float al[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        al[v] = 0.f;
        if (e0 + v < t && on) {
          xv[v] = reinterpret_cast<const f32x4*>(a.xl + (int64_t)a.col[e0 + v] * a.ldxl)[lane];
          al[v] = a.alpha[(int64_t)(e0 + v) * H + hd];
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float dal = head_sum<LPH>(dot4(g4, xv[v]), hd, H);
        if (e0 + v < t) {
          const float dev = al[v] * (dal - rdot);
          const f32x4 z = xv[v] + xr4;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool pos = z[k] > 0.f;
            dx[k] += dev * att4[k] * (pos ? 1.f : a.slope);
            da[k] += dev * (pos ? z[k] : a.slope * z[k]);
          }
          if (lead) a.de[(int64_t)(e0 + v) * H + hd] = dev;
        }
      }
    }
    if (on) reinterpret_cast<f32x4*>(a.dxr + i * HC)[lane] = dx;
  }
  part[wave][lane] = da;
  __syncthreads();
  if (wave == 0 && on)
    reinterpret_cast<f32x4*>(a.datt_part + (int64_t)blockIdx.x * HC)[lane] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// ---- source-major backward: the transformed source rows' gradient ---------------------------------------------------------
struct gatv2_src_args {
  const int* row_ptr_t;
  const int* col_t;           // destination row of every transposed entry
  const int* perm;            // its CSR edge
  int64_t n_src;
  const float* xl;
  int64_t ldxl;
  const float* xr;
  int64_t ldxr;
  const int64_t* xr_rows;
  const float* att;
  int H, C;
  float slope;
  const float* alpha;
  const float* de;
  const float* g;
  int64_t ldg;
  float* gx;                  // [n_src, ldgx]
  int64_t ldgx;
  int accumulate;
};

__global__ void __launch_bounds__(256) gatv2_bwd_src_kernel(gatv2_src_args a)
{
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lph = a.C / 4, H = a.H;
  if (j >= a.n_src || lane >= H * lph) return;
  const int hd = lane / lph;
  const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (s < t) {
    const f32x4 att4 = reinterpret_cast<const f32x4*>(a.att)[lane];
    const f32x4 xl4  = reinterpret_cast<const f32x4*>(a.xl + j * a.ldxl)[lane];
    for (int p0 = s; p0 < t; p0 += 4) {
      f32x4 gv[4], xr[4];
      float al[4], dv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        gv[v] = xr[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        al[v] = dv[v] = 0.f;
        if (p0 + v < t) {
          const int64_t i = a.col_t[p0 + v], e = a.perm[p0 + v];
          gv[v] = reinterpret_cast<const f32x4*>(a.g + i * a.ldg)[lane];
          xr[v] = reinterpret_cast<const f32x4*>(a.xr + (a.xr_rows ? a.xr_rows[i] : i) * a.ldxr)[lane];
          al[v] = a.alpha[e * H + hd];
          dv[v] = a.de[e * H + hd];
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {               // (entries join in transposed-CSR order)
        if (p0 + v < t) {
          const f32x4 z = xl4 + xr[v];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += al[v] * gv[v][k] + dv[v] * att4[k] * (z[k] > 0.f ? 1.f : a.slope);
        }
      }
    }
  }
  f32x4* o = reinterpret_cast<f32x4*>(a.gx + j * a.ldgx) + lane;
  *o = a.accumulate ? *o + acc : acc;
}

void gatv2_require_shape(int H, int C)
{
  if (!wgamd_gatv2_supported(H, C))
    throw logic_error(fmt("unsupported shape: H=%d (1 .. %d), C=%d (a multiple of 4), H C <= %d", H, kMaxH, C, kGatv2MaxHC));
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_gatv2_supported(int H, int C)
{
  return H >= 1 && H <= wgamd::kMaxH && C >= 4 && C % 4 == 0 && (int64_t)H * C <= wgamd::kGatv2MaxHC;
}

extern "C" int64_t wgamd_gatv2_bwd_blocks(int64_t n_rows)
{
  return n_rows <= 0 ? 0 : (n_rows + wgamd::kGatv2BwdRows - 1) / wgamd::kGatv2BwdRows;
}

extern "C" wholememory_error_code_t wgamd_gatv2_attention_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* xl, int64_t ldxl, const float* xr, int64_t ldxr,
    const int64_t* xr_rows, const float* att, int H, int C, float negative_slope, const float* bias, int relu, int mean, float* out,
    int64_t ldo, float* alpha, float* agg, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gatv2_attention_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    gatv2_require_shape(H, C);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && xl && xr && att && out, "null pointer");
    const int HC = H * C, N = mean ? C : HC;
    WG_REQUIRE_INPUT(ldxl >= HC && ldxr >= HC && ldo >= N, "leading dimension too small");
    if (!aligned_rows(xl, ldxl) || !aligned_rows(xr, ldxr) || !aligned_rows(out, ldo) || !aligned_rows(att, 0) ||
        (bias && !aligned_rows(bias, 0)) || (agg && !aligned_rows(agg, 0)))
      throw logic_error("xl / xr / out / att / bias / agg rows must be 16-B aligned");
    gatv2_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.xl = xl, a.ldxl = ldxl, a.xr = xr, a.ldxr = ldxr, a.xr_rows = xr_rows;
    a.att = att, a.H = H, a.C = C, a.slope = negative_slope, a.bias = bias, a.relu = relu ? 1 : 0, a.mean = mean ? 1 : 0;
    a.out = out, a.ldo = ldo, a.alpha = alpha, a.agg = agg;
    const dim3 grid((unsigned)((n_rows + 3) / 4));
    with_head_lanes(C, [&](auto lph) {
      gatv2_attention_kernel<decltype(lph)::value><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gatv2_bwd_dst_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* xl, int64_t ldxl, const float* xr, int64_t ldxr,
    const int64_t* xr_rows, const float* att, int H, int C, float negative_slope, const float* alpha, const float* g, int64_t ldg,
    const float* agg, float* dxr, float* de, float* datt_part, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gatv2_bwd_dst_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    gatv2_require_shape(H, C);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && xl && xr && att && alpha && g && agg && dxr && de && datt_part, "null pointer");
    const int HC = H * C;
    WG_REQUIRE_INPUT(ldxl >= HC && ldxr >= HC && ldg >= HC, "leading dimension too small");
    if (!aligned_rows(xl, ldxl) || !aligned_rows(xr, ldxr) || !aligned_rows(g, ldg) || !aligned_rows(att, 0) ||
        !aligned_rows(agg, 0) || !aligned_rows(dxr, 0) || !aligned_rows(datt_part, 0))
      throw logic_error("xl / xr / g / att / agg / dxr / datt_part rows must be 16-B aligned");
    gatv2_bwd_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.xl = xl, a.ldxl = ldxl, a.xr = xr, a.ldxr = ldxr, a.xr_rows = xr_rows;
    a.att = att, a.H = H, a.C = C, a.slope = negative_slope, a.alpha = alpha, a.g = g, a.ldg = ldg, a.agg = agg;
    a.dxr = dxr, a.de = de, a.datt_part = datt_part;
    const dim3 grid((unsigned)wgamd_gatv2_bwd_blocks(n_rows));
    with_head_lanes(C, [&](auto lph) {
      gatv2_bwd_dst_kernel<decltype(lph)::value><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gatv2_bwd_src_f32(
    const int* row_ptr_t, const int* col_t, const int* perm, int64_t n_src, const float* xl, int64_t ldxl, const float* xr,
    int64_t ldxr, const int64_t* xr_rows, const float* att, int H, int C, float negative_slope, const float* alpha, const float* de,
    const float* g, int64_t ldg, float* gx, int64_t ldgx, int accumulate, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gatv2_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    gatv2_require_shape(H, C);
    if (n_src == 0) return;
    WG_REQUIRE_INPUT(row_ptr_t && col_t && perm && xl && xr && att && alpha && de && g && gx, "null pointer");
    const int HC = H * C;
    WG_REQUIRE_INPUT(ldxl >= HC && ldxr >= HC && ldg >= HC && ldgx >= HC, "leading dimension too small");
    if (!aligned_rows(xl, ldxl) || !aligned_rows(xr, ldxr) || !aligned_rows(g, ldg) || !aligned_rows(att, 0) || !aligned_rows(gx, ldgx))
      throw logic_error("xl / xr / g / att / gx rows must be 16-B aligned");
    gatv2_src_args a{};
    a.row_ptr_t = row_ptr_t, a.col_t = col_t, a.perm = perm, a.n_src = n_src, a.xl = xl, a.ldxl = ldxl, a.xr = xr, a.ldxr = ldxr;
    a.xr_rows = xr_rows, a.att = att, a.H = H, a.C = C, a.slope = negative_slope, a.alpha = alpha, a.de = de, a.g = g, a.ldg = ldg;
    a.gx = gx, a.ldgx = ldgx, a.accumulate = accumulate ? 1 : 0;
    gatv2_bwd_src_kernel<<<(unsigned)((n_src + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
