// GATv2 attention WITH EDGE FEATURES (torch_geometric.nn.GATv2Conv(edge_dim=D)) over a sampled hop, on transformed rows:
//     s_ij    = XL[j] + XR[i] + W_e ea[e]                       (ea [E, D]: the edge's attributes, one row per CSR slot)
//     e_ijh   = sum_c att[h, c] LeakyReLU(s_ij[h, c])
//     alpha   = softmax_j(e_ijh),   agg_ih = sum_j alpha_ijh XL[j, h, :]           (the message carries no edge term)
// lin_edge(ea) is an [E, H C] tensor — 1 KiB per edge at H C = 256 — that these kernels never write: the edge row is D <= 16
// floats, and the lane that holds its float4 of XL[j] + XR[i] forms its four columns of W_e ea[e] in registers.
//
// The walk is wg_gatv2.hip's (one wave per row, lane = one float4 of the H C <= 256 wide row, edges in groups of four, head_sum and
// the online softmax; wg_gatv2_parts.hpp).  What is new in all three kernels:
//   * W_e^T [D, H C] sits in LDS (<= 16 KB, rows of 64 float4 with zeros behind the row), copied by the workgroup before ONE
//     barrier that comes ahead of every wave-uniform return.
//   * An edge's D attributes are wave-uniform.  A group's four edges are loaded by 4 D <= 64 lanes in one read (lane v D + d =
//     ea[e_v, d]: contiguous in the destination-major kernels, through perm in the source-major one) and each value is broadcast
//     with v_readlane, so it enters the multiply as a scalar operand.
//   * For each d ONE 16-byte LDS read of W_e^T[d] feeds the four edges in flight: z[v] += ea[e_v, d] w4.
// Matrix instructions do not fit: a row has about 11 entries, K = D <= 16, and the product is needed in the lane = column layout
// the softmax walk keeps, not in an MFMA accumulator layout.
//   * gatv2_edge_bwd_dst_kernel also makes dW_e^T[d, hc] = sum_e ea[e, d] de[e, h] att[hc] LeakyReLU'(s[hc]) in registers (4
//     columns x DP per lane, DP = D rounded up to a multiple of 4, the padding read as zeros).  Its grid is bounded (min(tiles,
//     4 x CUs) workgroups, each walking the tiles b, b + grid, ... at a FIXED stride), so the [D, H C] partial per workgroup
//     stays small and the order of every sum is the same from run to run; the four waves' sums are added in wave order through LDS.
// No atomics anywhere: the same bits from run to run.
#include "wg_gatv2_parts.hpp"

namespace wgamd {
namespace {

constexpr int kGatv2MaxD     = 16;    // 4 edges x D attributes within one wave's lanes; W_e^T within 16 KB of LDS
constexpr int kGatv2EdgeWgCu = 4;     // workgroups per CU of the destination-major backward

struct gatv2_edge_args : gatv2_args {
  const float* ea;            // [E, D] in CSR slot order
  const float* wet;           // W_e^T [D, H C]
  int D;
};

struct gatv2_edge_bwd_args : gatv2_bwd_args {
  const float* ea;
  const float* wet;
  int D;
  float* dwe_part;            // [n_blocks, D, H C]
  int n_tiles;
};

struct gatv2_edge_src_args : gatv2_src_args {
  const float* ea;            // read at perm
  const float* wet;
  int D;
};

using edge_weight_lds = f32x4[kGatv2MaxD][64];

// the workgroup's copy of W_e^T, zeros behind the row (an idle lane's edge term is zero); ends in the kernel's one barrier
__device__ __forceinline__ void load_edge_weight(edge_weight_lds& w, const float* wet, int D, int HC)
{
  const int q = HC / 4;
  for (int idx = threadIdx.x; idx < D * 64; idx += 256) {
    const int d = idx >> 6, l = idx & 63;
    w[d][l] = l < q ? reinterpret_cast<const f32x4*>(wet + (int64_t)d * HC)[l] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
}

// lane `at` of the group's attribute register, as a scalar (at is wave-uniform)
__device__ __forceinline__ float edge_value(float eav, int at)
{
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(eav), at));
}

// z[v] += W_e ea[e_v] for the four edges of a group: one LDS read per attribute
__device__ __forceinline__ void add_edge_term(f32x4 (&z)[4], float eav, const edge_weight_lds& w, int D, int lane)
{
  for (int d = 0; d < D; ++d) {
    const f32x4 w4 = w[d][lane];
#pragma unroll
    for (int v = 0; v < 4; ++v) z[v] += edge_value(eav, v * D + d) * w4;
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <int LPH>
__global__ void __launch_bounds__(256) gatv2_edge_attention_kernel(gatv2_edge_args a)
{
  __shared__ edge_weight_lds w;
  const int lane = threadIdx.x & 63;
  const int H = a.H, lph = a.C / 4, HC = H * a.C, D = a.D;
  load_edge_weight(w, a.wet, D, HC);
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_rows) return;                      // (wave-uniform, behind the barrier)
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
    f32x4 xv[4], z[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e0 + v < t && on) xv[v] = reinterpret_cast<const f32x4*>(a.xl + (int64_t)a.col[e0 + v] * a.ldxl)[lane];
      z[v] = xv[v] + xr4;
    }
    const float eav = lane < min(4, t - e0) * D ? a.ea[(int64_t)e0 * D + lane] : 0.f;     // the group's rows are contiguous
    add_edge_term(z, eav, w, D, lane);
    float sc[4];
    float mx = m;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
      for (int k = 0; k < 4; ++k) z[v][k] = z[v][k] > 0.f ? z[v][k] : a.slope * z[v][k];
      sc[v] = head_sum<LPH>(dot4(att4, z[v]), hd, H);
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
  gatv2_row_finish(a, i, lane, on, H, lph, HC, s, t, acc, l, m);
}

// ---- destination-major backward -----------------------------------------------------------------------------------------------
template <int LPH, int DP>
__global__ void __launch_bounds__(256) gatv2_edge_bwd_dst_kernel(gatv2_edge_bwd_args a)
{
  __shared__ edge_weight_lds w;
  __shared__ f32x4 part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = a.H, lph = a.C / 4, HC = H * a.C, D = a.D;
  load_edge_weight(w, a.wet, D, HC);
  const bool on = lane < H * lph;
  const int hd = on ? lane / lph : H;
  const bool lead = on && lane == hd * lph;
  f32x4 att4 = {0.f, 0.f, 0.f, 0.f}, da = att4, dw[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) dw[d] = att4;
  if (on) att4 = reinterpret_cast<const f32x4*>(a.att)[lane];
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {          // (a fixed stride: the same sums every run)
    const int64_t row0 = (int64_t)tile * kGatv2BwdRows;
    for (int r = wave; r < kGatv2BwdRows; r += 4) {
      const int64_t i = row0 + r;
      if (i >= a.n_rows) break;                   // (wave-uniform)
      const int s = a.row_ptr[i], t = a.row_ptr[i + 1];
      f32x4 g4 = {0.f, 0.f, 0.f, 0.f}, xr4 = g4, ag = g4, dx = g4;
      if (on) {
        g4 = reinterpret_cast<const f32x4*>(a.g + i * a.ldg)[lane];
        ag = reinterpret_cast<const f32x4*>(a.agg + i * HC)[lane];
        if (s < t) xr4 = reinterpret_cast<const f32x4*>(a.xr + (a.xr_rows ? a.xr_rows[i] : i) * a.ldxr)[lane];
      }
      const float rdot = head_sum<LPH>(dot4(g4, ag), hd, H);      // sum_j alpha dalpha = G_ih . agg_ih
      for (int e0 = s; e0 < t; e0 += 4) {
        f32x4 xv[4], z[4];
        float al[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
          al[v] = 0.f;
          if (e0 + v < t && on) {
            xv[v] = reinterpret_cast<const f32x4*>(a.xl + (int64_t)a.col[e0 + v] * a.ldxl)[lane];
            al[v] = a.alpha[(int64_t)(e0 + v) * H + hd];
          }
          z[v] = xv[v] + xr4;
        }
        const float eav = lane < min(4, t - e0) * D ? a.ea[(int64_t)e0 * D + lane] : 0.f;
        add_edge_term(z, eav, w, D, lane);
        f32x4 ds[4];                              // dL/d s_ij: what dXR, dXL and dW_e all take (zeros behind the row's end)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float dal = head_sum<LPH>(dot4(g4, xv[v]), hd, H);
          ds[v] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (e0 + v < t) {
            const float dev = al[v] * (dal - rdot);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const bool pos = z[v][k] > 0.f;
              ds[v][k] = dev * att4[k] * (pos ? 1.f : a.slope);
              dx[k] += ds[v][k];
              da[k] += dev * (pos ? z[v][k] : a.slope * z[v][k]);
            }
            if (lead) a.de[(int64_t)(e0 + v) * H + hd] = dev;
          }
        }
        // (a uniform branch per attribute: the padding costs nothing, and each value is broadcast where it is used — sixty-four
        //  scalars of a group would not fit the scalar registers at once)
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          if (d < D) {
#pragma unroll
            for (int v = 0; v < 4; ++v) dw[d] += edge_value(eav, v * D + d) * ds[v];
          }
        }
      }
      if (on) reinterpret_cast<f32x4*>(a.dxr + i * HC)[lane] = dx;
    }
  }
  part[wave][lane] = da;
  __syncthreads();
  if (wave == 0 && on)
    reinterpret_cast<f32x4*>(a.datt_part + (int64_t)blockIdx.x * HC)[lane] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
#pragma unroll
  for (int d = 0; d < DP; ++d) {                  // (uniform barriers: DP is the kernel's, every thread arrives)
    __syncthreads();
    part[wave][lane] = dw[d];
    __syncthreads();
    if (wave == 0 && on && d < D)
      reinterpret_cast<f32x4*>(a.dwe_part + ((int64_t)blockIdx.x * D + d) * HC)[lane] =
          ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
  }
}

// ---- source-major backward: the transformed source rows' gradient -------------------------------------------------------------
__global__ void __launch_bounds__(256) gatv2_edge_bwd_src_kernel(gatv2_edge_src_args a)
{
  __shared__ edge_weight_lds w;
  const int lane = threadIdx.x & 63;
  const int lph = a.C / 4, H = a.H, D = a.D;
  load_edge_weight(w, a.wet, D, H * a.C);
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= a.n_src) return;                       // (wave-uniform; idle lanes stay: they hold attributes of the group)
  const bool on = lane < H * lph;
  const int hd = on ? lane / lph : 0;
  const int gv = lane / D, gd = lane - gv * D;    // this lane's edge of the group and attribute
  const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (s < t) {
    f32x4 att4 = acc, xl4 = acc;
    if (on) {
      att4 = reinterpret_cast<const f32x4*>(a.att)[lane];
      xl4  = reinterpret_cast<const f32x4*>(a.xl + j * a.ldxl)[lane];
    }
    for (int p0 = s; p0 < t; p0 += 4) {
      f32x4 gv4[4], z[4];
      float al[4], dv[4];
      int64_t mine = -1;                          // the CSR edge this lane reads an attribute of
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        gv4[v] = z[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        al[v] = dv[v] = 0.f;
        if (p0 + v < t) {
          const int64_t i = a.col_t[p0 + v], e = a.perm[p0 + v];
          if (gv == v) mine = e;
          if (on) {
            gv4[v] = reinterpret_cast<const f32x4*>(a.g + i * a.ldg)[lane];
            z[v]   = xl4 + reinterpret_cast<const f32x4*>(a.xr + (a.xr_rows ? a.xr_rows[i] : i) * a.ldxr)[lane];
            al[v]  = a.alpha[e * H + hd];
            dv[v]  = a.de[e * H + hd];
          }
        }
      }
      const float eav = mine >= 0 ? a.ea[mine * D + gd] : 0.f;
      add_edge_term(z, eav, w, D, lane);
#pragma unroll
      for (int v = 0; v < 4; ++v) {               // (entries join in transposed-CSR order)
        if (p0 + v < t) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += al[v] * gv4[v][k] + dv[v] * att4[k] * (z[v][k] > 0.f ? 1.f : a.slope);
        }
      }
    }
  }
  if (on) {
    f32x4* o = reinterpret_cast<f32x4*>(a.gx + j * a.ldgx) + lane;
    *o = a.accumulate ? *o + acc : acc;
  }
}

void gatv2_edge_require_shape(int H, int C, int D)
{
  gatv2_require_shape(H, C);
  if (D < 1 || D > kGatv2MaxD) throw logic_error(fmt("unsupported edge_dim: D=%d (1 .. %d)", D, kGatv2MaxD));
}

// launch(std::integral_constant<int, DP>{}) for D attributes, DP = D rounded up to a multiple of 4
template <typename Launch>
void with_edge_dim(int D, Launch&& launch)
{
  switch ((D + 3) / 4) {
    case 1: launch(std::integral_constant<int, 4>{}); break;
    case 2: launch(std::integral_constant<int, 8>{}); break;
    case 3: launch(std::integral_constant<int, 12>{}); break;
    default: launch(std::integral_constant<int, 16>{}); break;
  }
}

int64_t gatv2_edge_tiles(int64_t n_rows) { return n_rows <= 0 ? 0 : (n_rows + kGatv2BwdRows - 1) / kGatv2BwdRows; }

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_gatv2_edge_supported(int H, int C, int D)
{
  return wgamd_gatv2_supported(H, C) && D >= 1 && D <= wgamd::kGatv2MaxD;
}

extern "C" int64_t wgamd_gatv2_edge_bwd_blocks(int64_t n_rows, int max_blocks)
{
  const int64_t cap = max_blocks > 0 ? max_blocks : (int64_t)wgamd::kGatv2EdgeWgCu * wgamd::stream_cu_count(nullptr);
  return std::min<int64_t>(wgamd::gatv2_edge_tiles(n_rows), cap);
}

extern "C" wholememory_error_code_t wgamd_gatv2_edge_attention_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* xl, int64_t ldxl, const float* xr, int64_t ldxr,
    const int64_t* xr_rows, const float* att, int H, int C, float negative_slope, const float* edge_attr, const float* w_edge_t, int D,
    const float* bias, int relu, int mean, float* out, int64_t ldo, float* alpha, float* agg, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gatv2_edge_attention_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    gatv2_edge_require_shape(H, C, D);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(row_ptr && col && xl && xr && att && out && edge_attr && w_edge_t, "null pointer");
    const int HC = H * C, N = mean ? C : HC;
    WG_REQUIRE_INPUT(ldxl >= HC && ldxr >= HC && ldo >= N, "leading dimension too small");
    if (!aligned_rows(xl, ldxl) || !aligned_rows(xr, ldxr) || !aligned_rows(out, ldo) || !aligned_rows(att, 0) ||
        !aligned_rows(w_edge_t, 0) || (bias && !aligned_rows(bias, 0)) || (agg && !aligned_rows(agg, 0)))
      throw logic_error("xl / xr / out / att / w_edge_t / bias / agg rows must be 16-B aligned");
    gatv2_edge_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.xl = xl, a.ldxl = ldxl, a.xr = xr, a.ldxr = ldxr, a.xr_rows = xr_rows;
    a.att = att, a.H = H, a.C = C, a.slope = negative_slope, a.bias = bias, a.relu = relu ? 1 : 0, a.mean = mean ? 1 : 0;
    a.out = out, a.ldo = ldo, a.alpha = alpha, a.agg = agg, a.ea = edge_attr, a.wet = w_edge_t, a.D = D;
    const dim3 grid((unsigned)((n_rows + 3) / 4));
    with_head_lanes(C, [&](auto lph) {
      gatv2_edge_attention_kernel<decltype(lph)::value><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gatv2_edge_bwd_dst_f32(
    const int* row_ptr, const int* col, int64_t n_rows, const float* xl, int64_t ldxl, const float* xr, int64_t ldxr,
    const int64_t* xr_rows, const float* att, int H, int C, float negative_slope, const float* edge_attr, const float* w_edge_t, int D,
    const float* alpha, const float* g, int64_t ldg, const float* agg, float* dxr, float* de, float* datt_part, float* dwe_part,
    int64_t n_blocks, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gatv2_edge_bwd_dst_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    gatv2_edge_require_shape(H, C, D);
    if (n_rows == 0) return;
    const int64_t tiles = gatv2_edge_tiles(n_rows);
    WG_REQUIRE_INPUT(n_blocks >= 1 && n_blocks <= tiles && tiles <= INT32_MAX, "n_blocks: 1 .. the hop's tiles of 16 rows");
    WG_REQUIRE_INPUT(row_ptr && col && xl && xr && att && alpha && g && agg && dxr && de && datt_part && dwe_part && edge_attr && w_edge_t,
                     "null pointer");
    const int HC = H * C;
    WG_REQUIRE_INPUT(ldxl >= HC && ldxr >= HC && ldg >= HC, "leading dimension too small");
    if (!aligned_rows(xl, ldxl) || !aligned_rows(xr, ldxr) || !aligned_rows(g, ldg) || !aligned_rows(att, 0) || !aligned_rows(w_edge_t, 0) ||
        !aligned_rows(agg, 0) || !aligned_rows(dxr, 0) || !aligned_rows(datt_part, 0) || !aligned_rows(dwe_part, 0))
      throw logic_error("xl / xr / g / att / w_edge_t / agg / dxr / datt_part / dwe_part rows must be 16-B aligned");
    gatv2_edge_bwd_args a{};
    a.row_ptr = row_ptr, a.col = col, a.n_rows = n_rows, a.xl = xl, a.ldxl = ldxl, a.xr = xr, a.ldxr = ldxr, a.xr_rows = xr_rows;
    a.att = att, a.H = H, a.C = C, a.slope = negative_slope, a.alpha = alpha, a.g = g, a.ldg = ldg, a.agg = agg;
    a.dxr = dxr, a.de = de, a.datt_part = datt_part, a.ea = edge_attr, a.wet = w_edge_t, a.D = D, a.dwe_part = dwe_part;
    a.n_tiles = (int)tiles;
    const dim3 grid((unsigned)n_blocks);
    with_head_lanes(C, [&](auto lph) {
      with_edge_dim(D, [&](auto dp) {
        gatv2_edge_bwd_dst_kernel<decltype(lph)::value, decltype(dp)::value><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
      });
    });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_gatv2_edge_bwd_src_f32(
    const int* row_ptr_t, const int* col_t, const int* perm, int64_t n_src, const float* xl, int64_t ldxl, const float* xr,
    int64_t ldxr, const int64_t* xr_rows, const float* att, int H, int C, float negative_slope, const float* edge_attr,
    const float* w_edge_t, int D, const float* alpha, const float* de, const float* g, int64_t ldg, float* gx, int64_t ldgx,
    int accumulate, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_gatv2_edge_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    gatv2_edge_require_shape(H, C, D);
    if (n_src == 0) return;
    WG_REQUIRE_INPUT(row_ptr_t && col_t && perm && xl && xr && att && alpha && de && g && gx && edge_attr && w_edge_t, "null pointer");
    const int HC = H * C;
    WG_REQUIRE_INPUT(ldxl >= HC && ldxr >= HC && ldg >= HC && ldgx >= HC, "leading dimension too small");
    if (!aligned_rows(xl, ldxl) || !aligned_rows(xr, ldxr) || !aligned_rows(g, ldg) || !aligned_rows(att, 0) ||
        !aligned_rows(w_edge_t, 0) || !aligned_rows(gx, ldgx))
      throw logic_error("xl / xr / g / att / w_edge_t / gx rows must be 16-B aligned");
    gatv2_edge_src_args a{};
    a.row_ptr_t = row_ptr_t, a.col_t = col_t, a.perm = perm, a.n_src = n_src, a.xl = xl, a.ldxl = ldxl, a.xr = xr, a.ldxr = ldxr;
    a.xr_rows = xr_rows, a.att = att, a.H = H, a.C = C, a.slope = negative_slope, a.alpha = alpha, a.de = de, a.g = g, a.ldg = ldg;
    a.gx = gx, a.ldgx = ldgx, a.accumulate = accumulate ? 1 : 0, a.ea = edge_attr, a.wet = w_edge_t, a.D = D;
    gatv2_edge_bwd_src_kernel<<<(unsigned)((n_src + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
