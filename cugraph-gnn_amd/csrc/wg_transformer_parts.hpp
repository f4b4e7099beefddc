// Shared pieces of the graph transformer layers (wg_transformer.hip, wg_transformer_hetero.hip): the shape limits, the wave sum,
// the head-bucket dispatch and THE row walk — the softmax-weighted blocks of one destination row of one relation.  Both layer
// kernels run this one function, so their blocks and alpha agree bit for bit.
#pragma once
#include "wg_layer_parts.hpp"

namespace wgamd {

constexpr int kMaxK = 1024;
constexpr int kMaxF = 256;     // one float4 of a source row per lane
constexpr int kMaxD = 32;      // [a | 1 | pad] within one wave's lanes
constexpr int kMaxH = 8;

// sum over the wave; xor butterflies give every lane the same bits (each step adds the same two values, commuted)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// floats of one head block [x | a | 1 | 0 pad]: every block starts 16-B aligned
__host__ __device__ inline int block_width(int F, int D) { return (F + D + 1 + 3) / 4 * 4; }

inline int heads_bucket(int H) { return H <= 1 ? 1 : H <= 2 ? 2 : H <= 4 ? 4 : 8; }

// launch(std::integral_constant<int, HM>{}) for the bucket HM of H heads
template <typename Launch>
void with_heads(int H, Launch&& launch)
{
  switch (heads_bucket(H)) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
}

// One relation's blocks of destination row i, by one wave: the edges [s, t) of the row -> blk[h W4 + :] for h < H, sources read
// at row_at(col[e]).  R is any struct with the relation's operands col, edge_attr ([E, D] in CSR order), u / ldu, w / ldw, alpha
// ([E, H] or null), F, D, H — tconv_layer_kernel's argument block, or a wgamd_hetero_transformer_relation_t; W4 = block_width(F,
// D).  row_at captures what it needs by value, not the argument block by reference (profiles/r10/README.md).  Lane = one float4 of the source row and, for lane <= D, one column of [a | 1]; groups of 4 edges; an online softmax
// (running max and sum per head, accumulators rescaled once per group, a group's terms summed before they join them); the logits
// go to alpha as they are made and become alpha in a second pass over the row.  A row without edges yields exact zeros and reads neither u nor w.
template <int HM, typename Rel, typename RowAt>
__device__ __forceinline__ void tconv_row_walk(const Rel& R, int W4, RowAt row_at, float* blk, int64_t i, int s, int t, int lane)
{
  const int F = R.F, H = R.H, D = R.D;
  const bool fx = lane < F / 4;
  const int ext_w = W4 - F;                       // [a | 1 | pad] columns of a head block
  f32x4 uh[HM], acc[HM];
  float wh[HM], ext[HM], m[HM], l[HM];
#pragma unroll
  for (int h = 0; h < HM; ++h) {
    uh[h] = acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    wh[h] = ext[h] = l[h] = 0.f;
    m[h] = -INFINITY;
    if (h < H && s < t) {
      if (fx) uh[h] = reinterpret_cast<const f32x4*>(R.u + i * R.ldu + (int64_t)h * F)[lane];
      if (lane < D) wh[h] = R.w[i * R.ldw + h * D + lane];
    }
  }
  for (int e0 = s; e0 < t; e0 += 4) {
    f32x4 xv[4];
    float av[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int e = e0 + v;
      xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      av[v] = 0.f;
      if (e < t) {
        const int j = R.col[e];
        if (fx) xv[v] = reinterpret_cast<const f32x4*>(row_at(j))[lane];
        av[v] = lane < D ? R.edge_attr[(int64_t)e * D + lane] : (lane == D ? 1.f : 0.f);
      }
    }
#pragma unroll
    for (int h = 0; h < HM; ++h) {
      if (h >= H) break;
      float sc[4];
      float mx = m[h];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        sc[v] = wave_sum(dot4(uh[h], xv[v]) + (lane < D ? wh[h] * av[v] : 0.f));
        if (e0 + v < t) mx = fmaxf(mx, sc[v]);
      }
      const float r = expf(m[h] - mx);            // (m = -inf before the first group: r = 0)
      acc[h] *= r;
      ext[h] *= r;
      l[h] *= r;
      // the group's four terms are summed on their own and enter the running sums as ONE term: a long row adds a quarter as
      // many small terms to a large sum (a 3000-edge row over 30 source rows: 1.2e-5 -> 1.4e-6 of the magnitude sum)
      f32x4 ga = {0.f, 0.f, 0.f, 0.f};
      float ge = 0.f, gl = 0.f;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (e0 + v < t) {
          const float p = expf(sc[v] - mx);
          ga += p * xv[v];
          ge += p * av[v];
          gl += p;
          if (R.alpha && lane == v) R.alpha[(int64_t)(e0 + v) * H + h] = sc[v];   // the logit; alpha after the row
        }
      }
      acc[h] += ga;
      ext[h] += ge;
      l[h] += gl;
      m[h] = mx;
    }
  }
#pragma unroll
  for (int h = 0; h < HM; ++h) {
    if (h >= H) break;
    const float inv = l[h] > 0.f ? 1.f / l[h] : 0.f;          // (no edges: acc = ext = 0 and inv = 0 — the block is exactly zero)
    if (fx) reinterpret_cast<f32x4*>(blk + h * W4)[lane] = acc[h] * inv;
    if (lane < ext_w) blk[h * W4 + F + lane] = ext[h] * inv;
    l[h] = inv;
  }
  if (R.alpha && s < t) {
    __threadfence_block();                        // the logits this wave wrote, read back by other lanes
    for (int e = s + lane; e < t; e += 64)
#pragma unroll
      for (int h = 0; h < HM; ++h) {
        if (h >= H) break;
        float* p = R.alpha + (int64_t)e * H + h;
        *p = expf(*p - m[h]) * l[h];
      }
  }
}

}  // namespace wgamd
