// What the two link-prediction heads (wg_link.hip: inner product; wg_link_mlp.hip: MLP edge decoder) share: the binary
// cross-entropy of one score with the coefficient the backward multiplies with, and the fixed-order sum of the per-workgroup
// loss partials by the last workgroup to finish (the ticket of wg_xent.hip).
#pragma once
#include "wg_common.hpp"

namespace wgamd {

constexpr int kLinkThreads = 256;
constexpr int kLinkMaxGrid = 2048;   // the grid of a BCE forward is bounded: one state serves every call

__device__ __forceinline__ float link_wave_sum(float v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// One pair's part of the loss: loss += w (max(s, 0) - s y + log1p(exp(-|s|))), wsum += w; returns c = w (sigmoid(s) - y), 0 for
// a pair that read nothing (good = false: s is NaN then, and so is the loss)
__device__ __forceinline__ float bce_pair(float s, bool good, float y, float w, float& loss, float& wsum)
{
  const float e = expf(-fabsf(s));
  loss += w * (fmaxf(s, 0.f) - s * y + log1pf(e));
  wsum += w;
  // sigmoid(s) - y without the cancellation of sigmoid - 1
  const float num = s >= 0.f ? (1.f - y) - y * e : (1.f - y) * e - y;
  return good ? w * num / (1.f + e) : 0.f;
}

// state: [0] loss, [1] sum of weights, [2] the ticket (as int; at a fixed place: the state serves launches of any grid),
// [3] unused, then per workgroup (loss, weight) pairs.  Every thread of every workgroup calls this once, with its own sums.
__device__ __forceinline__ void bce_finish(float loss, float wsum, float* __restrict__ state, float* __restrict__ coef, int64_t P,
                                           float* __restrict__ loss_out, int mean)
{
  constexpr int waves = kLinkThreads / 64;
  __shared__ float s_loss[waves], s_w[waves];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  loss = link_wave_sum(loss);
  wsum = link_wave_sum(wsum);
  if (lane == 0) {
    s_loss[wave] = loss;
    s_w[wave]    = wsum;
  }
  __syncthreads();
  float* part = state + 4;
  int* ticket = reinterpret_cast<int*>(state + 2);
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < waves; k++) a += s_loss[k], b += s_w[k];
    part[2 * blockIdx.x]     = a;
    part[2 * blockIdx.x + 1] = b;
    __threadfence();
    s_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (s_last) {   // thread k takes workgroups k, k + 256, ... in order, then a fixed tree
    __shared__ float t_loss[kLinkThreads], t_w[kLinkThreads];
    __threadfence();
    float a = 0.f, b = 0.f;
    for (unsigned k = threadIdx.x; k < gridDim.x; k += kLinkThreads) {
      a += __hip_atomic_load(&part[2 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      b += __hip_atomic_load(&part[2 * k + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    t_loss[threadIdx.x] = a;
    t_w[threadIdx.x]    = b;
    __syncthreads();
    for (int half = kLinkThreads / 2; half >= 1; half >>= 1) {
      if ((int)threadIdx.x < half) {
        t_loss[threadIdx.x] += t_loss[threadIdx.x + half];
        t_w[threadIdx.x] += t_w[threadIdx.x + half];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float l = mean ? t_loss[0] / t_w[0] : t_loss[0];
      state[0]  = l;
      state[1]  = t_w[0];
      coef[P]   = t_w[0];   // the sum of weights travels with the coefficients: the state is free for the next call
      *loss_out = l;
      *ticket   = 0;        // (the state is reusable without a memset)
    }
  }
}

}  // namespace wgamd
