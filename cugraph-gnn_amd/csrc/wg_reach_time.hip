// Reach times of a node type's vertex list in the TEMPORAL heterogeneous call-group walk (include/wgamd_ext.h:
// wgamd_reach_time_append; wholegraph_amd/fused.py: HeteroPygWalk).  Several edge-type calls of one hop can append to the same
// source type's list, and each call rebuilds that list batch-major, so the walk keeps a time list parallel to every type's
// `nodes` and carries it across each call: nodes_out lays a batch out as its old list followed by the vertices this call saw
// first, in first-appearance order (the emit kernels of wg_append_unique.hip: old entries at t0 + i + shift, new ones from
// tail_row + rank on, frontier_out[rank] the same vertex) — so the old times move with their batch and the call's
// frontier_time_out fills the rest.  A vertex that is already listed keeps its time whichever edge type reaches it again.
#include "wg_common.hpp"
#include "wgamd_ext.h"

namespace wgamd {
namespace {

__global__ void __launch_bounds__(256)
reach_time_append_kernel(const int64_t* __restrict__ time_in, int64_t time_in_cap, const int* __restrict__ node_seg,
                         const int64_t* __restrict__ f_time_out, int64_t f_cap, const int* __restrict__ f_out_seg,
                         const int* __restrict__ out_batch, const int* __restrict__ out_seg, int G, int64_t cap,
                         int64_t* __restrict__ time_out)
{
  const int64_t live = min((int64_t)out_seg[G], cap);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < live; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = out_batch[i];
    if ((unsigned)b >= (unsigned)G) continue;
    const int64_t l = i - out_seg[b];
    const int n0 = node_seg[b], n_old = node_seg[b + 1] - n0;
    if (l < 0) continue;
    if (l < n_old) {
      const int64_t src = (int64_t)n0 + l;
      if ((uint64_t)src < (uint64_t)time_in_cap) time_out[i] = time_in[src];
    } else {
      const int64_t src = (int64_t)f_out_seg[b] + (l - n_old);
      if ((uint64_t)src < (uint64_t)f_cap) time_out[i] = f_time_out[src];
    }
  }
}

}  // namespace
}  // namespace wgamd

extern "C" {

wholememory_error_code_t wgamd_reach_time_append(const int64_t* time_in, int64_t time_in_cap, const int* node_seg,
                                                 const int64_t* frontier_time_out, int64_t frontier_cap,
                                                 const int* frontier_out_seg, const int* nodes_out_batch,
                                                 const int* nodes_out_seg, int n_batches, int64_t capacity, int64_t* time_out,
                                                 void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_reach_time_append", [&] {
    WG_REQUIRE_INPUT(n_batches >= 1 && n_batches < (1 << 20), "bad batch count");
    WG_REQUIRE_INPUT(capacity >= 1 && capacity < ((int64_t)1 << 30) && time_in_cap >= 0 && frontier_cap >= 0, "bad capacities");
    WG_REQUIRE_INPUT((time_in || time_in_cap == 0) && node_seg && frontier_time_out && frontier_out_seg && nodes_out_batch &&
                       nodes_out_seg && time_out,
                     "null pointer");
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(capacity, (int64_t)256), 256 * 8));
    reach_time_append_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(
      time_in, time_in_cap, node_seg, frontier_time_out, frontier_cap, frontier_out_seg, nodes_out_batch, nodes_out_seg,
      n_batches, capacity, time_out);
    WG_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
