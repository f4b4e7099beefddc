// De-duplication of an id list whose ids are known to lie below a bound (the vertex count of the table they index):
//     distinct = the distinct non-negative ids, ASCENDING;   inverse[i] = position of ids[i] in `distinct` (-1 for ids[i] < 0).
//
// Why it exists: a call group of G mini-batches fetches the features of every (batch, vertex) pair — 10.9 M rows for 191
// products batches — but the graph only HAS 2.45 M vertices, so at most 2.45 M distinct rows are behind them.  On one GPU the
// repeats are served by L2 / Infinity Cache and cost little; over xGMI every repeat is wire traffic (7 links x ~64 GB/s per
// direction per GPU).  The partitioned FeatureStore therefore fetches the DISTINCT rows through the all-to-all and expands
// them locally (wholegraph_amd/tensor.py: DistributedWholeMemoryTensor.gather(dedup=...)): 4.4x fewer bytes on the wire for
// the products call group.  The reference's NCCL gather (wholememory_gather_nccl, gather_op_impl_nccl.cu:23-171) exchanges
// every requested id; its embedding cache path de-duplicates for a different purpose (embedding_cache_func.cuh).
//
// Because the ids are bounded the job needs no sort and no hash table: mark -> one word of bits per 32 ids -> scan over
// bound / 32 counts -> compact -> look up.  The compacted list comes out ascending, i.e. already grouped by owner rank of a
// range-partitioned table.
//
// Two ways to the bit words, chosen from the shape alone (no switch):
//   marks in LDS   R = ceil(bound / 2^20) <= 8, for every n.  Workgroup (range, slice) ORs the bits of its range into 128 KB of
//                  LDS while it streams its slice of the list, writes them once to the slice's slab; the slabs are OR-ed word by
//                  word, then scan and compaction are one launch.  Four launches, no memset, no copy; the list is read R times.
//   byte marks     every larger bound (papers100M: R = 106, RMAT-26: R = 64).  One byte per possible id in global memory, test
//                  before set, packed afterwards; the list is read once, every first mark is a fabric write.  Ten launches.
// The rule is fitted to a measured grid (profiles/r08/README.md: n = 1e5, 1e6, 1e7 x bound = 2^20 ... 111 M x both id types, us per
// call): the LDS path is faster at every n and for both id types up to R = 8 (10 M int64 ids: 84 against 139 us at R = 1, 155
// against 349 at R = 8) and slower at every point from R = 64 on; between them it depends on n and on the id type (int32 lists
// lose from R = 12 at n = 1e5 and from R = 24 at every n), and the byte path is kept there.  The rule looks at
// the bound only: `n` is the list's CAPACITY — the live count of a no-sync walk's list is on the device — and a short list
// costs the LDS path little, because the slices (at least 8192 ids each) are sized from it: 100 k ids wake 13 x R workgroups.
#include "wg_common.hpp"
#include "wgamd_ext.h"

namespace wgamd {
namespace {

// ---- byte marks (round 6; bounds above 2^23) ---------------------------------------------------------------------------------------
// The marks are one BYTE per possible id (2.4 MB for products: resident in every XCD's 4 MB L2, where the int flags'
// 10 MB were not), packed afterwards into one bit per id + a count per 32 ids; positions are prefix[id >> 5] + popc(bits below),
// kept side by side as {bits, prefix} so the look-up pass makes ONE scattered 8-byte load into 0.6 MB instead of two into 20 MB.
// For the 10.7 M listed rows of a products call group: mark 195 -> 134 us, look-up 114 -> 53 us (profiles/r06/README.md).  What is
// left of the mark is its stores (57 us without them, measured): every scattered byte store is one fabric write, and a mark set
// by one XCD is not seen by the other seven before the kernel ends, so an id listed by k batches is stored up to min(k, 8) times.
template <typename IdT>
__global__ void __launch_bounds__(256) unique_mark_kernel(const IdT* __restrict__ ids, int64_t n, int64_t bound, uint8_t* __restrict__ flags,
                                                          int* __restrict__ bad, const int* __restrict__ n_live)
{
  if (n_live) n = min(n, (int64_t)*n_live);   // (capacity-sized list of a no-sync walk: the live count is on the device)
  // four independent id loads, then four independent mark loads per trip
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 4 * T) {
    int64_t id[4];
    uint8_t f[4];
#pragma unroll
    for (int k = 0; k < 4; k++) id[k] = i + k * T < n ? (int64_t)ids[i + k * T] : -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (id[k] >= bound) {
        *bad  = 1;   // (every such lane writes the same value)
        id[k] = -1;
      }
      f[k] = id[k] >= 0 ? flags[id[k]] : 1;
    }
    // plain stores of one value: no atomics needed.  Test first: a call group names a hub thousands of times, and thousands of
    // stores to one address queue up in its L2 channel; the read of a byte that is already set is a broadcast hit
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (f[k] == 0) flags[id[k]] = 1;
  }
}

// 32 marks -> one word of bits + its population count (flags is padded with zeros to a multiple of 32)
__global__ void __launch_bounds__(256) unique_pack_kernel(const uint8_t* __restrict__ flags, int64_t n_words, uint2* __restrict__ rank,
                                                          int* __restrict__ cnt, int64_t cnt_padded)
{
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n_words) {
    const uint4* p = reinterpret_cast<const uint4*>(flags + w * 32);
    const uint4 a = p[0], b = p[1];
    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {   // bytes are 0 or 1: bit 0 of every byte, gathered
      const uint32_t x = v[k];
      word |= ((x & 1u) | ((x >> 7) & 2u) | ((x >> 14) & 4u) | ((x >> 21) & 8u)) << (4 * k);
    }
    rank[w].x = word;
    cnt[w]    = __popc(word);
  } else if (w < cnt_padded) {
    cnt[w] = 0;   // the scan reads whole tiles
  }
}

__global__ void __launch_bounds__(256) unique_compact_kernel(uint2* __restrict__ rank, const int* __restrict__ prefix, int64_t n_words,
                                                             int64_t* __restrict__ distinct, int* __restrict__ n_distinct)
{
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w == 0 && n_distinct) *n_distinct = prefix[n_words];
  if (w >= n_words) return;
  uint32_t word = rank[w].x;
  int at        = prefix[w];
  rank[w].y     = (uint32_t)at;   // {bits, ids set below this word} side by side: ONE scattered 8-byte load per look-up
  while (word) {
    const int k    = __ffs(word) - 1;
    distinct[at++] = w * 32 + k;
    word &= word - 1;
  }
}

template <typename IdT>
__global__ void __launch_bounds__(256) unique_inverse_kernel(const IdT* __restrict__ ids, int64_t n, int64_t bound, const uint2* __restrict__ rank,
                                                             int* __restrict__ inverse,
                                                             const int* __restrict__ n_live)
{
  if (n_live) n = min(n, (int64_t)*n_live);
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 4 * T) {
    int64_t id[4];
    uint2 r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) id[k] = i + k * T < n ? (int64_t)ids[i + k * T] : -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool ok = id[k] >= 0 && id[k] < bound;
      r[k]          = ok ? rank[id[k] >> 5] : make_uint2(0u, 0xffffffffu);
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (i + k * T < n) inverse[i + k * T] = (int)r[k].y + __popc(r[k].x & ((1u << (id[k] & 31)) - 1u));
  }
}


// ---- marks in LDS (round 8) ---------------------------------------------------------------------------------------------------
// A mark is one bit, and a range of 2^20 ids is 128 KB of bits: it fits one workgroup's LDS.  Workgroup (range r, slice s)
// streams slice s of the list and sets the bit of every id of range r in LDS — no store leaves the CU while the list is
// read — then writes its bit words once, to slab s.  The list is read R = ceil(bound / 2^20) times and the slabs make one
// round trip (<= 256 x 128 KB), against one fabric write per listed id on the byte path.
constexpr int kRangeBits   = 20;
constexpr int kRangeWords  = 1 << (kRangeBits - 5);   // 32768 words of 32 bits = 128 KB
constexpr int kMarkThreads = 1024;                    // one workgroup per CU (its LDS): 16 waves keep the list loads in flight
constexpr int kMarkLoads   = 8;                       // independent id loads per lane and trip
constexpr int kMarkBlocks  = 256;                     // workgroups of a launch (ranges x slices): one round on an MI355X
constexpr int kMinSlice    = kMarkThreads * kMarkLoads;
constexpr int kSumTile     = 64;                      // words per count: the reduce kernel sums one wave's words

// block -> (slice, range).  xcd_group: blocks b and b + 8 share an XCD (observed dispatch order), so the R workgroups that
// read one slice are given consecutive slots of ONE XCD and all but the first of their reads can hit its L2; slices are
// dealt over the eight labels, S is at most 8 floor(32 / R) so that no XCD gets more workgroups than it has CUs.
template <typename IdT>
__global__ void __launch_bounds__(kMarkThreads) unique_lds_mark_kernel(const IdT* __restrict__ ids, int64_t n, int64_t bound, int R, int S,
                                                                        int xcd_group, int64_t row_words, uint32_t* __restrict__ slabs,
                                                                        int* __restrict__ bad_flags, const int* __restrict__ n_live)
{
  extern __shared__ uint32_t s_bits[];
  __shared__ int s_bad;
  int slice, r;
  if (xcd_group) {
    const int k = blockIdx.x >> 3;
    slice       = (k / R) * 8 + (blockIdx.x & 7);
    r           = k % R;
  } else {
    slice = blockIdx.x / R;
    r     = blockIdx.x % R;
  }
  if (slice >= S) return;
  const int wr = (int)min((int64_t)kRangeWords, row_words - (int64_t)r * kRangeWords);   // a multiple of kSumTile
  uint4* s4    = reinterpret_cast<uint4*>(s_bits);
  for (int j = threadIdx.x; j < wr / 4; j += kMarkThreads) s4[j] = make_uint4(0u, 0u, 0u, 0u);
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();

  if (n_live) n = min(n, (int64_t)max(*n_live, 0));   // the slices divide the LIVE list
  const int64_t chunk = (n + S - 1) / S;
  const int64_t first = (int64_t)slice * chunk, last = min(n, first + chunk);
  bool bad = false;
  for (int64_t i = first + threadIdx.x; i < last; i += (int64_t)kMarkLoads * kMarkThreads) {
    int64_t id[kMarkLoads];
#pragma unroll
    for (int k = 0; k < kMarkLoads; k++) id[k] = i + k * kMarkThreads < last ? (int64_t)ids[i + k * kMarkThreads] : -1;
#pragma unroll
    for (int k = 0; k < kMarkLoads; k++) {
      bad |= id[k] >= bound;
      if (id[k] >= 0 && id[k] < bound && (id[k] >> kRangeBits) == r) {
        const uint32_t bit = (uint32_t)id[k] & ((1u << kRangeBits) - 1u), m = 1u << (bit & 31);
        // test first: the lanes of a wave that name one hub would queue up behind one LDS address
        if ((s_bits[bit >> 5] & m) == 0) atomicOr(&s_bits[bit >> 5], m);
      }
    }
  }
  if (bad) s_bad = 1;   // (every such lane writes the same value)
  __syncthreads();
  uint4* out = reinterpret_cast<uint4*>(slabs + (int64_t)slice * row_words + (int64_t)r * kRangeWords);
  for (int j = threadIdx.x; j < wr / 4; j += kMarkThreads) out[j] = s4[j];
  if (threadIdx.x == 0) bad_flags[slice * R + r] = s_bad;
}

// OR of the S slabs, word by word -> rank[w].x, and the ids set in every kSumTile words -> tsum.  Four waves share a tile's
// slabs (s = wave, wave + 4, ...) so that a word's S loads are spread over enough waves to be in flight together.  Block 0
// also folds the workgroups' out-of-bound flags into the caller's word: no memset before the chain, no copy behind it.
__global__ void __launch_bounds__(256) unique_lds_reduce_kernel(const uint32_t* __restrict__ slabs, int S, int64_t row_words, int64_t n_words,
                                                                uint2* __restrict__ rank, int* __restrict__ tsum,
                                                                const int* __restrict__ bad_flags, int n_flags, int* __restrict__ out_of_bound)
{
  __shared__ uint32_t part[4][kSumTile];
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * kSumTile + j;   // < row_words: the slabs are padded to whole tiles (with zeros)
  uint32_t v = 0;
#pragma unroll 8
  for (int s = g; s < S; s += 4) v |= slabs[(int64_t)s * row_words + w];
  part[g][j] = v;
  __syncthreads();
  if (g == 0) {
    v = part[0][j] | part[1][j] | part[2][j] | part[3][j];
    if (w < n_words) rank[w].x = v;
    int c = __popc(v);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if (j == 0) tsum[blockIdx.x] = c;
  }
  if (blockIdx.x == 0 && out_of_bound) {
    int any = 0;
    for (int t = threadIdx.x; t < n_flags; t += 256) any |= bad_flags[t];
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) *out_of_bound = any ? 1 : 0;
  }
}

// Scan and compaction in one launch: a workgroup of 256 words adds up the tile counts below its first word itself (at most
// a few thousand ints out of L2 for the bounds the LDS path takes), scans its own 256 counts and writes {bits, prefix} and
// the ids.  The last workgroup publishes the number of distinct ids.
__global__ void __launch_bounds__(256) unique_scan_compact_kernel(uint2* __restrict__ rank, const int* __restrict__ tsum, int64_t n_words,
                                                                  int64_t* __restrict__ distinct, int* __restrict__ n_distinct)
{
  __shared__ int wave_cnt[4], wave_below[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int below = 0;
  for (int64_t t = threadIdx.x; t < (int64_t)blockIdx.x * (256 / kSumTile); t += 256) below += tsum[t];
  uint32_t word = w < n_words ? rank[w].x : 0u;
  const int c   = __popc(word);
  int inc       = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) below += __shfl_xor(below, d, 64);
  if (lane == 63) wave_cnt[wave] = inc;
  if (lane == 0) wave_below[wave] = below;
  __syncthreads();
  int at = wave_below[0] + wave_below[1] + wave_below[2] + wave_below[3] + inc - c;
  for (int k = 0; k < wave; k++) at += wave_cnt[k];
  if (w == n_words - 1) *n_distinct = at + c;
  if (w >= n_words) return;
  rank[w].y = (uint32_t)at;   // {bits, ids set below this word} side by side: ONE scattered 8-byte load per look-up
  while (word) {
    const int k    = __ffs(word) - 1;
    distinct[at++] = w * 32 + k;
    word &= word - 1;
  }
}

// ---- which path (by shape only) -----------------------------------------------------------------------------------------------
// (the rule and its measurements: header of this file)
#ifndef WGAMD_UNIQUE_FORCE_PATH   // measurement builds only (profiles/r08): 0 = byte marks everywhere, 1 = LDS marks everywhere
constexpr int kLdsMaxRanges = 8;
#else
constexpr int kLdsMaxRanges = kMarkBlocks;
#endif
inline int lds_ranges(int64_t bound) { return (int)((bound + (1 << kRangeBits) - 1) >> kRangeBits); }
inline bool lds_bound(int64_t bound) { return lds_ranges(bound) <= kLdsMaxRanges; }
inline bool lds_path(int64_t n, int64_t bound)
{
#ifdef WGAMD_UNIQUE_FORCE_PATH
  (void)n;
  return WGAMD_UNIQUE_FORCE_PATH != 0 && lds_bound(bound);
#else
  (void)n;
  return lds_bound(bound);
#endif
}
#ifndef WGAMD_UNIQUE_XCD_GROUP
#define WGAMD_UNIQUE_XCD_GROUP 1
#endif
// slices of a launch over R ranges: every XCD label gets floor(32 / R) slices when the ranges of a slice are grouped
inline int lds_max_slices(int R)
{
  if (WGAMD_UNIQUE_XCD_GROUP && R <= 32) return 8 * (32 / R);
  return std::max(1, kMarkBlocks / R);
}

struct unique_plan {
  size_t flags, bits, cnt, tmp, bad, slabs, tsum, bad_flags, total;
  int64_t n_words, cnt_padded, row_words;
};
unique_plan plan_unique(int64_t bound)
{
  unique_plan p{};
  size_t at = 0;
  auto add  = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  p.n_words    = (bound + 31) / 32;
  p.cnt_padded = (p.n_words + kScanTile) / kScanTile * kScanTile;   // counts are read by the scan in whole tiles
  p.flags = add((size_t)p.n_words * 32);
  p.bits  = add(sizeof(uint2) * (size_t)p.n_words);
  p.cnt   = add(sizeof(int) * (size_t)(p.cnt_padded + 1));           // scanned in place: prefix[n_words] = number of distinct ids
  p.tmp   = add(sizeof(int) * (size_t)scan_tmp_ints(p.n_words));
  p.bad   = add(sizeof(int));
  p.row_words = (p.n_words + kSumTile - 1) / kSumTile * kSumTile;
  if (lds_bound(bound)) {   // sized for every n: the plan knows the bound only
    p.slabs     = add(sizeof(uint32_t) * (size_t)lds_max_slices(lds_ranges(bound)) * (size_t)p.row_words);
    p.tsum      = add(sizeof(int) * (size_t)(p.row_words / kSumTile));
    p.bad_flags = add(sizeof(int) * (size_t)kMarkBlocks);
  }
  p.total = at;
  return p;
}

}  // namespace
}  // namespace wgamd

extern "C" {

size_t wgamd_unique_bounded_workspace_bytes(int64_t id_bound)
{
  if (id_bound <= 0 || id_bound >= ((int64_t)1 << 31) - 4096) return 0;
  return wgamd::plan_unique(id_bound).total;
}

wholememory_error_code_t wgamd_unique_bounded(const void* ids, wholememory_dtype_t id_dtype, int64_t n, int64_t id_bound,
                                              int64_t* distinct, int* inverse, int* n_distinct_dev, int* out_of_bound_dev,
                                              void* workspace, size_t workspace_bytes, void* stream)
{
  return wgamd_unique_bounded_live(ids, id_dtype, n, nullptr, id_bound, distinct, inverse, n_distinct_dev, out_of_bound_dev,
                                   workspace, workspace_bytes, stream);
}

wholememory_error_code_t wgamd_unique_bounded_live(const void* ids, wholememory_dtype_t id_dtype, int64_t n, const int* n_live_dev,
                                                   int64_t id_bound, int64_t* distinct, int* inverse, int* n_distinct_dev,
                                                   int* out_of_bound_dev, void* workspace, size_t workspace_bytes, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_unique_bounded", [&] {
    WG_REQUIRE_INPUT(id_dtype == WHOLEMEMORY_DT_INT || id_dtype == WHOLEMEMORY_DT_INT64, "id dtype must be INT|INT64");
    WG_REQUIRE_INPUT(n >= 0 && n < ((int64_t)1 << 31), "bad id count");
    WG_REQUIRE_INPUT(id_bound > 0 && id_bound < ((int64_t)1 << 31) - 4096, "id_bound must be in (0, 2^31)");
    WG_REQUIRE_INPUT(n_distinct_dev && workspace && (n == 0 || (ids && distinct && inverse)), "null pointer");
    const unique_plan p = plan_unique(id_bound);
    WG_REQUIRE_INPUT(workspace_bytes >= p.total, "workspace too small: need %zu bytes", p.total);
    WG_REQUIRE_INPUT((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base     = static_cast<char*>(workspace);
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + p.flags);
    uint2* rank    = reinterpret_cast<uint2*>(base + p.bits);
    int* cnt       = reinterpret_cast<int*>(base + p.cnt);
    int* tmp       = reinterpret_cast<int*>(base + p.tmp);
    int* bad       = reinterpret_cast<int*>(base + p.bad);
    const bool ids64 = id_dtype == WHOLEMEMORY_DT_INT64;
    auto look_up     = [&] {
      if (n == 0) return;
      const int grid = (int)std::min<int64_t>(ceil_div(n, 256), 256 * 32);
      if (!ids64) unique_inverse_kernel<int32_t><<<grid, 256, 0, st>>>(static_cast<const int32_t*>(ids), n, id_bound, rank, inverse, n_live_dev);
      else unique_inverse_kernel<int64_t><<<grid, 256, 0, st>>>(static_cast<const int64_t*>(ids), n, id_bound, rank, inverse, n_live_dev);
      WG_HIP_CHECK(hipGetLastError());
    };
    if (lds_path(n, id_bound)) {
      const int R = lds_ranges(id_bound);
      // slices: by the CAPACITY n (the live count is on the device); a short list does not wake every CU
      const int S         = (int)std::max<int64_t>(1, std::min<int64_t>(lds_max_slices(R), ceil_div(n, kMinSlice)));
      const int xcd_group = WGAMD_UNIQUE_XCD_GROUP && R <= 32;
      const int grid      = xcd_group ? 8 * R * ceil_div(S, 8) : S * R;
      const size_t lds    = sizeof(uint32_t) * (size_t)std::min<int64_t>(kRangeWords, p.row_words);
      uint32_t* slabs     = reinterpret_cast<uint32_t*>(base + p.slabs);
      int* tsum           = reinterpret_cast<int*>(base + p.tsum);
      int* bad_flags      = reinterpret_cast<int*>(base + p.bad_flags);
      auto mark           = [&](auto kern, auto* typed) {
        if (lds > 64 * 1024)
          WG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kern<<<grid, kMarkThreads, lds, st>>>(typed, n, id_bound, R, S, xcd_group, p.row_words, slabs, bad_flags, n_live_dev);
        WG_HIP_CHECK(hipGetLastError());
      };
      if (!ids64) mark(unique_lds_mark_kernel<int32_t>, static_cast<const int32_t*>(ids));
      else mark(unique_lds_mark_kernel<int64_t>, static_cast<const int64_t*>(ids));
      unique_lds_reduce_kernel<<<(int)(p.row_words / kSumTile), 256, 0, st>>>(slabs, S, p.row_words, p.n_words, rank, tsum, bad_flags, S * R,
                                                                            out_of_bound_dev);
      unique_scan_compact_kernel<<<(int)ceil_div(p.n_words, 256), 256, 0, st>>>(rank, tsum, p.n_words, distinct, n_distinct_dev);
      WG_HIP_CHECK(hipGetLastError());
      look_up();
      return;
    }
    WG_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)p.n_words * 32, st));
    WG_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), st));
    if (n > 0) {
      const int grid = (int)std::min<int64_t>(ceil_div(n, 256), 256 * 32);
      if (id_dtype == WHOLEMEMORY_DT_INT) unique_mark_kernel<int32_t><<<grid, 256, 0, st>>>(static_cast<const int32_t*>(ids), n, id_bound, flags, bad, n_live_dev);
      else unique_mark_kernel<int64_t><<<grid, 256, 0, st>>>(static_cast<const int64_t*>(ids), n, id_bound, flags, bad, n_live_dev);
      WG_HIP_CHECK(hipGetLastError());
    }
    unique_pack_kernel<<<(int)ceil_div(p.cnt_padded, 256), 256, 0, st>>>(flags, p.n_words, rank, cnt, p.cnt_padded);
    exclusive_scan_i32(cnt, cnt, p.n_words, tmp, st);   // cnt[w] -> ids set below word w; cnt[n_words] = number of distinct ids
    unique_compact_kernel<<<(int)ceil_div(p.n_words, 256), 256, 0, st>>>(rank, cnt, p.n_words, distinct, n_distinct_dev);
    WG_HIP_CHECK(hipGetLastError());
    look_up();
    if (out_of_bound_dev) WG_HIP_CHECK(hipMemcpyAsync(out_of_bound_dev, bad, sizeof(int), hipMemcpyDeviceToDevice, st));
  });
}

}  // extern "C"
