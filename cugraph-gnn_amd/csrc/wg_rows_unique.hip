// Row-wise first-appearance de-duplication of a link call group's seed-edge endpoints (include/wgamd_ext.h:
// wgamd_rows_first_unique): ends [G, S] -> per row its distinct values in order of first position, the rows' lists back to back
// (uniq, seg, batch), and for every element its position in its row's list (local).  The torch formulation sorts G S keys
// (torch.unique) inside a dozen ops and reads one size back; here it is TWO launches and nothing comes back to the host.
//
// Launch 1, one workgroup per row (bounded grid, stride over rows): an open-addressing table in LDS holds per distinct id
// the packed word [id : 40 | smallest position : 24] — the word of wg_append_unique.hip's per-batch tables.  Insert is a compare-
// and-swap on an empty slot (all ones: never a live word, positions stay below 2^24 - 1) or an LDS min on the slot that already
// holds the id, so after the barrier every slot holds a well-defined minimum whatever the order of the lanes.  "Position s is a
// first appearance" is minpos(ends[g, s]) == s; a ballot per wave and pass plus one scan of the wave counts ranks those flags in
// position order; the rank replaces the position in the slot, so local[g, s] is one more look at the slot the element already
// found.  The row's list goes to the workspace at g S + rank (the group-wide compaction would overlap it in uniq), its count to
// the workspace too.  The last workgroup to finish (the ticket of wg_xent.hip) scans the counts into seg.
// Launch 2 moves every list to seg[g] in uniq, writes batch and zeroes both tails.
//
// Memory safety does not rest on the promise about the values: an id is masked to 40 bits before it is hashed or packed, every
// store is addressed by a position or by a rank (< S by construction), and a row inserts at most S ids into >= 2 S slots, so a
// probe always ends.  Values outside [0, 2^40) give a de-duplication of their low 40 bits, nothing worse.
//
// wgamd_rows_first_values (further down) carries a value per element to the lists: the value at an id's first position, e.g. the
// seed time of a de-duplicated endpoint of a temporal link call group.
#include "wg_common.hpp"
#include "wgamd_ext.h"

namespace wgamd {
namespace {

constexpr int kRowsPosBits   = 24;
constexpr int kRowsIdBits    = 40;
constexpr int kRowsMaxS      = WGAMD_ROWS_FIRST_UNIQUE_MAX_S;   // 2 S slots of 8 B = 128 KiB of the CU's 160 KiB of LDS
constexpr int kRowsMaxPasses = 8;                               // positions per thread
constexpr int kRowsBigBlock  = 1024;
constexpr int kRowsSmallBlock = 256;
constexpr int kRowsSmallMaxS = 512;                             // rows up to here run on the small workgroup
constexpr int kRowsMaxGrid   = 1024;
constexpr unsigned long long kRowsEmpty   = ~0ull;
constexpr unsigned long long kRowsPosMask = (1ull << kRowsPosBits) - 1;
constexpr unsigned long long kRowsIdMask  = (1ull << kRowsIdBits) - 1;

static_assert(kRowsMaxS <= kRowsBigBlock * kRowsMaxPasses && kRowsSmallMaxS <= kRowsSmallBlock * kRowsMaxPasses, "passes");
static_assert(kRowsMaxS < (1 << kRowsPosBits) - 1, "the empty mark must not be a live word");

__device__ __forceinline__ int rows_wave_inclusive(int v, int lane)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// workspace: ticket (int) | counts [G] | lists [G, S]
template <int T>
__global__ void __launch_bounds__(T)
rows_first_unique_kernel(const int64_t* __restrict__ ends, int64_t G, int S, int lg_slots, int64_t* __restrict__ lists,
                         int* __restrict__ counts, int64_t* __restrict__ local, int* __restrict__ ticket, int* __restrict__ seg)
{
  constexpr int NW = T / 64;
  extern __shared__ __align__(8) unsigned long long table[];
  __shared__ int s_wave[kRowsMaxPasses * NW];
  __shared__ int s_total, s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slots = 1 << lg_slots, mask = slots - 1;
  const int passes = (S + T - 1) / T;

  for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
    for (int i = tid; i < slots; i += T) table[i] = kRowsEmpty;
    __syncthreads();
    const int64_t* row = ends + g * S;
    int64_t v[kRowsMaxPasses];
    int slot[kRowsMaxPasses];
#pragma unroll
    for (int k = 0; k < kRowsMaxPasses; k++) {
      const int s = k * T + tid;
      v[k] = 0, slot[k] = 0;
      if (k < passes && s < S) {
        v[k]                          = row[s];
        const unsigned long long id   = (unsigned long long)v[k] & kRowsIdMask;
        const unsigned long long word = (id << kRowsPosBits) | (unsigned long long)s;
        int h = (int)((id * 0x9E3779B97F4A7C15ull) >> (64 - lg_slots));
        for (;;) {
          const unsigned long long old = atomicCAS(&table[h], kRowsEmpty, word);
          if (old == kRowsEmpty) break;
          if ((old >> kRowsPosBits) == id) {
            atomicMin(&table[h], word);
            break;
          }
          h = (h + 1) & mask;
        }
        slot[k] = h;
      }
    }
    __syncthreads();
    unsigned first = 0;
#pragma unroll
    for (int k = 0; k < kRowsMaxPasses; k++) {
      if (k < passes) {   // (uniform: whole waves take the ballot)
        const int s  = k * T + tid;
        const bool f = s < S && (int)(table[slot[k]] & kRowsPosMask) == s;
        const unsigned long long b = __ballot(f);
        if (f) first |= 1u << k;
        if (lane == 0) s_wave[k * NW + wave] = __popcll(b);
      }
    }
    __syncthreads();
    if (wave == 0) {   // passes * NW <= 128 wave counts, two per lane, in (pass, wave) = position order
      const int n = passes * NW;
      const int a = 2 * lane < n ? s_wave[2 * lane] : 0, b = 2 * lane + 1 < n ? s_wave[2 * lane + 1] : 0;
      const int incl = rows_wave_inclusive(a + b, lane);
      if (2 * lane < n) s_wave[2 * lane] = incl - a - b;
      if (2 * lane + 1 < n) s_wave[2 * lane + 1] = incl - b;
      if (lane == 63) s_total = incl;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRowsMaxPasses; k++) {
      if (k < passes) {
        const bool f = (first >> k) & 1u;
        const unsigned long long b = __ballot(f);
        if (f) {
          const int rank = s_wave[k * NW + wave] + __popcll(b & ((1ull << lane) - 1ull));
          table[slot[k]] = (table[slot[k]] & ~kRowsPosMask) | (unsigned long long)rank;   // the one writer of this slot
          lists[g * S + rank] = v[k];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRowsMaxPasses; k++) {
      const int s = k * T + tid;
      if (k < passes && s < S) local[g * S + s] = (int64_t)(table[slot[k]] & kRowsPosMask);
    }
    if (tid == 0) counts[g] = s_total;
    __syncthreads();   // the table and s_wave are the next row's
  }

  if (tid == 0) {
    __threadfence();
    s_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  int carry = 0;   // the same in every thread
  if (tid == 0) seg[0] = 0;
  for (int64_t base = 0; base < G; base += T) {
    const int64_t g = base + tid;
    const int c     = g < G ? __hip_atomic_load(&counts[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    int incl        = rows_wave_inclusive(c, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int t = s_wave[w];
      before += w < wave ? t : 0;
      all += t;
    }
    if (g < G) seg[g + 1] = carry + before + incl;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *ticket = 0;   // (the workspace is reusable without a memset)
}

__global__ void __launch_bounds__(256)
rows_compact_kernel(const int64_t* __restrict__ lists, const int* __restrict__ seg, int64_t G, int S, int64_t* __restrict__ uniq,
                    int* __restrict__ batch)
{
  const int64_t total = G * S, live = seg[G];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)((unsigned)i / (unsigned)S), r = (int)(i - (int64_t)g * S);
    const int b = seg[g], n = seg[g + 1] - b;    // n <= S, b + n <= live <= total: launch 1 counted ranks, not values
    if (r < n) {
      uniq[b + r]  = lists[i];
      batch[b + r] = g;
    }
    if (i >= live) uniq[i] = 0, batch[i] = 0;
  }
}

// wgamd_rows_first_values: a value per distinct id of a row, taken at the id's first position.  The lists are numbered in order
// of first position, so s is a first position exactly when local[g, s] is larger than every earlier local[g, .]: one workgroup
// per row walks it 256 positions at a time with an exclusive prefix maximum (a wave scan, the waves' maxima in LDS, the running
// maximum of the row carried from pass to pass) and stores once per first position, at seg[g] + local[g, s].  A local outside
// [0, S) counts as no position at all, and a store needs its slot below seg[G] <= G S: nothing lands outside `out`.  The tail
// from seg[G] on is zeroed by the whole grid.
constexpr int kRowsValThreads = 256;

__global__ void __launch_bounds__(kRowsValThreads)
rows_first_values_kernel(const int64_t* __restrict__ local, const int* __restrict__ seg, const int64_t* __restrict__ values,
                         int64_t G, int S, int64_t* __restrict__ out)
{
  constexpr int T = kRowsValThreads, NW = T / 64;
  __shared__ int s_wave[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t total = G * S;
  const int64_t live  = min(max((int64_t)seg[G], (int64_t)0), total);
  for (int64_t i = live + (int64_t)blockIdx.x * T + tid; i < total; i += (int64_t)gridDim.x * T) out[i] = 0;

  for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
    const int64_t base = (int64_t)seg[g];
    int carry = -1;   // the running maximum of the row before this pass: the same in every thread
    for (int s0 = 0; s0 < S; s0 += T) {
      const int s     = s0 + tid;
      const int64_t l = s < S ? local[g * S + s] : -1;
      const int mine  = (l >= 0 && l < S) ? (int)l : -1;
      int incl        = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl = max(incl, up);
      }
      int before = __shfl_up(incl, 1, 64);
      if (lane == 0) before = -1;
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      int all = carry;
      before  = max(before, carry);
#pragma unroll
      for (int w = 0; w < NW; w++) {
        const int t = s_wave[w];
        if (w < wave) before = max(before, t);
        all = max(all, t);
      }
      if (mine > before) {
        const int64_t at = base + mine;
        if (at >= 0 && at < live) out[at] = values[g * S + s];
      }
      carry = all;
      __syncthreads();   // s_wave is the next pass's
    }
  }
}

struct rows_ws {
  int* ticket;
  int* counts;
  int64_t* lists;
};

inline size_t rows_counts_bytes(int64_t G) { return ((size_t)G * sizeof(int) + 255) / 256 * 256; }

inline rows_ws rows_carve(void* workspace, int64_t G)
{
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  return {reinterpret_cast<int*>(p), reinterpret_cast<int*>(p + 256), reinterpret_cast<int64_t*>(p + 256 + rows_counts_bytes(G))};
}

template <int T>
void rows_launch(const int64_t* ends, int64_t G, int S, const rows_ws& w, int64_t* local, int* seg, hipStream_t st)
{
  int lg_slots = 6;
  while ((1 << lg_slots) < 2 * S) lg_slots++;
  const size_t lds = sizeof(unsigned long long) << lg_slots;
  auto kern        = rows_first_unique_kernel<T>;
  if (lds > 48 * 1024)
    WG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned grid = (unsigned)std::min<int64_t>(G, kRowsMaxGrid);
  kern<<<grid, T, lds, st>>>(ends, G, S, lg_slots, w.lists, w.counts, local, w.ticket, seg);
  WG_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace wgamd

extern "C" {

int wgamd_rows_first_unique_supported(int64_t n_rows, int64_t row_len, int64_t n_ids)
{
  using namespace wgamd;
  return n_rows >= 1 && row_len >= 1 && row_len <= kRowsMaxS && n_rows <= (((int64_t)1 << 31) - 1) / row_len && n_ids >= 1 &&
         n_ids <= ((int64_t)1 << kRowsIdBits);
}

size_t wgamd_rows_first_unique_workspace_bytes(int64_t n_rows, int64_t row_len)
{
  using namespace wgamd;
  if (n_rows < 1 || row_len < 1 || row_len > kRowsMaxS || n_rows > (((int64_t)1 << 31) - 1) / row_len) return 0;
  return 256 + 256 + rows_counts_bytes(n_rows) + (size_t)n_rows * (size_t)row_len * sizeof(int64_t);
}

wholememory_error_code_t wgamd_rows_first_unique(const int64_t* ends, int64_t n_rows, int64_t row_len, int64_t n_ids, int64_t* uniq,
                                                 int* seg, int* batch, int64_t* local, void* workspace, size_t workspace_bytes,
                                                 int workspace_is_zeroed, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_rows_first_unique", [&] {
    WG_REQUIRE_INPUT(wgamd_rows_first_unique_supported(n_rows, row_len, n_ids), "outside the domain (wgamd_rows_first_unique_supported)");
    WG_REQUIRE_INPUT(ends && uniq && seg && batch && local && workspace, "null pointer");
    WG_REQUIRE_INPUT(workspace_bytes >= wgamd_rows_first_unique_workspace_bytes(n_rows, row_len), "workspace too small");
    auto st         = static_cast<hipStream_t>(stream);
    const rows_ws w = rows_carve(workspace, n_rows);
    if (!workspace_is_zeroed) WG_HIP_CHECK(hipMemsetAsync(w.ticket, 0, 256, st));
    const int S = (int)row_len;
    if (S <= kRowsSmallMaxS)
      rows_launch<kRowsSmallBlock>(ends, n_rows, S, w, local, seg, st);
    else
      rows_launch<kRowsBigBlock>(ends, n_rows, S, w, local, seg, st);
    const int64_t total = n_rows * row_len;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    rows_compact_kernel<<<grid, 256, 0, st>>>(w.lists, seg, n_rows, S, uniq, batch);
    WG_HIP_CHECK(hipGetLastError());
  });
}

wholememory_error_code_t wgamd_rows_first_values(const int64_t* local, const int* seg, const int64_t* values, int64_t n_rows,
                                                 int64_t row_len, int64_t* out, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_rows_first_values", [&] {
    WG_REQUIRE_INPUT(wgamd_rows_first_unique_supported(n_rows, row_len, 1), "outside the domain (wgamd_rows_first_unique_supported)");
    WG_REQUIRE_INPUT(local && seg && values && out, "null pointer");
    const unsigned grid = (unsigned)std::min<int64_t>(n_rows, kRowsMaxGrid);
    rows_first_values_kernel<<<grid, kRowsValThreads, 0, static_cast<hipStream_t>(stream)>>>(local, seg, values, n_rows, (int)row_len,
                                                                                             out);
    WG_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
