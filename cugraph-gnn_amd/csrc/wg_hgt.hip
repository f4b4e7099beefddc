// Heterogeneous Graph Transformer layer (torch_geometric.nn.HGTConv) over one (hop, destination type) of a call group.  The
// caller has folded the node-type key / value weights, the relation's head-wise D x D maps and its prior into one operand per
// relation, so a source row j of relation r holds  kv_r[j] = [ k'_j | v'_j ]  (2C floats side by side: one contiguous read per
// edge fetches both) with  k'_j[h] = (k_j[h] @ k_rel[r, h]) p_rel[r][h] / sqrt(D),  v'_j[h] = v_j[h] @ v_rel[r, h]:
//     logit_ijh = q_i[h] . k'_j[h]
//     alpha     = softmax over ALL edges into i of ALL relations, per head
//     agg_i     = sum alpha_ijh v'_j[h]                                                  (0 for a row without any edge)
//     o_i       = gelu(agg_i) @ w_out^T + b_out                                          (exact, erf GELU)
//     out[p]    = act( g o_i + (1 - g) XD[i] ),  g = sigmoid(*skip)  (skip null: out = act(o_i)),  p = out_rows ? out_rows[i] : i
//
//   * hgt_layer_kernel — ONE launch whatever the number of relations.  A workgroup of 4 waves owns a 16-row tile; one wave per
//     destination row, a lane = one float4 of the C-wide row (D % 4 == 0: a lane's columns lie in one head).  q_i stays in
//     registers; the wave walks relation after relation, four neighbour rows in flight (k4 and v4 of each loaded once), the logit
//     per head by butterflies inside the head's lanes (masked wave sums when D / 4 is no power of two).  ONE online softmax state
//     (m, l, acc) per head runs across all relations of the row — the running maximum carries from one relation's CSR row into
//     the next, the accumulators are rescaled once per group of edges.  gelu(acc / l) goes to an LDS tile; the out_lin product is
//     tile_times_wt (wg_layer_parts.hpp, the exact fp32 matrix pipe) into a second LDS tile the way the GIN family's first
//     product does; the gate (skip read on the device), ReLU and the row placement follow as float4 stores.  A training launch
//     also writes the pre-GELU agg [n, C] and one log-sum-exp per (row, head): nothing per edge, no concatenated edge list.
//   * hgt_bwd_dst_kernel — destination-major, one wave per row: delta_ih = dagg_ih . agg_ih, then all relations again with
//     alpha = exp(q.k' - lse), ds = alpha (dagg_ih . v'_j - delta_ih), dq_i += ds k'_j.  Writes dq [n, C] and delta [n, H].
//   * hgt_bwd_src_kernel — source-major over one relation hop's transpose, one wave per source row holding kv_j: every entry
//     reads q, dagg, lse and delta of its destination, recomputes alpha and ds, dkv_j = [ sum ds q_i | sum alpha dagg_i ] in
//     transposed-CSR order (a hub source is one wave's sequential walk, four entries in flight).  Every row of dkv is written.
// No atomics anywhere: the same bits from run to run.
#include "wg_gatv2_parts.hpp"

namespace wgamd {
namespace {

constexpr int kHgtMaxRel = WGAMD_HETERO_SAGE_MAX_RELATIONS;
constexpr int kHgtMaxC   = 256;   // one float4 of the row per lane
constexpr int kHgtEdges  = 4;     // neighbour rows of a destination (destinations of a source) in flight
constexpr int kHgtBwdRows = 4;    // rows per workgroup of the two backward kernels: one per wave

struct hgt_args {
  wgamd_hgt_relation_t rel[kHgtMaxRel];
  int n_rel, H, C;
  int64_t n_rows;
  const float* q;             // [n_rows, ldq]
  int64_t ldq;
  const float* wo;            // [C, ldwo]
  int64_t ldwo;
  const float* bo;            // nullable
  const float* skip;          // ONE float on the device; null = no gate
  const float* x_dst;         // the gate's other side: XD[i] = x_dst[ids[dst_rows ? dst_rows[i] : i]]
  int64_t ldx_dst;
  const int64_t* dst_rows;
  const void* dst_ids;
  int dst_kind;
  int relu;
  const int64_t* out_rows;
  float* out;
  int64_t ldo;
  float* agg_out;             // nullable
  int64_t ld_agg;
  float* lse_out;             // nullable: [n_rows, ld_lse], H used
  int64_t ld_lse;
  int C16, SD;
};

// k'4 / v'4 of the neighbour rows of edges [e0, e0 + 4) below t (zeros past the row's end and in the lanes behind the row)
__device__ __forceinline__ void hgt_load_group(const wgamd_hgt_relation_t& R, int e0, int t, int lane, bool on, int C4,
                                               f32x4 (&k)[kHgtEdges], f32x4 (&v)[kHgtEdges])
{
#pragma unroll
  for (int u = 0; u < kHgtEdges; ++u) {
    k[u] = v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (e0 + u < t && on) {
      const f32x4* row = reinterpret_cast<const f32x4*>(R.kv + (int64_t)R.col[e0 + u] * R.ldkv);
      k[u] = row[lane];
      v[u] = row[C4 + lane];
    }
  }
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

template <int LPH>
__global__ void __launch_bounds__(kThreads) hgt_layer_kernel(hgt_args a)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int rp[kHgtMaxRel][kTileRows + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, a.n_rows - row0);
  const int C4 = a.C / 4, lph = C4 / a.H;
  const bool on = lane < C4;
  const int hd = lane / lph;                       // (the lanes behind the row: hd >= H, no head)
  load_row_windows(rp, a.rel, a.n_rel, row0, rows_here);
  zero_tile_padding(tile, a.SD, a.C, a.C16);
  __syncthreads();

  // ---- phase 1: one wave per destination row, ONE softmax across the relations in turn ----
  for (int lr = wave; lr < kTileRows; lr += 4) {
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    if (lr < rows_here) {
      const int64_t i = row0 + lr;
      f32x4 q4 = {0.f, 0.f, 0.f, 0.f}, acc = q4;
      if (on) q4 = reinterpret_cast<const f32x4*>(a.q + i * a.ldq)[lane];
      float m = -INFINITY, l = 0.f;
      for (int r = 0; r < a.n_rel; ++r) {
        const wgamd_hgt_relation_t& R = a.rel[r];
        const int s = rp[r][lr], t = rp[r][lr + 1];
        for (int e0 = s; e0 < t; e0 += kHgtEdges) {
          f32x4 k[kHgtEdges], v[kHgtEdges];
          hgt_load_group(R, e0, t, lane, on, C4, k, v);
          float sc[kHgtEdges];
          float mx = m;
#pragma unroll
          for (int u = 0; u < kHgtEdges; ++u) {
            sc[u] = head_sum<LPH>(dot4(q4, k[u]), hd, a.H);
            if (e0 + u < t) mx = fmaxf(mx, sc[u]);
          }
          const float rs = expf(m - mx);           // (m = -inf before the row's first group, in whatever relation: rs = 0)
          acc *= rs;
          l *= rs;
          f32x4 ga = {0.f, 0.f, 0.f, 0.f};         // the group's terms enter the running sums as ONE term
          float gl = 0.f;
#pragma unroll
          for (int u = 0; u < kHgtEdges; ++u) {
            if (e0 + u < t) {
              const float p = expf(sc[u] - mx);
              ga += p * v[u];
              gl += p;
            }
          }
          acc += ga;
          l += gl;
          m = mx;
        }
      }
      const float inv = l > 0.f ? 1.f / l : 0.f;   // (no edge in any relation: acc = 0 and inv = 0 — agg is exactly zero)
      const f32x4 agg = acc * inv;
      if (on) {
        if (a.agg_out) reinterpret_cast<f32x4*>(a.agg_out + i * a.ld_agg)[lane] = agg;
        if (a.lse_out && lane % lph == 0) a.lse_out[i * a.ld_lse + hd] = l > 0.f ? m + logf(l) : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = gelu_erf(agg[c]);
      }
    }
    if (on) reinterpret_cast<f32x4*>(tile + lr * a.SD)[lane] = y;
  }
  __syncthreads();

  // ---- phase 2: [16 x C16] tile @ w_out^T + b_out -> the second LDS tile (all 16 rows: rows past n_rows are never written out) ----
  float* hid = tile + kTileRows * a.SD;
  tile_times_wt(tile, a.SD, a.C, a.C16, a.wo, a.ldwo, a.C, a.bo, 0, hid, a.SD, 0, kTileRows);
  __syncthreads();

  // ---- the gate against the destination row, ReLU, placement: float4 stores ----
  const float g = a.skip ? 1.f / (1.f + expf(-*a.skip)) : 1.f;
  for (int idx = tid; idx < rows_here * C4; idx += kThreads) {
    const int r = idx / C4, c = idx % C4;
    const int64_t i = row0 + r;
    f32x4 o = reinterpret_cast<const f32x4*>(hid + r * a.SD)[c];
    if (a.skip) {
      const int64_t self = a.dst_rows ? a.dst_rows[i] : i;
      const f32x4 x4 = reinterpret_cast<const f32x4*>(row_of(a.x_dst, a.ldx_dst, a.dst_ids, a.dst_kind, self))[c];
      o = g * o + (1.f - g) * x4;
    }
    if (a.relu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
    }
    reinterpret_cast<f32x4*>(a.out + (a.out_rows ? a.out_rows[i] : i) * a.ldo)[c] = o;
  }
}

// ---- destination-major backward: dq and delta ------------------------------------------------------------------------------------
struct hgt_bwd_args {
  wgamd_hgt_relation_t rel[kHgtMaxRel];
  int n_rel, H, C;
  int64_t n_rows;
  const float* q;
  int64_t ldq;
  const float* dagg;          // dL / d agg (pre-GELU)
  int64_t ld_dagg;
  const float* agg;
  int64_t ld_agg;
  const float* lse;
  int64_t ld_lse;
  float* dq;
  int64_t ld_dq;
  float* delta;               // [n_rows, ld_delta], H used
  int64_t ld_delta;
};

template <int LPH>
__global__ void __launch_bounds__(kThreads) hgt_bwd_dst_kernel(hgt_bwd_args a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kHgtBwdRows + wave;
  if (i >= a.n_rows) return;                       // (the whole wave)
  const int C4 = a.C / 4, lph = C4 / a.H;
  const bool on = lane < C4;
  const int hd = lane / lph;
  f32x4 q4 = {0.f, 0.f, 0.f, 0.f}, g4 = q4, o4 = q4, dq = q4;
  float L = 0.f;
  if (on) {
    q4 = reinterpret_cast<const f32x4*>(a.q + i * a.ldq)[lane];
    g4 = reinterpret_cast<const f32x4*>(a.dagg + i * a.ld_dagg)[lane];
    o4 = reinterpret_cast<const f32x4*>(a.agg + i * a.ld_agg)[lane];
    L  = a.lse[i * a.ld_lse + hd];
  }
  const float dl = head_sum<LPH>(dot4(g4, o4), hd, a.H);      // sum_j alpha_ij (dagg . v'_j) = dagg . agg
  for (int r = 0; r < a.n_rel; ++r) {
    const wgamd_hgt_relation_t& R = a.rel[r];
    const int s = R.row_ptr[i], t = R.row_ptr[i + 1];
    for (int e0 = s; e0 < t; e0 += kHgtEdges) {
      f32x4 k[kHgtEdges], v[kHgtEdges];
      hgt_load_group(R, e0, t, lane, on, C4, k, v);
#pragma unroll
      for (int u = 0; u < kHgtEdges; ++u) {
        if (e0 + u < t) {                          // (the whole wave)
          const float sc = head_sum<LPH>(dot4(q4, k[u]), hd, a.H);
          const float dv = head_sum<LPH>(dot4(g4, v[u]), hd, a.H);
          const float ds = expf(sc - L) * (dv - dl);
          dq += ds * k[u];
        }
      }
    }
  }
  if (on) {
    reinterpret_cast<f32x4*>(a.dq + i * a.ld_dq)[lane] = dq;
    if (lane % lph == 0) a.delta[i * a.ld_delta + hd] = dl;
  }
}

// ---- source-major backward over one relation hop's transpose: dkv ----------------------------------------------------------------
struct hgt_src_args {
  const int* row_ptr_t;
  const int* col_t;           // destination row of every entry
  int64_t n_src;
  int H, C;
  const float* kv;
  int64_t ldkv;
  const float* q;
  int64_t ldq;
  const float* dagg;
  int64_t ld_dagg;
  const float* lse;
  int64_t ld_lse;
  const float* delta;
  int64_t ld_delta;
  float* dkv;                 // [n_src, ld_dkv], every row written
  int64_t ld_dkv;
};

template <int LPH>
__global__ void __launch_bounds__(kThreads) hgt_bwd_src_kernel(hgt_src_args a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * kHgtBwdRows + wave;
  if (j >= a.n_src) return;                        // (the whole wave)
  const int C4 = a.C / 4, lph = C4 / a.H;
  const bool on = lane < C4;
  const int hd = lane / lph;
  f32x4 k4 = {0.f, 0.f, 0.f, 0.f}, v4 = k4, dk = k4, dv4 = k4;
  const int s = a.row_ptr_t[j], t = a.row_ptr_t[j + 1];
  if (on && s < t) {
    const f32x4* row = reinterpret_cast<const f32x4*>(a.kv + j * a.ldkv);
    k4 = row[lane];
    v4 = row[C4 + lane];
  }
  for (int e0 = s; e0 < t; e0 += kHgtEdges) {
    f32x4 qi[kHgtEdges], gi[kHgtEdges];
    float Li[kHgtEdges], di[kHgtEdges];
#pragma unroll
    for (int u = 0; u < kHgtEdges; ++u) {
      qi[u] = gi[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      Li[u] = di[u] = 0.f;
      if (e0 + u < t && on) {
        const int64_t i = a.col_t[e0 + u];
        qi[u] = reinterpret_cast<const f32x4*>(a.q + i * a.ldq)[lane];
        gi[u] = reinterpret_cast<const f32x4*>(a.dagg + i * a.ld_dagg)[lane];
        Li[u] = a.lse[i * a.ld_lse + hd];
        di[u] = a.delta[i * a.ld_delta + hd];
      }
    }
#pragma unroll
    for (int u = 0; u < kHgtEdges; ++u) {
      if (e0 + u < t) {                            // (the whole wave)
        const float sc = head_sum<LPH>(dot4(qi[u], k4), hd, a.H);
        const float dv = head_sum<LPH>(dot4(gi[u], v4), hd, a.H);
        const float al = expf(sc - Li[u]);
        dk  += (al * (dv - di[u])) * qi[u];
        dv4 += al * gi[u];
      }
    }
  }
  if (on) {
    f32x4* row = reinterpret_cast<f32x4*>(a.dkv + j * a.ld_dkv);
    row[lane] = dk;
    row[C4 + lane] = dv4;
  }
}

void hgt_require_shape(int H, int C, int n_rel)
{
  if (!wgamd_hgt_layer_supported(H, C, n_rel))
    throw logic_error(fmt("unsupported shape: H=%d (1 .. %d), C=%d (<= %d, a multiple of H with C / H a multiple of 4), %d relations "
                          "(<= %d)", H, kMaxH, C, kHgtMaxC, n_rel, kHgtMaxRel));
}

// the relation descriptors of a launch, checked, into rel[]
void hgt_take_relations(wgamd_hgt_relation_t (&rel)[kHgtMaxRel], const wgamd_hgt_relation_t* rels, int n_rel, int C)
{
  WG_REQUIRE_INPUT(n_rel == 0 || rels != nullptr, "null pointer");
  for (int r = 0; r < n_rel; ++r) {
    WG_REQUIRE_INPUT(rels[r].row_ptr && rels[r].col && rels[r].kv, "null pointer");
    WG_REQUIRE_INPUT(rels[r].ldkv >= 2 * C, "leading dimension too small");
    if (!aligned_rows(rels[r].kv, rels[r].ldkv)) throw logic_error("kv rows must be 16-B aligned");
    rel[r] = rels[r];
  }
}

unsigned hgt_bwd_grid(int64_t rows)
{
  const int64_t blocks = (rows + kHgtBwdRows - 1) / kHgtBwdRows;
  WG_REQUIRE_INPUT(blocks <= INT32_MAX, "too many rows for one launch");
  return (unsigned)blocks;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_hgt_layer_supported(int H, int C, int n_rel)
{
  using namespace wgamd;
  return H >= 1 && H <= kMaxH && C >= 4 && C <= kHgtMaxC && C % H == 0 && (C / H) % 4 == 0 && n_rel >= 0 && n_rel <= kHgtMaxRel;
}

extern "C" wholememory_error_code_t wgamd_hgt_layer_f32(
    const wgamd_hgt_relation_t* rels, int n_rel, int64_t n_rows, int H, int C, const float* q, int64_t ldq, const float* w_out,
    int64_t ldw, const float* b_out, const float* skip, const float* x_dst, int64_t ldx_dst, const int64_t* dst_rows,
    const void* dst_ids, int dst_ids_kind, int flags, const int64_t* out_rows, float* out, int64_t ldo, float* agg_out, int64_t ld_agg,
    float* lse_out, int64_t ld_lse, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_hgt_layer_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    hgt_require_shape(H, C, n_rel);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(q && w_out && out, "null pointer");
    WG_REQUIRE_INPUT(ldq >= C && ldw >= C && ldo >= C && (agg_out == nullptr || ld_agg >= C) && (lse_out == nullptr || ld_lse >= H),
                     "leading dimension too small");
    WG_REQUIRE_INPUT((skip == nullptr) == (x_dst == nullptr), "skip and x_dst come together (the gate), or neither");
    hgt_args a{};
    hgt_take_relations(a.rel, rels, n_rel, C);
    if (x_dst) {
      WG_REQUIRE_INPUT(ldx_dst >= C, "leading dimension too small");
      WG_REQUIRE_INPUT(dst_ids_kind >= 0 && dst_ids_kind <= 2 && (dst_ids_kind == 0) == (dst_ids == nullptr), "bad node list kind");
    }
    if (!aligned_rows(q, ldq) || !aligned_rows(w_out, ldw) || !aligned_rows(out, ldo) || (x_dst && !aligned_rows(x_dst, ldx_dst)) ||
        (agg_out && !aligned_rows(agg_out, ld_agg)))
      throw logic_error("q / w_out / out / x_dst / agg_out rows must be 16-B aligned");
    a.n_rel = n_rel, a.H = H, a.C = C, a.n_rows = n_rows, a.q = q, a.ldq = ldq, a.wo = w_out, a.ldwo = ldw, a.bo = b_out;
    a.skip = skip, a.x_dst = x_dst, a.ldx_dst = ldx_dst, a.dst_rows = dst_rows, a.dst_ids = dst_ids, a.dst_kind = dst_ids_kind;
    a.relu = (flags & WGAMD_HGT_RELU) != 0, a.out_rows = out_rows, a.out = out, a.ldo = ldo;
    a.agg_out = agg_out, a.ld_agg = ld_agg, a.lse_out = lse_out, a.ld_lse = ld_lse;
    tile_geometry(C, a.C16, a.SD);
    const dim3 grid((unsigned)((n_rows + kTileRows - 1) / kTileRows));
    const size_t lds = (size_t)2 * kTileRows * a.SD * 4;      // two tiles of at most 16 x 260 floats: 33 KB
    auto st = static_cast<hipStream_t>(stream);
    with_head_lanes(C / H, [&](auto lph) { hgt_layer_kernel<decltype(lph)::value><<<grid, kThreads, lds, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_hgt_bwd_dst_f32(
    const wgamd_hgt_relation_t* rels, int n_rel, int64_t n_rows, int H, int C, const float* q, int64_t ldq, const float* dagg,
    int64_t ld_dagg, const float* agg, int64_t ld_agg, const float* lse, int64_t ld_lse, float* dq, int64_t ld_dq, float* delta,
    int64_t ld_delta, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_hgt_bwd_dst_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    hgt_require_shape(H, C, n_rel);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(q && dagg && agg && lse && dq && delta, "null pointer");
    WG_REQUIRE_INPUT(ldq >= C && ld_dagg >= C && ld_agg >= C && ld_dq >= C && ld_lse >= H && ld_delta >= H, "leading dimension too small");
    if (!aligned_rows(q, ldq) || !aligned_rows(dagg, ld_dagg) || !aligned_rows(agg, ld_agg) || !aligned_rows(dq, ld_dq))
      throw logic_error("q / dagg / agg / dq rows must be 16-B aligned");
    hgt_bwd_args a{};
    hgt_take_relations(a.rel, rels, n_rel, C);
    a.n_rel = n_rel, a.H = H, a.C = C, a.n_rows = n_rows, a.q = q, a.ldq = ldq, a.dagg = dagg, a.ld_dagg = ld_dagg;
    a.agg = agg, a.ld_agg = ld_agg, a.lse = lse, a.ld_lse = ld_lse, a.dq = dq, a.ld_dq = ld_dq, a.delta = delta, a.ld_delta = ld_delta;
    const dim3 grid(hgt_bwd_grid(n_rows));
    auto st = static_cast<hipStream_t>(stream);
    with_head_lanes(C / H, [&](auto lph) { hgt_bwd_dst_kernel<decltype(lph)::value><<<grid, kThreads, 0, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_hgt_bwd_src_f32(
    const int* row_ptr_t, const int* col_t, int64_t n_src, int H, int C, const float* kv, int64_t ldkv, const float* q, int64_t ldq,
    const float* dagg, int64_t ld_dagg, const float* lse, int64_t ld_lse, const float* delta, int64_t ld_delta, float* dkv,
    int64_t ld_dkv, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_hgt_bwd_src_f32", [&] {
    WG_REQUIRE_INPUT(n_src >= 0, "bad sizes");
    hgt_require_shape(H, C, 1);
    if (n_src == 0) return;
    WG_REQUIRE_INPUT(row_ptr_t && col_t && kv && q && dagg && lse && delta && dkv, "null pointer");
    WG_REQUIRE_INPUT(ldkv >= 2 * C && ld_dkv >= 2 * C && ldq >= C && ld_dagg >= C && ld_lse >= H && ld_delta >= H,
                     "leading dimension too small");
    if (!aligned_rows(kv, ldkv) || !aligned_rows(dkv, ld_dkv) || !aligned_rows(q, ldq) || !aligned_rows(dagg, ld_dagg))
      throw logic_error("kv / dkv / q / dagg rows must be 16-B aligned");
    hgt_src_args a{};
    a.row_ptr_t = row_ptr_t, a.col_t = col_t, a.n_src = n_src, a.H = H, a.C = C, a.kv = kv, a.ldkv = ldkv, a.q = q, a.ldq = ldq;
    a.dagg = dagg, a.ld_dagg = ld_dagg, a.lse = lse, a.ld_lse = ld_lse, a.delta = delta, a.ld_delta = ld_delta;
    a.dkv = dkv, a.ld_dkv = ld_dkv;
    const dim3 grid(hgt_bwd_grid(n_src));
    auto st = static_cast<hipStream_t>(stream);
    with_head_lanes(C / H, [&](auto lph) { hgt_bwd_src_kernel<decltype(lph)::value><<<grid, kThreads, 0, st>>>(a); });
    WG_HIP_CHECK(hipGetLastError());
  });
}
