/*
 * wgamd_ext.h — entry points that have NO counterpart in libwholegraph's C ABI.
 *
 * (1) Mini-batch aggregation.  The reference ships no SpMM/SDDMM kernel: its models call
 *     torch_geometric.nn.SAGEConv / GATConv (third party; call sites
 *     /root/reference/python/pylibwholegraph/pylibwholegraph/torch/gnn_model.py:25-59,119-125,178-199).
 *     These entry points are what a PyTorch-ROCm autograd.Function binds to get the same maths
 *     (PyG formulas, fp32) from hand-written gfx950 kernels over the sampler's per-hop CSR
 *     (row_ptr = sample offsets, col = raw_to_unique mapping; graph_structure.py:186-195).
 * (2) A no-host-sync variant of the sampling + renumbering walk for the loader's steady state:
 *     same results as chaining the wgamd_ops.h ops, but every size stays on the device and
 *     outputs go to caller-provided capacity buffers, so a whole multi-hop mini-batch is a
 *     fixed sequence of launches (hipGraph-capturable) with no D2H round trip per op
 *     (the reference pays >= 5 stream syncs per hop).
 *
 * Plain pointers and sizes only; all pointers are device pointers unless stated; `stream` is a
 * hipStream_t passed as void*.  All calls are asynchronous on `stream`.
 */
#ifndef WGAMD_EXT_H_
#define WGAMD_EXT_H_

#include "wgamd_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) aggregation -------------------------------------------------------------------- */

/* out[i, 0:F] = REDUCE_{e in [row_ptr[i], row_ptr[i+1])} x[src(e), 0:F]
 *   src(e) = col[e]                      when src_ids == NULL
 *          = src_ids[col[e]]             otherwise (fused feature fetch: x is then the global
 *                                        feature table and src_ids the batch's local->global map;
 *                                        src_ids_dtype = WHOLEMEMORY_DT_INT | WHOLEMEMORY_DT_INT64)
 *   REDUCE = sum (mean == 0) or sum / max(deg_i, 1) (mean != 0).  fp32, summed in CSR order.
 * row_ptr int32[n_rows+1], col int32[nnz]; ldx / ldo = row strides in elements. */
wholememory_error_code_t wgamd_spmm_csr_f32(const int* row_ptr,
                                            const int* col,
                                            int64_t n_rows,
                                            const float* x,
                                            int64_t ldx,
                                            int F,
                                            const void* src_ids,
                                            wholememory_dtype_t src_ids_dtype,
                                            int mean,
                                            float* out,
                                            int64_t ldo,
                                            void* stream);

/* SAGEConv input builder: the mean (or sum) aggregate AND the root term side by side, so that
 *   lin_l(mean_j x_j) + lin_r(x_i)  is ONE dense GEMM  [agg | x_self] @ [W_l | W_r]^T :
 *   out[i, 0:F]  = REDUCE_{e in row i} x[col[e], :]
 *   out[i, F:2F] = x[self_rows[i], :]
 * self_rows int64[n_rows] = row of destination i inside x (i itself for a single mini-batch, the
 * block-diagonal row for a call group); ldo >= 2F. */
wholememory_error_code_t wgamd_sage_aggregate_f32(const int* row_ptr,
                                                  const int* col,
                                                  int64_t n_rows,
                                                  const float* x,
                                                  int64_t ldx,
                                                  int F,
                                                  const int64_t* self_rows,
                                                  int mean,
                                                  float* out,
                                                  int64_t ldo,
                                                  void* stream);

/* The same with the FEATURE FETCH fused in: `table` is the global feature table and src_ids the mini-batch's
 * local -> global map (INT|INT64), so the batch feature matrix x = table[src_ids] is never materialised:
 *   out[i, 0:F]  = REDUCE_e table[src_ids[col[e]], :]      out[i, F:2F] = table[src_ids[self_rows[i]], :] */
wholememory_error_code_t wgamd_sage_aggregate_fetch_f32(const int* row_ptr,
                                                        const int* col,
                                                        int64_t n_rows,
                                                        const float* table,
                                                        int64_t ldt,
                                                        int F,
                                                        const void* src_ids,
                                                        wholememory_dtype_t src_ids_dtype,
                                                        const int64_t* self_rows,
                                                        int mean,
                                                        float* out,
                                                        int64_t ldo,
                                                        void* stream);

/* Sum aggregation over a CSR whose rows may be very long — the TRANSPOSED sampled hop of the backward pass, where a hub
 * source is a neighbour of thousands of rows.  Rows are summed in pieces of 64 entries by different lane groups and the
 * pieces of a row are then added up in order: same values from run to run (no atomics on the data), no launch that lasts as
 * long as its longest row.  out[r, :] = sum_{e in row r} x[col[e], :].  Workspace: wgamd_spmm_csr_segmented_workspace_bytes
 * (n_entries = row_ptr[n_rows], known to the caller). */
size_t wgamd_spmm_csr_segmented_workspace_bytes(int64_t n_entries, int F);
wholememory_error_code_t wgamd_spmm_csr_segmented_f32(const int* row_ptr, const int* col, int64_t n_rows, int64_t n_entries,
                                                      const float* x, int64_t ldx, int F, float* out, int64_t ldo,
                                                      void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the above w.r.t. x (src_ids == NULL form):
 *   grad_x[col[e], :] += grad_out[i, :] * (mean ? 1/max(deg_i,1) : 1)   for every edge e of row i.
 * grad_x must be zero-initialised (or hold the gradient to accumulate into) by the caller. */
wholememory_error_code_t wgamd_spmm_csr_bwd_f32(const int* row_ptr,
                                                const int* col,
                                                int64_t n_rows,
                                                const float* grad_out,
                                                int64_t ldg,
                                                int F,
                                                int mean,
                                                float* grad_x,
                                                int64_t ldx,
                                                void* stream);

/* Transpose of a sampled-hop CSR (rows = destinations, col = source rows in [0, n_src)) for the atomic-free backward
 * passes: the edges sorted by source, STABLE (edge order inside a source = edge order of the hop, so gradient sums are
 * reproducible).  One radix sort of (source, edge) pairs over ceil(log2 n_src) bits + two small kernels.
 *   row_ptr_t [n_src + 1]  : CSR offsets over the sources
 *   edge_perm [n_edges]    : edge ids in source-major order                      (may be NULL)
 *   edge_dst  [n_edges]    : destination row of every ORIGINAL edge id           (may be NULL)
 *   col_t     [n_edges]    : destination row of the k-th source-major edge = edge_dst[edge_perm[k]]   (may be NULL)
 * workspace: wgamd_csr_transpose_workspace_bytes(n_edges, n_src) bytes of device scratch. */
size_t wgamd_csr_transpose_workspace_bytes(int64_t n_edges, int64_t n_src);
wholememory_error_code_t wgamd_csr_transpose_i32(const int* row_ptr,
                                                 const int* col,
                                                 int64_t n_rows,
                                                 int64_t n_edges,
                                                 int64_t n_src,
                                                 int* row_ptr_t,
                                                 int* edge_perm,
                                                 int* edge_dst,
                                                 int* col_t,
                                                 void* workspace,
                                                 size_t workspace_bytes,
                                                 void* stream);

/* PyG COO edge_index (src, dst int64; dst ids in [0, n_dst)) -> destination-major int32 CSR for the aggregation kernels:
 * stable radix sort of (dst, edge) over ceil(log2 n_dst) bits, row_ptr [n_dst + 1] from the run boundaries,
 * col[k] = src of the k-th destination-major edge, edge_perm (may be NULL) = the edge ids in that order. */
size_t wgamd_coo_to_csr_workspace_bytes(int64_t n_edges, int64_t n_dst);
wholememory_error_code_t wgamd_coo_to_csr_i64(const int64_t* src,
                                              const int64_t* dst,
                                              int64_t n_edges,
                                              int64_t n_dst,
                                              int* row_ptr,
                                              int* col,
                                              int* edge_perm,
                                              void* workspace,
                                              size_t workspace_bytes,
                                              void* stream);

/* GATConv message passing (edge-softmax SDDMM + weighted SpMM), H heads x C channels:
 *   s_e      = leaky_relu(a_src[col[e], h] + a_dst[i, h], negative_slope)
 *   alpha_e  = softmax over the edges e of row i (per head)
 *   out[i,h,:] = sum_e alpha_e * x[col[e], h, :]
 * x [N_src, H*C] (row stride ldx), a_src [N_src, H], a_dst [n_rows, H], out [n_rows, H*C]
 * (row stride ldo), alpha_out nullable [nnz, H].  Rows without edges produce zeros. */
wholememory_error_code_t wgamd_gat_csr_f32(const int* row_ptr,
                                           const int* col,
                                           int64_t n_rows,
                                           const float* x,
                                           int64_t ldx,
                                           const float* a_src,
                                           const float* a_dst,
                                           int H,
                                           int C,
                                           float negative_slope,
                                           float* alpha_out,
                                           float* out,
                                           int64_t ldo,
                                           void* stream);

/* ---- (2) no-sync sampling walk ---------------------------------------------------------- */

/* One hop of uniform sampling + renumbering with device-resident sizes.
 *   in : targets (INT|INT64 = id_dtype)[<= target_cap], *n_targets_dev = how many are valid
 *   out: offsets int32[target_cap+1]   exclusive scan of min(deg, M); entries past n_targets
 *                                      repeat the total
 *        neighbor_lid int32[edge_cap]  raw_to_unique mapping of every sampled edge (CSR col)
 *        center_lid  int32[edge_cap]   row index of every sampled edge (nullable)
 *        edge_gid    int64[edge_cap]   CSR position of every sampled edge (nullable)
 *        unique      (id_dtype)[target_cap + edge_cap]  targets ++ new nodes (first appearance),
 *                                        capacity slack padded with -1 (a gather skips it)
 *        counts_dev  int32[2]          {n_edges, n_unique}
 * edge_cap must be >= target_cap * M (M > 0 required).  Results are identical to
 * wholegraph_csr_unweighted_sample_without_replacement followed by graph_append_unique.
 * workspace: wgamd_sample_hop_workspace_bytes(target_cap, edge_cap, id_dtype) bytes. */
size_t wgamd_sample_hop_workspace_bytes(int64_t target_cap, int64_t edge_cap, wholememory_dtype_t id_dtype);
size_t wgamd_sample_hop_weighted_workspace_bytes(int64_t target_cap, int64_t edge_cap, wholememory_dtype_t id_dtype,
                                                 int64_t max_row_len);

wholememory_error_code_t wgamd_sample_hop_nosync(const int64_t* csr_row_ptr,
                                                 const void* csr_col,
                                                 wholememory_dtype_t id_dtype,
                                                 const void* targets,
                                                 const int* n_targets_dev,
                                                 int64_t target_cap,
                                                 int max_sample_count,
                                                 unsigned long long random_seed,
                                                 int* offsets,
                                                 int* neighbor_lid,
                                                 int* center_lid,
                                                 int64_t* edge_gid,
                                                 int64_t edge_cap,
                                                 void* unique,
                                                 int* counts_dev,
                                                 void* workspace,
                                                 size_t workspace_bytes,
                                                 void* stream);

/* The same hop for a CALL GROUP of n_batches mini-batches handled by one launch sequence (the
 * idea of cugraph_pyg's local_seeds_per_call,
 * /root/reference/python/cugraph-pyg/cugraph_pyg/sampler/distributed_sampler.py:279-343): every
 * launch carries G x the work, every mini-batch gets exactly the result a single-batch call with
 * its own seed would produce (its PCG streams are numbered from the start of its own segment and
 * it is renumbered on its own).
 *   in : targets        concatenation of the batches' targets, batch b = [target_seg[b], target_seg[b+1])
 *        target_batch   int32[target_cap]  batch of every target
 *        target_seg     int32[n_batches+1] (device); target_seg[n_batches] = live target count
 *        random_seeds_dev u64[n_batches]   (device) one sampling seed per mini-batch
 *   out: offsets        int32[target_cap+1] global CSR row_ptr over all targets
 *        neighbor_row   int32[edge_cap]  GLOBAL row (into `unique`) of every sampled edge's neighbour;
 *                                        the per-batch local id is neighbor_row - unique_seg[b]
 *        center_row     int32[edge_cap]  global target row of every sampled edge (required)
 *        unique         ids[target_cap+edge_cap]  per-batch unique lists, concatenated: batch b =
 *                                        [unique_seg[b], unique_seg[b+1]) = its targets ++ its new nodes;
 *                                        slack padded with -1 (see WGAMD_HOP_NO_UNIQUE_PAD)
 *        unique_batch   int32[target_cap+edge_cap], unique_seg int32[n_batches+1]:
 *                                        feed them back as target_batch / target_seg of the next hop
 *        counts_dev     int32[2] {n_edges, n_unique}
 * Workspace as for the single-batch hop. */
wholememory_error_code_t wgamd_sample_hop_batched_nosync(const int64_t* csr_row_ptr,
                                                         const void* csr_col,
                                                         wholememory_dtype_t id_dtype,
                                                         const void* targets,
                                                         const int* target_batch,
                                                         const int* target_seg,
                                                         int n_batches,
                                                         int64_t target_cap,
                                                         int max_sample_count,
                                                         const unsigned long long* random_seeds_dev,
                                                         int* offsets,
                                                         int* neighbor_row,
                                                         int* center_row,
                                                         int64_t* edge_gid,
                                                         int64_t edge_cap,
                                                         void* unique,
                                                         int* unique_batch,
                                                         int* unique_seg,
                                                         int* counts_dev,
                                                         void* workspace,
                                                         size_t workspace_bytes,
                                                         int64_t n_vertices /* ids are < n_vertices; 0 = unknown.  A bound
                                                           lets the renumber table pack (batch, id, first position) into
                                                           one 64-bit word per slot (one atomic per key instead of two) */,
                                                         void* stream);

/* Flags of the call-group hops.  WGAMD_HOP_NO_UNIQUE_PAD: do not write the -1 padding into the capacity slack of
 * `unique` / `nodes_out` — for callers that read counts_dev / unique_seg (host or device) and never look past the live end.
 * The capacity is the worst case (every seed with fan-out^hops distinct neighbours), 3-4x the live size on real graphs, so
 * the padding is most of what the renumber step writes: walk 1.18 -> 1.09 ms per call group of 191 on the products-like graph.
 * Everything below the live end is identical with and without the flag. */
#define WGAMD_HOP_NO_UNIQUE_PAD 1u
/* WGAMD_HOP_COL_INT32: `csr_col` holds INT (32-bit) entries although id_dtype is WHOLEMEMORY_DT_INT64 — a graph with fewer
 * than 2^31 vertices kept compact behind an INT64 API (needs 0 < n_vertices < 2^31).  Targets, `unique` and the frontier
 * lists stay INT64; the sampled neighbours travel through the hop as 32-bit values (half the sector footprint of the
 * sampler's random column picks, half the bytes of every renumber pass) and are widened where `unique` is written.  Same
 * results as the INT64 column array, bit for bit.  In the _ex entry point `unique_batch` may be NULL (not produced). */
#define WGAMD_HOP_COL_INT32 2u
/* WGAMD_HOP_UNIFORM_BATCHES: the caller promises that every mini-batch of the call group started from the same number of
 * seeds, so that no batch samples more than ceil(edge_cap / n_batches) edges in this hop.  Where a batch's first-occurrence
 * bits and their running counts for that many edges (12 bytes per 64) fit a workgroup's LDS, the renumbering resolves the
 * first-appearance ranks per batch in LDS instead of over the whole edge array (three launches per hop instead of six).
 * Same results, bit for bit; without the flag, or where the window does not fit, the hop runs as before.  A broken promise
 * writes nothing out of bounds: the hop then publishes counts_dev = {n_edges, -1} and leaves its other outputs unwritten.
 * (Bit value 4 is not assigned and is refused like any unknown bit.) */
#define WGAMD_HOP_UNIFORM_BATCHES 8u

wholememory_error_code_t wgamd_sample_hop_batched_nosync_ex(const int64_t* csr_row_ptr,
                                                         const void* csr_col,
                                                         wholememory_dtype_t id_dtype,
                                                         const void* targets,
                                                         const int* target_batch,
                                                         const int* target_seg,
                                                         int n_batches,
                                                         int64_t target_cap,
                                                         int max_sample_count,
                                                         const unsigned long long* random_seeds_dev,
                                                         int* offsets,
                                                         int* neighbor_row,
                                                         int* center_row,
                                                         int64_t* edge_gid,
                                                         int64_t edge_cap,
                                                         void* unique,
                                                         int* unique_batch,
                                                         int* unique_seg,
                                                         int* counts_dev,
                                                         void* workspace,
                                                         size_t workspace_bytes,
                                                         int64_t n_vertices /* ids are < n_vertices; 0 = unknown.  A bound
                                                           lets the renumber table pack (batch, id, first position) into
                                                           one 64-bit word per slot (one atomic per key instead of two) */,
                                                         unsigned flags,
                                                         void* stream);

/* One hop of the PyG-style walk for a call group — what cugraph_pyg's sampling call produces
 * (pylibcugraph.*_neighbor_sample(renumber=True, prior_sources_behavior="exclude",
 * deduplicate_sources=True, retain_seeds=True); call site
 * /root/reference/python/cugraph-pyg/cugraph_pyg/sampler/distributed_sampler.py:877-908): hop k expands only
 * the vertices FIRST SEEN by hop k-1 (the frontier), and renumbers the sampled neighbours against ALL
 * vertices of the mini-batch so far.  Same kernels as the WholeGraph-style hop; per mini-batch the
 * result equals chaining wholegraph_csr_unweighted_sample_without_replacement(frontier) and
 * graph_append_unique(nodes, neighbours) with that batch's seed.
 *   nodes / node_batch / node_seg        per-batch vertex lists so far, concatenated (batch b =
 *                                        [node_seg[b], node_seg[b+1]); node_seg[G] = live count)
 *   frontier / _batch / _seg / _local0   the vertices to expand, by batch; local0[b] = local id (inside
 *                                        batch b) of its first frontier vertex
 *   offsets           int32[frontier_cap+1]  CSR row_ptr over the frontier
 *   neighbor_local / center_local  int32[edge_cap]  per-batch LOCAL ids of both ends of every sampled edge
 *                                        (PyG: row = neighbor_local, col = center_local)
 *   edge_gid          int64[edge_cap] CSR slot of every sampled edge (nullable)
 *   nodes_out / _batch / _seg            the grown per-batch lists (input lists ++ new vertices), slack = -1
 *   frontier_out / _batch / _seg / _local0   the next hop's frontier (= vertices first seen now)
 *   counts_dev        int32[2] {n_edges, n_nodes_out}
 *   neighbor_row_scratch / center_row_scratch int32[edge_cap] scratch
 * Capacities: edge_cap >= frontier_cap * M; nodes_out holds node_cap + edge_cap entries.
 * Workspace: wgamd_sample_hop_workspace_bytes(max(node_cap, frontier_cap), edge_cap, id_dtype). */
typedef struct wgamd_pyg_hop_t {
  const int64_t* csr_row_ptr;
  const void* csr_col;
  wholememory_dtype_t id_dtype;
  int n_batches;
  int max_sample_count;
  const unsigned long long* random_seeds_dev;
  const void* nodes;
  const int* node_batch;
  const int* node_seg;
  int64_t node_cap;
  const void* frontier;
  const int* frontier_batch;
  const int* frontier_seg;
  const int* frontier_local0;
  int64_t frontier_cap;
  int* offsets;
  int* neighbor_local;
  int* center_local;
  int64_t* edge_gid;
  int64_t edge_cap;
  void* nodes_out;
  int* nodes_out_batch;
  int* nodes_out_seg;
  void* frontier_out;
  int* frontier_out_batch;
  int* frontier_out_seg;
  int* frontier_out_local0;
  int* counts_dev;
  int* neighbor_row_scratch;
  int* center_row_scratch;
  void* workspace;
  size_t workspace_bytes;
  /* biased hop (NULL = uniform): weight of every CSR slot, FLOAT | DOUBLE; fan-out <= 256; max_row_len = the graph's
   * maximum degree (sizes the key slabs); workspace then = wgamd_sample_hop_weighted_workspace_bytes(...).  Rows with at
   * most max_sample_count candidates are copied whole, zero-weight edges included (the reference's kernel does the same:
   * weighted_sample_without_replacement_func.cuh:592-647).  Same results as
   * wholegraph_csr_weighted_sample_without_replacement + graph_append_unique per mini-batch. */
  const void* csr_weight;
  wholememory_dtype_t weight_dtype;
  int64_t max_row_len;
  int64_t n_vertices; /* ids are < n_vertices (0 = unknown): enables the packed renumber table, see above */
  unsigned flags;     /* WGAMD_HOP_* bits, 0 = defaults */
} wgamd_pyg_hop_t;

wholememory_error_code_t wgamd_sample_hop_pyg_nosync(const wgamd_pyg_hop_t* p, void* stream);

/* The TEMPORAL hop of the PyG-style walk for a call group: wgamd_sample_hop_pyg_nosync restricted to the CSR slots whose
 * time qualifies against the time their frontier vertex was reached at.  `p` is the block of the plain hop (its layout is
 * unchanged), `t` the times:
 *   csr_time          int64 per CSR slot
 *   frontier_time     int64[frontier_cap]  time every frontier entry was reached at (hop 0: the seeds' input time)
 *   frontier_time_out int64[edge_cap]      time of every entry of frontier_out = time of the FIRST sampled edge (lowest
 *                                          position in the hop's edge list) that reached it: the next hop's frontier_time
 *   comparison        slot s of a row reached at t_v qualifies when
 *                       1 strictly increasing  time[s] >  t_v      2 monotonically increasing  time[s] >= t_v
 *                       3 strictly decreasing  time[s] <  t_v      4 monotonically decreasing  time[s] <= t_v
 * and, with p->csr_weight, when its weight rounded to float is > 0.  Per row: A-Res over the whole row on the key stream of
 * the biased hop with the effective weight (the weight, or 1.0f when p->csr_weight is NULL = uniform temporal, of a
 * qualifying slot; 0 otherwise) — every slot consumes its draws —, the picks that do not qualify dropped, the others in CSR
 * order: min(qualifying slots, max_sample_count) edges.  Renumbering as in the plain hop, over the surviving edges.  Per
 * mini-batch the result equals the biased ABI op over an array of effective weights + graph_append_unique.
 * Needs 0 < max_sample_count <= 256, max_row_len > 0 (the graph's maximum degree), edge_gid; workspace:
 * wgamd_sample_hop_temporal_workspace_bytes(max(node_cap, frontier_cap), edge_cap, id_dtype, max_row_len).  A bad block is
 * WHOLEMEMORY_INVALID_INPUT before anything touches the device. */
typedef struct wgamd_pyg_hop_time_t {
  const int64_t* csr_time;
  const int64_t* frontier_time;
  int64_t* frontier_time_out;
  int comparison;
} wgamd_pyg_hop_time_t;
size_t wgamd_sample_hop_temporal_workspace_bytes(int64_t target_cap, int64_t edge_cap, wholememory_dtype_t id_dtype,
                                                 int64_t max_row_len);
wholememory_error_code_t wgamd_sample_hop_pyg_temporal_nosync(const wgamd_pyg_hop_t* p, const wgamd_pyg_hop_time_t* t,
                                                              void* stream);

/* Rows of the hop's targets inside its block-diagonal `unique` list — the "x[:num_dst]" of a single mini-batch becomes
 * an index list for a call group:  rows[i] = i + unique_seg[b] - target_seg[b],  b = target_batch[i],  for i < n_targets.
 * One launch (the SAGEConv root term and the next layer's row list read it); everything is device memory. */
wholememory_error_code_t wgamd_call_group_target_rows(const int* unique_seg, const int* target_seg, const int* target_batch,
                                                      int64_t n_targets, int64_t* rows, void* stream);

/* Frontier of a node type between two hops of a heterogeneous call-group walk: batch b (of n_batches <= 4095) gained the
 * vertices [begin[b], seg[b+1] - seg[b]) of its batch-major list `nodes` (n_nodes entries, offsets seg [n_batches + 1]) since
 * the previous hop.  Writes them batch-major into ids[capacity] with their batch[capacity] and the offsets f_seg [n_batches + 1];
 * slots past f_seg[n_batches] are padding no consumer reads.  (The per-hop frontier the reference's distributed sampler keeps
 * per batch, python/cugraph-pyg/cugraph_pyg/sampler/distributed_sampler.py:808-824, for a whole call group.) */
wholememory_error_code_t wgamd_frontier_list(const int64_t* nodes, int64_t n_nodes, const int* seg, const int* begin, int n_batches,
                                             int64_t capacity, int64_t* ids, int* batch, int* f_seg, void* stream);

/* Reach times of a node type's batch-major list across one TEMPORAL call of a heterogeneous call-group walk
 * (csrc/wg_reach_time.hip).  The call appended to the list `nodes` (offsets node_seg [n_batches + 1], times time_in
 * [time_in_cap], parallel to it) and left nodes_out: per batch the old list, then the vertices first seen by this call in
 * first-appearance order (offsets nodes_out_seg, batch of every entry nodes_out_batch), whose times are the call's
 * frontier_time_out (offsets frontier_out_seg).  For entry i of batch b at position l = i - nodes_out_seg[b], with
 * n_old = node_seg[b + 1] - node_seg[b]:
 *   time_out[i] = l < n_old ? time_in[node_seg[b] + l] : frontier_time_out[frontier_out_seg[b] + l - n_old]
 * for i < min(nodes_out_seg[n_batches], capacity).  One launch, a thread per entry, no atomics, every size read from the
 * device; a source index outside its capacity (time_in_cap / frontier_cap) or a batch outside [0, n_batches) writes nothing.
 * time_in may be NULL when time_in_cap is 0 (a type that had no vertices yet). */
wholememory_error_code_t wgamd_reach_time_append(const int64_t* time_in, int64_t time_in_cap, const int* node_seg,
                                                 const int64_t* frontier_time_out, int64_t frontier_cap,
                                                 const int* frontier_out_seg, const int* nodes_out_batch,
                                                 const int* nodes_out_seg, int n_batches, int64_t capacity, int64_t* time_out,
                                                 void* stream);

/* One (hop, edge type) of a heterogeneous call group (wgamd_sample_hop_pyg_nosync outputs) in the form the layers consume:
 * dst_full[j] / dst_compact[j] = row of frontier entry j in the destination type's batch-major node list — all vertices of
 * the walk (segments seg_dst [G+1]) / the vertices discovered by hops 0-1 only (compact_seg_dst [G+1], int64; NULL with
 * dst_compact NULL) — and col_full[e] / col_compact[e] = row of edge e's source in the source type's list, the same two ways
 * (row_local = the hop's `neighbor_local`).  Entry j of batch b has local id frontier_local0[b] + (j - frontier_seg[b]). */
wholememory_error_code_t wgamd_call_group_hop_rows(const int* offsets, const int* frontier_batch, const int* frontier_seg,
                                                   const int* frontier_local0, const int* row_local, int64_t n_frontier,
                                                   const int* seg_dst, const int64_t* compact_seg_dst, const int* seg_src,
                                                   const int64_t* compact_seg_src, int64_t* dst_full, int64_t* dst_compact,
                                                   int* col_full, int* col_compact, void* stream);
/* wgamd_call_group_hop_rows with the number of mini-batches given (frontier_seg has n_batches + 1 entries, the last =
 * n_frontier; the batch of an entry follows from it): one block per (batch, stretch of its frontier entries) reads the batch's
 * segment starts once and streams entries and edges with every lane — 3-4x faster at call-group sizes. */
wholememory_error_code_t wgamd_call_group_hop_rows_batched(const int* offsets, const int* frontier_seg, const int* frontier_local0,
                                                           const int* row_local, int64_t n_frontier, int n_batches,
                                                           const int* seg_dst, const int64_t* compact_seg_dst, const int* seg_src,
                                                           const int64_t* compact_seg_src, int64_t* dst_full, int64_t* dst_compact,
                                                           int* col_full, int* col_compact, void* stream);

/* ONE mini-batch of a PyG-style call group copied into fixed-size buffers (cugraph_pyg_amd.loader.PerBatchStep): the
 * reference's training loops step the optimizer once per mini-batch (pylibwholegraph/torch/gnn_model.py:119-125); with
 * every per-batch array at a fixed address and size the whole step can be captured in one hipGraph and replayed per
 * mini-batch.  For hop k (arrays of n_hops pointers): frontier entries [frontier_seg[k][batch], frontier_seg[k][batch + 1]) of
 * `offsets[k]` / `row_local[k]` (the hop's CSR over its frontier and the batch-local id of every sampled neighbour) become
 * row_ptr_out[k] (int32 [row_cap[k] + 1], from 0, row_ptr_out[k][row_cap[k]] = edge_cap[k]: the slack edges are dealt evenly
 * to the slack rows — at least one: a hop with row_cap[k] live rows overflows — with sources spread over the input rows, so
 * every entry of the fixed-size arrays is a well-formed edge of a row nobody reads), self_rows_out[k] (int64 [row_cap[k]]:
 * batch-local id of the entry = its row of x; 0 in the padding), col_out[k] (int32 [edge_cap[k]]: batch-local ids) and, when col_seg_out
 * is given, col_seg_out[k]: the same sources as rows of a trimmed layer's output, laid out as hop 0's row_cap[0] rows, then
 * hop 1's row_cap[1], ... .  n_id_out [node_cap] = the mini-batch's vertices (padding repeats the first).  sizes_out
 * (nullable, int32 [2 n_hops + 2]): live rows and edges per hop, live vertices, 1 if anything exceeded its capacity (the
 * copy is then truncated).  row_ptr_all_out (nullable, int32 [sum row_cap + 1]): the hops' CSRs back to back as ONE CSR — hop
 * k's rows start at sum(row_cap[:k]) and point at edges from sum(edge_cap[:k]); a caller that allocates the hops' col /
 * self_rows arrays back to back runs a layer over hops 0..j as one launch over a prefix of it; inv_deg_all_out (nullable, float
 * [sum row_cap]) = 1 / max(degree, 1) of every row of that CSR (what the backward of a mean aggregation scales by);
 * seed_mask_out (nullable, float [row_cap[0]]) = 1 for a live seed row, 0 for the padding (the row weights of the loss over the
 * last layer's row_cap[0] output rows: no slice, no mask arithmetic in the captured step).  One launch, no synchronisation. */
wholememory_error_code_t wgamd_call_group_stage_batch(int n_hops, const int* const* offsets, const int* const* row_local,
                                                      const int* const* frontier_seg, const int* const* frontier_local0,
                                                      const void* nodes, wholememory_dtype_t id_dtype, const int* node_seg,
                                                      int batch, const int* row_cap, const int* edge_cap, int node_cap,
                                                      int* const* row_ptr_out, int64_t* const* self_rows_out, int* const* col_out,
                                                      int* const* col_seg_out, void* n_id_out, int* sizes_out, int* row_ptr_all_out,
                                                      float* inv_deg_all_out, float* seed_mask_out, void* stream);

/* One hop of a PyG-style call group renumbered for the LAYER that consumes it (cugraph_pyg_amd.loader.CallGroup).  The
 * layer's input rows are `n_segments` segments per batch: local ids [local0[s][b], local0[s+1][b]) of batch b sit at rows
 * seg_base[s] + start[s][b] + (local id - local0[s][b]); seg_tab is int32 [2 n_segments, n_batches + 1] with row 2s =
 * local0[s], row 2s + 1 = start[s].  One segment whose start = the node-list offsets is the batch-major list of all
 * vertices (x = feat[n_id]); the output of a trimmed layer is one segment per hop it ran (that hop's frontier list).
 * Writes self_rows[j] (int64, nullable) = input row of frontier entry j itself (local id frontier_local0[b] + j -
 * frontier_seg[b]) and col[e] = input row of edge e's sampled neighbour (row_local[e] = the hop's `neighbor_local`).
 * frontier_seg has n_batches + 1 entries (the last = n_frontier); frontier_batch is not read (may be NULL). */
wholememory_error_code_t wgamd_call_group_layer_cols(const int* offsets, const int* frontier_batch, const int* frontier_seg,
                                                     const int* frontier_local0, const int* row_local, int64_t n_frontier,
                                                     int n_batches, int n_segments, const int* seg_tab, const int64_t* seg_base,
                                                     int64_t* self_rows, int* col, void* stream);

/* wgamd_gat_csr_f32 over a SUBSET of a larger destination list, optionally accumulating: row i of this launch reads
 * a_dst[dst_rows[i], :] and writes (accumulate: adds to) out[dst_rows[i], :].  This is one hop and edge type of a
 * heterogeneous call group: its rows are the frontier entries of that hop, dst_rows their places in the node list of the
 * destination type, and HeteroConv's sum over the relations ending in one node type is accumulate = 1 on stream-ordered
 * launches.  dst_rows = NULL, accumulate = 0: exactly wgamd_gat_csr_f32.  Row indirection / accumulation need H*C % 4 == 0,
 * H*C <= 256 and 16-byte aligned rows (WHOLEMEMORY_LOGIC_ERROR otherwise). */
wholememory_error_code_t wgamd_gat_csr_rows_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                const float* a_src, const float* a_dst, int H, int C, float negative_slope,
                                                const int64_t* dst_rows, int accumulate, float* alpha_out, float* out,
                                                int64_t ldo, void* stream);

/* out[dst_rows ? dst_rows[i] : i, 0:C] = act(in[i, 0:C] + bias)  (bias nullable, relu 0/1; C % 4 == 0, 16-byte aligned rows):
 * the tail of a HeteroConv layer — bias, ReLU and the placement of a hop's rows in the destination type's list — in one pass. */
wholememory_error_code_t wgamd_bias_act_rows_f32(const float* in, int64_t ldi, int64_t n_rows, int C, const float* bias, int relu,
                                                 const int64_t* dst_rows, float* out, int64_t ldo, void* stream);

/* GAT aggregation BEFORE the dense transform (csrc/wg_aggregate.hip) — for sampled hops, where destinations are 10-20x
 * fewer than sources.  The attention-weighted sum is linear in the source rows, so
 *   agg[i, h, :] = sum_{e in row i} alpha_e^h x[col[e], :]          (x UNTRANSFORMED, F floats; out row i = [H][F])
 * followed by H small GEMMs  out[i, h, :] = agg[i, h, :] @ W[:, h*C:(h+1)*C]  over the destination rows only equals
 * GATConv's  sum_e alpha_e^h (x W)[col[e], h, :]  up to fp32 reassociation, without the lin GEMM over every source row.
 * alpha as in wgamd_gat_csr_f32 from a_src [N_src, H] (= x_src @ fold(W, att_src)) and a_dst[dst_rows ? dst_rows[i] : i, :].
 * Shapes: F % 4 == 0, F <= 256, H in {1, 2, 4, 8}, 16-byte aligned rows, ldo >= H * F. */
wholememory_error_code_t wgamd_gat_aggregate_heads_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                       int64_t ldx, int F, const float* a_src, const float* a_dst, int H,
                                                       float negative_slope, const int64_t* dst_rows, float* out, int64_t ldo,
                                                       void* stream);
/* The same aggregation reading the source rows THROUGH an id list (fetch in the layer): neighbour j's row is x[src_ids[j]] — x
 * the feature table, src_ids (int64) the call group's node list of the source type — while a_src stays indexed by j.  The
 * [n_src, F] copy of the rows (wholememory_gather's output) is never written.  src_ids NULL = wgamd_gat_aggregate_heads_f32.
 * terms_by_id: bit 0 — a_src holds the attention terms of the TABLE's rows and is read at row src_ids[j]; bit 1 — a_dst
 * likewise at row dst_ids[dst_rows ? dst_rows[i] : i] (dst_ids = the node list of the destination type).  The per-list terms
 * are then never made: a call group lists a table row once per mini-batch that sampled it. */
wholememory_error_code_t wgamd_gat_aggregate_heads_ids_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                           int64_t ldx, const int64_t* src_ids, const int64_t* dst_ids,
                                                           int terms_by_id, int F, const float* a_src,
                                                           const float* a_dst, int H, float negative_slope,
                                                           const int64_t* dst_rows, float* out, int64_t ldo, void* stream);
/* Backward of wgamd_gat_aggregate_heads[_ids]_f32 (csrc/wg_gat_bwd.hip): given grad_agg = dL/dagg [n_rows, H F],
 * ACCUMULATES (float atomics, caller-zeroed buffers) grad_a_src / grad_a_dst at the rows the forward read its terms from
 * (per listed row, or per TABLE row with terms_by_id) and, when grad_x is given, grad_x[row of x an edge read] += sum_h
 * alpha_e^h grad_agg[i, h, :].  de: scratch [edges, H] floats (holds dL/d(score) per edge and head on return).  Same
 * addressing arguments as the forward. */
wholememory_error_code_t wgamd_gat_aggregate_heads_bwd_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                           int64_t ldx, const int64_t* src_ids, const int64_t* dst_ids,
                                                           int terms_by_id, int F, const float* a_src, const float* a_dst, int H,
                                                           float negative_slope, const int64_t* dst_rows, const float* grad_agg,
                                                           int64_t ldg, float* de, float* grad_a_src, float* grad_a_dst,
                                                           float* grad_x, int64_t ldgx, float* stats, void* stream);
/* (stats, nullable: [2][n_rows][H] floats — the rows' softmax maxima and denominators, what the kernel below reads.)
 * grad_x of the same aggregation WITHOUT atomics, source-major over the transposed hop (row_ptr_t [n_src + 1], col_t = the
 * destination row of every entry: wgamd_csr_transpose_i32): every row of grad_x [n_src, F] is written exactly once.  Plain
 * addressing (a_src per source row, a_dst at dst_rows[i]): the case of a hidden-state input. */
wholememory_error_code_t wgamd_gat_aggregate_heads_bwd_gx_f32(const int* row_ptr_t, const int* col_t, int64_t n_src, int64_t n_rows,
                                                              int F, const float* a_src, const float* a_dst, int H,
                                                              float negative_slope, const int64_t* dst_rows, const float* stats,
                                                              const float* grad_agg, int64_t ldg, float* grad_x, int64_t ldgx,
                                                              void* stream);

/* The dense tail after wgamd_gat_aggregate_heads_f32 on the matrix pipe at fp32 accuracy (csrc/wg_gat_transform.hip):
 *   out[out_rows ? out_rows[i] : i, h C + c] = act( sum_k agg[i, h F + k] W[k, h C + c] (+ acc_in[i, h C + c]) (+ bias[h C + c]) )
 * — the H per-head GEMMs, HeteroConv's sum over the relations of a destination type (`acc_in`, may alias `out` when
 * out_rows is null) and the layer's bias / ReLU / row placement in one pass.  The product is the exact 3-way bf16 split of
 * wgamd_sage_layer_fused_bf16x3 (six bf16 MFMAs per fp32 product, fp32 accumulate).  `w_tiles` = W [F, H C] row-major
 * re-ordered by wgamd_gat_transform_weight_tiles into wgamd_gat_transform_weight_bytes(F, H, C) bytes.
 * Shapes (wgamd_gat_transform_heads_supported): C == 64, F in {64, 128, 256}; rows and the bias 16-byte aligned. */
int wgamd_gat_transform_heads_supported(int F, int H, int C);
size_t wgamd_gat_transform_weight_bytes(int F, int H, int C);
wholememory_error_code_t wgamd_gat_transform_weight_tiles(const float* w, int64_t ldw, int F, int H, int C, void* tiles,
                                                          void* stream);
wholememory_error_code_t wgamd_gat_transform_heads_bf16x3(const float* agg, int64_t ld_agg, int64_t n_rows, int F, int H, int C,
                                                          const void* w_tiles, const float* acc_in, int64_t ld_acc,
                                                          const float* bias, int relu, const int64_t* out_rows, float* out,
                                                          int64_t ldo, void* stream);

/* wgamd_gat_aggregate_heads_f32 + wgamd_gat_transform_heads_bf16x3 as ONE kernel (csrc/wg_gat_fused.hip): the [n_rows, H F]
 * aggregate stays in LDS.  Same arguments and semantics as the two calls (a_src [N_src, H], a_dst row dst_rows ? dst_rows[i] : i,
 * leaky-ReLU slope, then acc_in / bias / relu / out_rows / out of the transform).  Built for the deep hop of a sampled walk:
 * rows of up to 10 neighbours run from registers, longer rows are correct but slow.
 * Shapes (wgamd_gat_layer_fused_supported): F == 128, H == 4, C == 64; 16-byte aligned rows, terms and bias. */
int wgamd_gat_layer_fused_supported(int F, int H, int C);
wholememory_error_code_t wgamd_gat_layer_fused_bf16x3(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                      int F, const float* a_src, const float* a_dst, int H, int C,
                                                      float negative_slope, const int64_t* dst_rows, const void* w_tiles,
                                                      const float* acc_in, int64_t ld_acc, const float* bias, int relu,
                                                      const int64_t* out_rows, float* out, int64_t ldo, void* stream);
/* wgamd_gat_layer_fused_bf16x3 reading the source rows through an id list (see wgamd_gat_aggregate_heads_ids_f32). */
wholememory_error_code_t wgamd_gat_layer_fused_ids_bf16x3(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                          int64_t ldx, const int64_t* src_ids, const int64_t* dst_ids,
                                                          int terms_by_id, int F, const float* a_src,
                                                          const float* a_dst, int H, int C, float negative_slope,
                                                          const int64_t* dst_rows, const void* w_tiles, const float* acc_in,
                                                          int64_t ld_acc, const float* bias, int relu, const int64_t* out_rows,
                                                          float* out, int64_t ldo, void* stream);

/* Backward of wgamd_gat_csr_f32 (csrc/wg_gat_bwd.hip): given grad_out [n_rows, H*C] and the forward's alpha [E, H], writes
 * grad_x [n_src, H*C], grad_a_src [n_src, H], grad_a_dst [n_rows, H]; de [E, H] is scratch.  Needs the hop CSR transposed:
 * row_ptr_t [n_src+1], edge_perm [E] (edge ids sorted by source, stable), edge_dst [E] (destination row of every edge).
 * Shapes: C % 4 == 0, C/4 a power of two, H*C <= 256 — anything else returns WHOLEMEMORY_LOGIC_ERROR.
 * workspace (wgamd_gat_csr_bwd_workspace_bytes(n_entries, H, C) bytes; NULL = none): with it the source-major pass sums long
 * source rows in pieces of 64 entries and adds the pieces up in order (a power-law hop has hub sources with thousands of
 * entries).  Two entry points, one algorithm:
 *   wgamd_gat_csr_bwd_f32     — the signature of rounds 1-2 (no n_entries): the piece capacity is what the workspace holds;
 *   wgamd_gat_csr_bwd_f32_v2  — n_entries = E, the entry count of the transposed hop (row_ptr_t[n_src]): a non-NULL workspace
 *                               smaller than wgamd_gat_csr_bwd_workspace_bytes(n_entries, H, C) returns
 *                               WHOLEMEMORY_INVALID_INPUT (as wgamd_spmm_csr_segmented_f32 does).
 * Either way the slots are bounded on the device: a long row whose pieces do not fit gets none, nothing is written past the
 * workspace, and the int at byte 8 of the (256-byte aligned) workspace is set to 1 — the gradients of that row are then
 * incomplete; with the workspace size the query returns for the true E it cannot happen. */
size_t wgamd_gat_csr_bwd_workspace_bytes(int64_t n_entries, int H, int C);
wholememory_error_code_t wgamd_gat_csr_bwd_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                               const float* a_src, const float* a_dst, int H, int C, float negative_slope,
                                               const float* alpha, const float* grad_out, int64_t ldg, const int* row_ptr_t,
                                               const int* edge_perm, const int* edge_dst, int64_t n_src, float* de,
                                               float* grad_x, int64_t ldgx, float* grad_a_src, float* grad_a_dst,
                                               void* workspace, size_t workspace_bytes, void* stream);
wholememory_error_code_t wgamd_gat_csr_bwd_f32_v2(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                  const float* a_src, const float* a_dst, int H, int C, float negative_slope,
                                                  const float* alpha, const float* grad_out, int64_t ldg, const int* row_ptr_t,
                                                  const int* edge_perm, const int* edge_dst, int64_t n_src, float* de,
                                                  float* grad_x, int64_t ldgx, float* grad_a_src, float* grad_a_dst,
                                                  int64_t n_entries, void* workspace, size_t workspace_bytes, void* stream);

/* A whole SAGEConv layer over a sampled hop in ONE kernel (csrc/wg_sage_fused.hip):
 *   out[i,:] = act( [ mean|sum_{e in row i} X[col[e]] | X[self_rows[i]] ] @ w_t + bias ),  X[r] = x[src_ids ? src_ids[r] : r]
 * feature fetch -> aggregation (fp32, CSR order) -> fp32-MFMA transform; the [n_rows, 2F] operand lives only in LDS.
 * w_t: [2F, N] row-major (rows 0..F-1 = W_l^T, rows F..2F-1 = W_r^T), ldw >= N; bias nullable; relu != 0 applies max(.,0).
 * x_rows = number of rows of x (0 = unknown): below 4 GB the kernel uses 32-bit row offsets.
 * Shapes: F % 4 == 0, F <= 256, N in {64, 128, 256}, x rows 16-B aligned — anything else returns WHOLEMEMORY_LOGIC_ERROR
 * (callers then use wgamd_sage_aggregate_f32 + a library GEMM).  Semantics: torch_geometric.nn.SAGEConv as the reference
 * uses it (python/pylibwholegraph/pylibwholegraph/torch/gnn_model.py:25-59). */
wholememory_error_code_t wgamd_sage_layer_fused_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                    int64_t ldx, int64_t x_rows, int F, const void* src_ids,
                                                    wholememory_dtype_t src_ids_dtype, const int64_t* self_rows, int mean,
                                                    const float* w_t, int64_t ldw, int N, const float* bias, int relu,
                                                    float* out, int64_t ldo, void* stream);

/* The same layer with the dense product evaluated on the bf16 matrix pipe at fp32 accuracy: both operands are split
 * exactly into three bf16 pieces (a = a_hi + a_mid + a_lo; 24 = 3 x 8 significand bits) and the six products of weight
 * >= 2^-16 are accumulated in fp32 (v_mfma_f32_32x32x16_bf16); the dropped terms are <= 2^-23 |a b|, the class of fp32
 * round-off.  Six bf16 MFMAs cost 6/16 of one fp32 MFMA, which takes the layer from the fp32-MFMA roof to the HBM roof.
 * `w_planes` is the weight [2F, N] re-ordered by wgamd_sage_split_weight_bf16x3 into wgamd_sage_weight_planes_bytes(2F, N)
 * bytes (do it once per weight update): since round 3 fp32 tiles [k-step][column][16 consecutive k] — the weight travels as
 * 4 bytes per element and the multiplying waves split it in registers (the pre-split planes were 6; the weight stream is what
 * the layer's time is most sensitive to).  The buffer is opaque to callers; the entry-point names are kept.  Shapes: F % 4 == 0 and small enough for two 32-row tiles of 3 bf16 planes in
 * 160 KB of LDS (F <= 208), N in {64, 128, 256}: wgamd_sage_layer_bf16x3_supported.  Inf/NaN features give NaN rows. */
size_t wgamd_sage_weight_planes_bytes(int K, int N);
int wgamd_sage_layer_bf16x3_supported(int F, int N);
/* The same buffer (and the padded bias) straight from a layer's parameters in torch.nn.Linear's layout — w_l, w_r [N, F]
 * row-major, bias [N] (nullable): the operand [W_l | W_r]^T with its columns zero-padded from N to Np, one launch.  `planes`
 * holds wgamd_sage_weight_planes_bytes(2F, Np) bytes, `bias_out` (nullable) Np floats; `full_tiles`: see WGAMD_SAGE_FULL_TILES. */
wholememory_error_code_t wgamd_sage_layer_weight_planes(const float* w_l, int64_t ldl, const float* w_r, int64_t ldr,
                                                        const float* bias, int F, int N, int Np, void* planes,
                                                        float* bias_out, int full_tiles, void* stream);
/* Tile shape of the layer kernel.  F > 148 (wgamd_sage_layer_uses_half_tiles) runs 64-row tiles whose mean half alone goes
 * through LDS, with pre-split weight planes; a launch of a few thousand rows (ONE mini-batch: 20 tiles on 256 CUs, each a serial
 * chain of row fetches) is faster on whole 32-row tiles.  Such a launch passes `relu | WGAMD_SAGE_FULL_TILES` and planes made with
 * full_tiles = 1 (fp32 tiles); both default to the throughput shape. */
#define WGAMD_SAGE_FULL_TILES 2
int wgamd_sage_layer_uses_half_tiles(int F);
wholememory_error_code_t wgamd_sage_split_weight_bf16x3(const float* w_t, int64_t ldw, int K, int N, void* planes,
                                                        void* stream);
wholememory_error_code_t wgamd_sage_layer_fused_bf16x3(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                       int64_t ldx, int64_t x_rows, int F, const void* src_ids,
                                                       wholememory_dtype_t src_ids_dtype, const int64_t* self_rows, int mean,
                                                       const void* w_planes, int N, const float* bias, int relu, float* out,
                                                       int64_t ldo, void* stream);

/* ---- training: the one-kernel layer's forward with the aggregate kept, and its weight gradient ------------------------------
 * The reference's models train (python/pylibwholegraph/pylibwholegraph/torch/gnn_model.py:25-59,119-125; every example ends in
 * loss.backward()): these two entry points are what the autograd.Function of wholegraph_amd.nn binds.
 *
 * wgamd_sage_layer_fused_bf16x3_train: wgamd_sage_layer_fused_bf16x3 (same launch, same bits in `out`) that also writes the
 * aggregate half of its operand, agg_out[i, 0:F] = mean|sum_{e in row i} X[col[e]] (fp32, ld_agg >= F floats, rows 16-B
 * aligned; NULL = not kept): n_rows F 4 bytes written once instead of E F 4 bytes of neighbour rows fetched again in the
 * backward pass. */
wholememory_error_code_t wgamd_sage_layer_fused_bf16x3_train(const int* row_ptr, const int* col, int64_t n_rows, const float* x,
                                                             int64_t ldx, int64_t x_rows, int F, const void* src_ids,
                                                             wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                                             int mean, const void* w_planes, int N, const float* bias, int relu,
                                                             float* out, int64_t ldo, float* agg_out, int64_t ld_agg,
                                                             void* stream);

/* ---- the one-kernel layer over a float16 / bfloat16 feature table -------------------------------------------------------------
 * wgamd_sage_layer_fused_bf16x3_x(_train): the two launches above with the element type of `x` as an argument — x_dtype =
 * WHOLEMEMORY_DT_FLOAT, WHOLEMEMORY_DT_HALF or WHOLEMEMORY_DT_BF16; `ldx` counts ELEMENTS of that type (ldx % 4 == 0; x is 16-B
 * aligned for FLOAT, 8-B aligned for the 16-bit types).  The stored value becomes fp32 exactly as it is read (as the reference's
 * WholeMemory gather converts a 16-bit store on the way out), everything after that is the float32 layer: `out` and `agg_out` are
 * bit for bit those of the FLOAT launch over the same values.  The row fetch, most of the launch's bytes, moves 2 bytes per
 * feature instead of 4.  With FLOAT they ARE the entry points above (which call these).  A 16-bit x is read by row (src_ids NULL)
 * or through INT / INT64 row numbers; WGAMD_IDS_BYTE_OFFSETS with a 16-bit x is WHOLEMEMORY_LOGIC_ERROR.
 * wgamd_sage_layer_x16_supported(F, N, x_dtype): wgamd_sage_layer_bf16x3_supported for one of the three types, 0 for any other. */
int wgamd_sage_layer_x16_supported(int F, int N, wholememory_dtype_t x_dtype);
wholememory_error_code_t wgamd_sage_layer_fused_bf16x3_x(const int* row_ptr, const int* col, int64_t n_rows, const void* x,
                                                         wholememory_dtype_t x_dtype, int64_t ldx, int64_t x_rows, int F,
                                                         const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                         const int64_t* self_rows, int mean, const void* w_planes, int N,
                                                         const float* bias, int relu, float* out, int64_t ldo, void* stream);
wholememory_error_code_t wgamd_sage_layer_fused_bf16x3_x_train(const int* row_ptr, const int* col, int64_t n_rows, const void* x,
                                                               wholememory_dtype_t x_dtype, int64_t ldx, int64_t x_rows, int F,
                                                               const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                               const int64_t* self_rows, int mean, const void* w_planes, int N,
                                                               const float* bias, int relu, float* out, int64_t ldo,
                                                               float* agg_out, int64_t ld_agg, void* stream);

/* Weight gradient of the layer  out = act([agg | X[self_rows]] @ [W_l | W_r]^T + b)  over one hop (csrc/wg_sage_bwd.hip):
 *   dZ[i, :]      = grad_out[i, :]  where  act_out == NULL or act_out[i, :] > 0,  else 0        (ReLU mask folded in)
 *   grad_w_l[n,f] (+)= sum_i dZ[i, n] agg[i, f]          grad_w_r[n,f] (+)= sum_i dZ[i, n] X[self_rows[i], f]
 *   grad_bias[n]  (+)= sum_i dZ[i, n]                                                           (nullable)
 * X[r] = x[src_ids ? src_ids[r] : r] as in the forward; grad_w_l / grad_w_r are [N, F] row-major contiguous (the layout of
 * torch.nn.Linear.weight); accumulate != 0 adds to what they hold (a layer that ran over several hops).  A split-K product on
 * the bf16 matrix pipe at fp32 accuracy (the exact 3-way split of the forward, six products per term, fp32 accumulate): every
 * workgroup owns a contiguous range of rows, keeps its [2F, N] partial sum in registers and writes it once; the partial sums
 * are added in workgroup order by a second launch — no atomics, the same bits from run to run.
 * Shapes: F % 4 == 0, F <= 256, N <= 256; x / agg rows 16-B aligned.  workspace: wgamd_sage_wgrad_workspace_bytes(n_rows, F, N)
 * bytes of device scratch (0 = shape not supported).  Extents: x of any size (64-bit row offsets, every id kind); agg, grad_out
 * and act_out anywhere, any n_rows, but a tile of rows is read with 32-bit offsets from its first row: a row stride (ld_agg, ldg,
 * ld_act) of 2^24 floats or more (64 rows spanning 4 GiB) is WHOLEMEMORY_INVALID_INPUT. */
size_t wgamd_sage_wgrad_workspace_bytes(int64_t n_rows, int F, int N);
wholememory_error_code_t wgamd_sage_wgrad_bf16x3(const float* agg, int64_t ld_agg, const float* x, int64_t ldx, int F,
                                                 const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                 const int64_t* self_rows, int64_t n_rows, const float* grad_out, int64_t ldg,
                                                 const float* act_out, int64_t ld_act, int N, float* grad_w_l,
                                                 float* grad_w_r, float* grad_bias, int accumulate, void* workspace,
                                                 size_t workspace_bytes, void* stream);

/* ---- the feature fetch of the one-kernel layer over a PEER-MAPPED table ------------------------------------------------------
 * src_ids_dtype = WGAMD_IDS_BYTE_OFFSETS in wgamd_sage_layer_fused_bf16x3(_train) / wgamd_sage_wgrad_bf16x3: `src_ids` is then
 * an int64 list of BYTE offsets from `x` (row r of the layer's input starts at (char*)x + src_ids[r]) instead of row numbers —
 * what wgamd_mapped_row_offsets (include/wgamd_comm.h) makes of a call group's node ids for a CHUNKED / CONTINUOUS table whose
 * partitions live on several GPUs: the layer kernel then reads remote rows over xGMI itself, x = table[n_id] never exists. */
#define WGAMD_IDS_BYTE_OFFSETS ((wholememory_dtype_t)64)

/* Biased (A-Res) sampling, fan-out <= 32: how wholegraph_csr_weighted_sample_without_replacement and the biased call-group
 * hop find the M largest keys.  pruning = 1 (default): a cheap lower bound of every |key| first, exact keys (log1pf, two
 * divisions) only for the candidates that can still reach the M-th largest one — same picks as computing every key
 * (csrc/wg_sample.hip, "threshold pruning").  force_redo = 1 (default 0) sends every row through the hand-back path the pruned
 * kernels take for a row they cannot decide: a test switch.  A negative argument leaves that setting as it is. */
void wgamd_set_weighted_sampling_mode(int pruning, int force_redo);
/* Uniform hops of a call group whose frontier capacity is at least `min_capacity` entries (and whose fan-out is at most 32)
 * walk the frontier grouped by vertex-id range instead of in list order: identical results (every entry keeps its own PCG
 * streams and output positions), a third of the cache-line fetches where the frontier repeats its hubs batch after batch.
 * OFF by default (the sampling kernel is bound by VALU issue on an MI355X, not by the lines it fetches: same duration, plus
 * the two launches that build the order); environment: WGAMD_SAMPLE_LOCALITY=<n>; min_capacity <= 0 switches it off. */
void wgamd_set_sample_locality_min(int64_t min_capacity);

/* Uniform neighbour sampling WITH replacement (cugraph_pyg `replace=True`; the reference forwards it to libcugraph,
 * sampler/distributed_sampler.py:775-792,864 — not in its tree, so the draw layout is this library's and is pinned by
 * the CPU restatement of the parity tests).  Same tensors, contexts and error behaviour as wholegraph_csr_unweighted_sample_without_replacement
 * (include/wgamd_ops.h); a seed with N > 0 neighbours yields exactly `sample_count` picks,
 * pick t = col[start + G(random_seed, i * sample_count + t).i31() % N] in draw order, a seed without neighbours none. */
wholememory_error_code_t wgamd_csr_uniform_sample_with_replacement(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t center_nodes_tensor, int sample_count, wholememory_tensor_t output_sample_offset_tensor,
  void* output_dest_memory_context, void* output_center_localid_memory_context, void* output_edge_gid_memory_context,
  unsigned long long random_seed, wholememory_env_func_t* p_env_fns, void* stream);

/* Feature gather with a narrow product folded in, one pass over the gathered rows:
 *   out_x[i, :] = table[ids[i], :]          out_terms[i, :] = table[ids[i], :] @ v       (v [F, T] row-major, T <= 32)
 * fp32 in, exact-fp32 MFMA products, fp32 accumulation.  A negative id skips the row (out_x[i] untouched) and yields zero terms.
 * For the attention logits of GATConv (x_j . fold(W, att) per relation end — the reference's models build
 * torch_geometric.nn.GATConv, /root/reference/python/pylibwholegraph/pylibwholegraph/torch/gnn_model.py:45-59): the second pass
 * over every gathered row that a separate [n, F] x [F, T] GEMM costs disappears.
 * term_group = 0: out_terms is [n, T] rows (ldo floats apart).  term_group = 4 (T % 4 == 0): slabs [T / 4][n][4] — the four
 * terms of relation end k for all rows are contiguous (what a GAT kernel with H = 4 heads reads), ldo unused.
 * ids = NULL: the rows 0 .. n-1 of `table` as they lie; out_x = NULL: only the terms are produced (both: the narrow product
 * of a resident [n, F] matrix in one streaming pass — the layer-2 attention logits of a hidden state).
 * Shapes: F in {32, 64, 128, 256} (wgamd_gather_terms_supported), rows 16-byte aligned; others: WHOLEMEMORY_LOGIC_ERROR. */
int wgamd_gather_terms_supported(int F, int T);
wholememory_error_code_t wgamd_gather_terms_f32(const float* table, int64_t ldt, const void* ids, wholememory_dtype_t id_dtype,
                                                int64_t n, int F, const float* v, int T, float* out_x, int64_t ldx,
                                                float* out_terms, int64_t ldo, int term_group, void* stream);
/* slabs_out[k][i][0..3] = slabs_in[k][ids[i]][0..3], k < n_slabs: the attention terms of a call group's rows taken from the
 * terms of the TABLE's rows ([n_slabs][n_in][4], what wgamd_gather_terms_f32 writes with ids = NULL and term_group = 4).  A
 * call group lists a table row once per mini-batch that sampled it; when the table is shorter than the list, x @ v over the
 * table + this gather of 16-byte rows replaces x[ids] @ v over the list.  A negative or out-of-range id gives zero terms. */
wholememory_error_code_t wgamd_gather_term_slabs_f32(const float* slabs_in, int64_t n_in, int n_slabs, const void* ids,
                                                     wholememory_dtype_t id_dtype, int64_t n, float* slabs_out, void* stream);
/* dv [F, T] += x^T [F, n] . dterms [n, T] (row-major, contiguous): the weight gradient of terms = x @ v for a narrow v
 * (T <= 32) over a LONG x (a whole feature table: the reduction runs over its rows); float atomics into the caller's
 * (zeroed) dv.  F <= 256. */
wholememory_error_code_t wgamd_rows_terms_bwd_f32(const float* x, int64_t ldx, int64_t n, int F, const float* dterms, int T,
                                                  float* dv, void* stream);

/* De-duplication of an id list with a known bound (ids < id_bound, e.g. the vertex count of the table they index):
 *   distinct[0 .. *n_distinct_dev)  the distinct non-negative ids, ASCENDING (so already grouped by owner rank of a
 *                                   range-partitioned table); capacity min(n, id_bound) entries
 *   inverse[i]                      position of ids[i] in `distinct`; -1 for a negative id (a row to skip) and for an id
 *                                   >= id_bound (then *out_of_bound_dev = 1, nullable)
 * Mark -> scan over the bound -> compact -> look up: no sort, no hash table, no host synchronisation (csrc/wg_unique.hip).
 * Used by the partitioned FeatureStore to send each distinct row of a call group over xGMI ONCE
 * (wholegraph_amd/tensor.py, DistributedWholeMemoryTensor.gather(dedup=...)): the reference's
 * wholememory_gather_nccl exchanges every requested id (/root/reference/cpp/src/wholememory_ops/gather_op_impl_nccl.cu:23-171).
 * Workspace: wgamd_unique_bounded_workspace_bytes(id_bound) (0 = bound not supported: must be in (0, 2^31 - 4096)), 256-byte aligned:
 * about 1.4 bytes per possible id, plus — for bounds up to 2^23, whose marks are kept as bits in LDS — the workgroups' bit slabs,
 * up to 256 x 128 KB = 32 MB.  Always ask; the size depends on the bound only, never on n. */
size_t wgamd_unique_bounded_workspace_bytes(int64_t id_bound);
wholememory_error_code_t wgamd_unique_bounded(const void* ids, wholememory_dtype_t id_dtype, int64_t n, int64_t id_bound,
                                              int64_t* distinct, int* inverse, int* n_distinct_dev, int* out_of_bound_dev,
                                              void* workspace, size_t workspace_bytes, void* stream);
/* The same over a CAPACITY-sized list whose live length is on the device (`n_live_dev`, nullable = n): the node list of a
 * no-sync call-group walk.  Lets the de-duplication run on the walk's stream right behind the walk, its count travelling
 * with the walk's own size read-back — the call group's distinct feature rows are then fetched ONCE and the first layer
 * reads them through `inverse` (its src_ids), at N = 1 as at N > 1 (bench.py, round 6). */
wholememory_error_code_t wgamd_unique_bounded_live(const void* ids, wholememory_dtype_t id_dtype, int64_t n, const int* n_live_dev,
                                                   int64_t id_bound, int64_t* distinct, int* inverse, int* n_distinct_dev,
                                                   int* out_of_bound_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Softmax cross-entropy of the seeds' logits — the loss of every training loop of the reference
 * (/root/reference/python/pylibwholegraph/pylibwholegraph/torch/gnn_model.py:119-125: F.cross_entropy inside the batch loop).
 *   loss = sum_i w_i (lse_i - x[i, t_i]) / sum_i w_i  over rows with 0 <= t_i < n_classes (a negative target = torch's
 *   ignore_index), w_i = row_weight[i] or 1;   d x[i, c] = g w_i (exp(x[i, c] - lse_i) - [c == t_i]) / sum_i w_i.
 * forward: ONE launch; writes lse [n_rows], *loss_out, and into `state` (wgamd_softmax_xent_state_bytes(n_rows) bytes, zeroed
 * by the call unless state_is_zeroed; reusable as it is left) the sum of weights the backward divides by.  Per-workgroup
 * partial sums are added in workgroup order: run-to-run deterministic.  backward: ONE launch; grad_loss (nullable = 1) is a
 * DEVICE scalar, so the pair sits inside a captured per-mini-batch step (cugraph_pyg_amd.loader.PerBatchStep). */
size_t wgamd_softmax_xent_state_bytes(int64_t n_rows);
wholememory_error_code_t wgamd_softmax_xent_forward_f32(const float* logits, int64_t ld, int64_t n_rows, int n_classes,
                                                        const int64_t* target, const float* row_weight, float* lse, void* state,
                                                        int state_is_zeroed, float* loss_out, void* stream);
wholememory_error_code_t wgamd_softmax_xent_backward_f32(const float* logits, int64_t ld, int64_t n_rows, int n_classes,
                                                         const int64_t* target, const float* row_weight, const float* lse,
                                                         const void* state, const float* grad_loss, float* grad_logits, int64_t ldg,
                                                         void* stream);

/* ---- Link-prediction head (csrc/wg_link.hip) ---------------------------------------------------------------------------------
 * The inner-product decoder of the reference's link examples (cugraph_pyg/examples/mag_lp_mnmg.py; GAE's InnerProductDecoder in
 * rgcn_link_class_mnmg.py) and its binary cross-entropy, over P pairs (index_src[p], index_dst[p]) of rows of two float32 tables
 * [n_src, n_cols] / [n_dst, n_cols] (row strides ld_*, unit column stride; the same table twice is the homogeneous case):
 *   s_p  = sum_c x_src[index_src[p], c] x_dst[index_dst[p], c]
 *   loss = sum_p w_p (max(s_p, 0) - s_p y_p + log1p(exp(-|s_p|)))  (`mean`: / sum_p w_p),  y_p = label[p] in [0, 1],
 *          w_p = pair_weight[p] (nullable = 1)
 *   c_p  = w_p (sigmoid(s_p) - y_p)   -> coef [n_pairs + 1]: the coefficients the backward multiplies with, then sum_p w_p
 * A pair with an index outside its table reads nothing: s_p = NaN (so is the loss), c_p = 0.
 * forward: ONE launch each.  16-byte row loads when n_cols, both strides and both bases allow it, scalar loads otherwise.
 * _bce_: `score` is nullable; `state` (wgamd_pair_bce_state_bytes bytes, zeroed by the call unless state_is_zeroed, reusable as
 * it is left by any later call on the same stream) holds the per-workgroup partial sums, added in workgroup order by the last
 * workgroup to finish: the loss is run-to-run bit-identical.  *loss_out and coef[n_pairs] are device scalars.
 * backward, ONE launch per side, no atomics on floats, run-to-run bit-identical:
 *   out[r] = scale * sum_{k in row r} coef[pair[k]] x_other[index_other[pair[k]]]  (+ acc[r]),  scale = *scale_num / *scale_den
 * (both nullable = 1: the upstream gradient, and coef + n_pairs for the mean) over the side's incidence list (row_ptr [n_rows + 1],
 * pair [n_pairs]: the pair ids grouped by row in pair order — wgamd_coo_to_csr_i64's row_ptr and edge_perm over index_row clamped
 * into [0, n_rows); n_pairs, n_rows, n_other < 2^31).  A pair whose index_row or index_other is out of range adds nothing; rows without pairs get zeros (acc[r]).
 * The list is summed in chunks of 64 entries whatever rows they cover and the pieces of a row are added in chunk order, so the
 * launch does not last as long as its longest row.  acc may be out itself.  workspace: wgamd_pair_grad_workspace_bytes bytes; its
 * counters are zeroed by the call unless counters_are_zeroed, and left zeroed.  No host synchronisation, no allocation. */
size_t wgamd_pair_bce_state_bytes(int64_t n_pairs);
wholememory_error_code_t wgamd_pair_dot_forward_f32(const float* x_src, int64_t ld_src, int64_t n_src, const float* x_dst,
                                                    int64_t ld_dst, int64_t n_dst, int n_cols, const int64_t* index_src,
                                                    const int64_t* index_dst, int64_t n_pairs, float* score, void* stream);
wholememory_error_code_t wgamd_pair_bce_forward_f32(const float* x_src, int64_t ld_src, int64_t n_src, const float* x_dst,
                                                    int64_t ld_dst, int64_t n_dst, int n_cols, const int64_t* index_src,
                                                    const int64_t* index_dst, int64_t n_pairs, const float* label,
                                                    const float* pair_weight, int mean, float* score, float* coef, void* state,
                                                    int state_is_zeroed, float* loss_out, void* stream);
size_t wgamd_pair_grad_workspace_bytes(int64_t n_pairs, int n_cols);
wholememory_error_code_t wgamd_pair_grad_f32(const int* row_ptr, const int* pair, int64_t n_rows, int64_t n_pairs,
                                             const int64_t* index_row, const int64_t* index_other, const float* coef,
                                             const float* x_other, int64_t ld_other, int64_t n_other, int n_cols,
                                             const float* scale_num, const float* scale_den, const float* acc, int64_t ld_acc,
                                             float* out, int64_t ld_out, void* workspace, size_t workspace_bytes,
                                             int counters_are_zeroed, void* stream);

/* ---- MLP edge decoder of link prediction (csrc/wg_link_mlp.hip) ---------------------------------------------------------------
 * The EdgeDecoder of the reference's cugraph_pyg/examples/movielens_mnmg.py and taobao_mnmg.py over the pairs of the head above:
 *   a_p = [x_src[index_src[p]] | x_dst[index_dst[p]]]   (K = c_src + c_dst columns)
 *   h_p = relu(a_p W1^T + b1)                            W1 [hidden, ldw1] row-major (torch.nn.Linear.weight), b1 nullable
 *   s_p = h_p . w2 + b2                                  w2 [hidden]; b2 nullable, ONE float on the device
 * and, when `label` is given, the binary cross-entropy of the head above over s_p (label, pair_weight, mean, coef [n_pairs + 1],
 * state of wgamd_pair_bce_state_bytes bytes, *loss_out: exactly as wgamd_pair_bce_forward_f32; `score` is then nullable).
 * forward: ONE launch, 16 pairs per tile; neither the gathered rows nor their concatenation reach memory, and the hidden
 * activation only when hidden_out is given ([n_pairs, ld_hidden], ld_hidden >= hidden rounded up to 4, rows 16-B aligned; the
 * columns up to that width are written).  Product 1 runs on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
 * wgamd_pair_mlp_supported: c_src, c_dst multiples of 4, c_src + c_dst <= 1024, 1 <= hidden <= 256; x_src / x_dst / w1 rows
 * 16-B aligned.  A pair with an index outside its table reads nothing: s_p = NaN (so is the loss), c_p = 0, hidden_out row 0.
 * backward, ONE launch over the kept hidden rows: hidden_io[p] <- dZ_p = g_p w2 * [h_p > 0], grad_w2 = sum_p g_p h_p,
 * grad_b2 = sum_p g_p (both nullable), g_p = g[p] * *scale_num / *scale_den (both nullable = 1), 0 for a pair with an index
 * outside its table.  Per-workgroup partial sums added in workgroup order: no float atomics, run-to-run bit-identical.
 * workspace: wgamd_pair_mlp_backward_workspace_bytes bytes, its ticket zeroed by the call unless workspace_is_zeroed, and left
 * zeroed.  The sums of dZ over a row's pairs are wgamd_pair_grad_f32 (x_other = dZ, index_other = 0..n_pairs-1, coef = 1). */
int wgamd_pair_mlp_supported(int c_src, int c_dst, int hidden);
wholememory_error_code_t wgamd_pair_mlp_forward_f32(const float* x_src, int64_t ld_src, int64_t n_src, const float* x_dst,
                                                    int64_t ld_dst, int64_t n_dst, int c_src, int c_dst, const int64_t* index_src,
                                                    const int64_t* index_dst, int64_t n_pairs, const float* w1, int64_t ldw1,
                                                    int hidden, const float* b1, const float* w2, const float* b2,
                                                    const float* label, const float* pair_weight, int mean, float* score,
                                                    float* coef, void* state, int state_is_zeroed, float* loss_out,
                                                    float* hidden_out, int64_t ld_hidden, void* stream);
size_t wgamd_pair_mlp_backward_workspace_bytes(int hidden);
wholememory_error_code_t wgamd_pair_mlp_backward_f32(float* hidden_io, int64_t ld_hidden, int64_t n_pairs, int hidden,
                                                     const float* w2, const float* g, const float* scale_num,
                                                     const float* scale_den, const int64_t* index_src, int64_t n_src,
                                                     const int64_t* index_dst, int64_t n_dst, float* grad_w2, float* grad_b2,
                                                     void* workspace, size_t workspace_bytes, int workspace_is_zeroed,
                                                     void* stream);

/* ---- Row-wise first-appearance de-duplication (csrc/wg_rows_unique.hip) --------------------------------------------------------
 * The endpoints of a link call group's seed edges, ends int64 [n_rows, row_len] (contiguous; one row per mini-batch, values
 * promised in [0, n_ids), id 0 a real id), de-duplicated row by row in order of first position:
 *   uniq  int64 [n_rows row_len]: row g's distinct values, in order of first position, back to back from seg[g]; 0 from seg[n_rows] on
 *   seg   int32 [n_rows + 1]:     prefix sum of the rows' distinct counts
 *   batch int32 [n_rows row_len]: batch[seg[g] + r] = g; 0 from seg[n_rows] on
 *   local int64 [n_rows, row_len]: local[g, s] = position of ends[g, s] in row g's list
 * Two launches, no host synchronisation, no allocation; every first position is a minimum, so the result does not depend on
 * scheduling.  wgamd_rows_first_unique_supported: n_rows >= 1, 1 <= row_len <= WGAMD_ROWS_FIRST_UNIQUE_MAX_S (one workgroup's
 * LDS table: 2 row_len slots of 8 bytes, 128 KiB of the CU's 160 KiB at the bound), n_rows row_len < 2^31, 1 <= n_ids <= 2^40
 * (an id and a position share a 64-bit word, 40 + 24 bits).  Whatever ends holds, nothing is written outside the outputs and the
 * workspace: a value outside [0, 2^40) is de-duplicated by its low 40 bits.  workspace: wgamd_rows_first_unique_workspace_bytes
 * bytes; its ticket (the first 256 bytes after rounding the pointer up to 256) is zeroed by the call unless
 * workspace_is_zeroed, and left zeroed. */
#define WGAMD_ROWS_FIRST_UNIQUE_MAX_S 8192
int wgamd_rows_first_unique_supported(int64_t n_rows, int64_t row_len, int64_t n_ids);
size_t wgamd_rows_first_unique_workspace_bytes(int64_t n_rows, int64_t row_len);
wholememory_error_code_t wgamd_rows_first_unique(const int64_t* ends, int64_t n_rows, int64_t row_len, int64_t n_ids, int64_t* uniq,
                                                 int* seg, int* batch, int64_t* local, void* workspace, size_t workspace_bytes,
                                                 int workspace_is_zeroed, void* stream);

/* A value per distinct id of every row, taken at the id's FIRST position (the seed time of a de-duplicated endpoint is the time
 * of the first seed edge that names it): with local / seg as wgamd_rows_first_unique leaves them and values int64
 * [n_rows, row_len] parallel to ends,
 *   out int64 [n_rows row_len]: out[seg[g] + local[g, s]] = values[g, s] for every first position s of row g; 0 from seg[n_rows] on
 * — parallel to uniq.  Position s is a first position exactly when local[g, s] exceeds every earlier local[g, .] (the lists
 * are numbered in order of first position).  One launch, one workgroup per row with the running maximum of the row in LDS,
 * one store per first position, no atomics, nothing read back.  Domain: wgamd_rows_first_unique_supported(n_rows, row_len, 1).
 * Whatever local and seg hold, nothing is written outside out. */
wholememory_error_code_t wgamd_rows_first_values(const int64_t* local, const int* seg, const int64_t* values, int64_t n_rows,
                                                 int64_t row_len, int64_t* out, void* stream);

/* ---- GCN layer (csrc/wg_gcn.hip): torch_geometric.nn.GCNConv over a sampled hop ---------------------------------------------
 * The model of the reference's headline cugraph-pyg example (python/cugraph-pyg/cugraph_pyg/examples/gcn_dist_mnmg.py):
 *   agg[i]  = s_i ( sum_{e = (j -> i), not a loop} w_e d_j X[j]  +  [loops] loopw_i d_self X[self_rows[i]] )
 *   out[i]  = act(agg[i] @ W^T + b)
 * "a loop" = col[e] == self_rows[i] while WGAMD_GCN_ADD_SELF_LOOPS is set (add_remaining_self_loops: the loop edge is not
 * summed, it gives the added loop its weight — the last one of the row; loopw_i = fill when the row has none);
 * w_e = edge_weight[e] (nullable = 1); d_j = dinv_src[j] (nullable = 1); s_i = dinv_dst[i], or dinv_src[self_rows[i]] when
 * dinv_dst is null (1 when both are); d_self = dinv_src[self_rows[i]].  self_rows[i] < 0: row i has no self term (a
 * transposed hop's source-only rows).  X[r] = x[src_ids ? src_ids[r] : r] (INT, INT64 or WGAMD_IDS_BYTE_OFFSETS).  W is
 * [N, ldw] row-major (the layout of torch.nn.Linear.weight).  Sums run in CSR order: run-to-run deterministic.
 * Layer kernel: wgamd_gcn_layer_supported(F, N) (F % 4 == 0, F <= 256, N <= 256), x / w rows 16-B aligned; the product runs
 * on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32).  _train also writes agg [n_rows, F] (ld_agg, 16-B aligned rows;
 * same bits as the operand of the product) for the weight gradient.  wgamd_gcn_aggregate_f32: agg alone, any F. */
#define WGAMD_GCN_ADD_SELF_LOOPS 1
#define WGAMD_GCN_RELU 2
#define WGAMD_GCN_MAX_HOPS 8
int wgamd_gcn_layer_supported(int F, int N);
wholememory_error_code_t wgamd_gcn_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F,
                                             const void* src_ids, wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                             const float* edge_weight, const float* dinv_src, const float* dinv_dst, float fill,
                                             const float* w, int64_t ldw, int N, const float* bias, int flags, float* out,
                                             int64_t ldo, void* stream);
wholememory_error_code_t wgamd_gcn_layer_f32_train(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                   int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                   const int64_t* self_rows, const float* edge_weight, const float* dinv_src,
                                                   const float* dinv_dst, float fill, const float* w, int64_t ldw, int N,
                                                   const float* bias, int flags, float* out, int64_t ldo, float* agg_out,
                                                   int64_t ld_agg, void* stream);
wholememory_error_code_t wgamd_gcn_aggregate_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                 int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                 const int64_t* self_rows, const float* edge_weight, const float* dinv_src,
                                                 const float* dinv_dst, float fill, int flags, float* out, int64_t ldo,
                                                 void* stream);
/* dinv = deg^-1/2 (0 where deg == 0) of the destination rows of up to WGAMD_GCN_MAX_HOPS hops in ONE launch: deg_i = the
 * weights of row i's edges (loop edges excluded and loopw_i added when add_self_loops, as above).  Row i of hop h goes to
 * dinv[out_base[h] + i], or to dinv[self_rows[h][i]] when out_base[h] < 0; indices outside [0, n_out) are skipped, entries
 * no row reaches are left as they are.  The arrays of pointers / counts are host arrays of n_hops entries (edge_weight:
 * nullable, or an array of nullable pointers). */
wholememory_error_code_t wgamd_gcn_degrees_f32(int n_hops, const int* const* row_ptr, const int* const* col,
                                               const int64_t* const* self_rows, const float* const* edge_weight,
                                               const int64_t* n_rows, const int64_t* out_base, float fill, int add_self_loops,
                                               float* dinv, int64_t n_out, void* stream);
/* Weight gradient of the GCN layer over one hop: dZ = grad_out masked by act_out > 0 (act_out nullable = no activation),
 *   grad_w[n, f] (+)= sum_i dZ[i, n] agg[i, f]        grad_bias[n] (+)= sum_i dZ[i, n]        (grad_bias nullable)
 * F, N <= 256.  Split-K over row ranges on fp32 MFMA; partial sums (workspace: wgamd_gcn_wgrad_workspace_bytes bytes) added
 * in workgroup order — no atomics, the same bits from run to run. */
size_t wgamd_gcn_wgrad_workspace_bytes(int64_t n_rows, int F, int N);
wholememory_error_code_t wgamd_gcn_wgrad_f32(const float* agg, int64_t ld_agg, int64_t n_rows, int F, const float* grad_out,
                                             int64_t ldg, const float* act_out, int64_t ld_act, int N, float* grad_w,
                                             float* grad_bias, int accumulate, void* workspace, size_t workspace_bytes,
                                             void* stream);
/* The same over up to max_split (1..1024) row ranges instead of the 128 a hop's rows ask for: operands of many more rows (the
 * whole tables under a link head).  The ranges, hence the bits, depend on n_rows and max_split alone. */
size_t wgamd_gcn_wgrad_split_workspace_bytes(int64_t n_rows, int F, int N, int max_split);
wholememory_error_code_t wgamd_gcn_wgrad_split_f32(const float* agg, int64_t ld_agg, int64_t n_rows, int F, const float* grad_out,
                                                   int64_t ldg, const float* act_out, int64_t ld_act, int N, float* grad_w,
                                                   float* grad_bias, int accumulate, int max_split, void* workspace,
                                                   size_t workspace_bytes, void* stream);

/* ---- RGCN layer (csrc/wg_rgcn.hip): torch_geometric.nn.RGCNConv / FastRGCNConv over a sampled hop -----------------------------
 * The model of the reference's cugraph-pyg example rgcn_link_class_mnmg.py:
 *   C_b[i]  = sum_{e = (j -> i)} coef[e] comp[rel[e], b] X[j]      (b < B; comp null = the identity, B = R)
 *   out[i]  = act( sum_b C_b[i] @ basis_b  +  [has_root] X[self_rows[i]] @ root  +  bias )
 * X[r] = x[src_ids ? src_ids[r] : r] (INT, INT64 or WGAMD_IDS_BYTE_OFFSETS); self_rows[i] < 0: no root term (a transposed hop's
 * source-only rows).  The weight goes in transposed and stacked: wt [N, ldw] with wt[n, b F + f] = basis_b[f, n] and
 * wt[n, B F + f] = root[f, n].  Sums run in CSR order: run-to-run deterministic.  Domain: wgamd_rgcn_layer_supported
 * (F % 4 == 0, N <= 256, K = (B + has_root) F <= 1024: one float4 of the C row per thread, a 16 x K fp32 tile in LDS);
 * x / wt rows 16-B aligned.  The product runs on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
 * wgamd_rgcn_edge_coef: per edge of a hop, rel[e] = edge_type[e] and coef[e] = 1 / (edges of row i with that relation) when
 * mean, else 1; an id outside [0, R) gets rel 0 and coef 0 (callers refuse such ids; the kernels never index with them). */
int wgamd_rgcn_layer_supported(int F, int N, int B, int has_root);
wholememory_error_code_t wgamd_rgcn_edge_coef(const int* row_ptr, int64_t n_rows, const void* edge_type,
                                              wholememory_dtype_t edge_type_dtype, int R, int mean, int* rel, float* coef,
                                              void* stream);
wholememory_error_code_t wgamd_rgcn_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F,
                                              const void* src_ids, wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                              const int* rel, const float* coef, const float* comp, int B, int has_root,
                                              const float* wt, int64_t ldw, int N, const float* bias, int relu, float* out,
                                              int64_t ldo, void* stream);
/* Relation-segmented weight gradient: M[s] (n_seg x [F, N], row-major) = sum over pairs p of segment s of
 *   pair_coef[p] X[pair_src[p]]^T grad[pair_dst[p]]
 * with the pairs sorted by segment (seg_ptr [n_seg + 1]: pair range of each segment) and cut into work items of at most
 * pairs_per_item pairs of one segment (item_start [n_seg + 1]: first item of each segment, on the device; max_items >= the
 * total, the launch's grid).  Item partials (workspace: wgamd_rgcn_wgrad_workspace_bytes) are added in item order — no
 * atomics, the same bits from run to run.  N <= 256, pairs_per_item % 4 == 0. */
size_t wgamd_rgcn_wgrad_workspace_bytes(int64_t max_items, int F, int N);
wholememory_error_code_t wgamd_rgcn_wgrad_f32(const float* x, int64_t ldx, int F, const void* src_ids,
                                              wholememory_dtype_t src_ids_dtype, const int64_t* pair_src, const int64_t* pair_dst,
                                              const float* pair_coef, const float* grad, int64_t ldg, int N,
                                              const int64_t* item_start, const int64_t* seg_ptr, int n_seg, int64_t pairs_per_item,
                                              int64_t max_items, float* M, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Graph transformer layer (csrc/wg_transformer.hip): torch_geometric.nn.TransformerConv over a sampled hop ---------------------
 * The model of the reference's cugraph-pyg example mag_lp_mnmg.py, aggregate-first:
 *   s[e, h]  = u[i, h F + :] . X[j]  +  w[i, h D + :] . edge_attr[e]          (e = (j -> i); u, w already scaled by 1 / sqrt(C))
 *   alpha    = softmax over the edges of row i of s[:, h]
 *   A[i]     = [ blk_0 | ... | blk_(H-1) | XD[self_rows[i]] ],  blk_h = sum_e alpha[e, h] [X[j] | edge_attr[e] | 1 | 0 ...]
 *   out[i]   = act( A[i] @ Wstack + bias )
 * X[r] = x[src_ids ? src_ids[r] : r] (INT, INT64 or WGAMD_IDS_BYTE_OFFSETS); XD[r] = x_dst[r], or x_dst[src_ids[r]] with
 * x_dst_ids.  Each head block is W4 = wgamd_transformer_block_width(F_src, D) = ceil4(F_src + D + 1) wide; K = H W4 + F_dst
 * (F_dst = 0: no skip block).  The weight goes in transposed: wt [N, ldwt] = Wstack^T.  edge_attr [E, D] row-major in CSR
 * order.  A row without edges has a zero aggregate.  alpha (optional, [E, H]) receives the attention weights, a_save (optional,
 * [n_rows, K] row-major, 16-B aligned) the rows A — what the backward reads.  Sums run in CSR order: run-to-run deterministic.
 * Domain: wgamd_transformer_layer_supported (F_src, F_dst multiples of 4 and <= 256, D <= 32, H <= 8, N <= 256, K <= 1024);
 * x / x_dst / u / wt rows 16-B aligned.  The product runs on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
 * wgamd_transformer_bwd_dst_f32 (destination-major, given dA = dZ Wstack^T [n_rows, ldda] and the saved A): per edge and head
 * dalpha = dA[i, blk_h] . [X[j] | edge_attr[e] | 1] and ds = alpha (dalpha - dA[i, blk_h] . A[i, blk_h]); du [n_rows, H F_src]
 * = sum_e ds X[j], dw [n_rows, H D] = sum_e ds edge_attr[e], ds [E, H].
 * wgamd_transformer_bwd_src_f32 (source-major over the hop's transpose: row_ptr_t / col_t = destination rows / perm = CSR edge
 * of every transposed entry, over n_src input rows and the hop's n_rows destinations):
 *   gx[j] (+)= sum_e sum_h (alpha dA[i, h W4 + :F] + ds u[i, h F + :])  +  dA[self_t[j] - n_rows, skip_at + :]
 * where self_t[j] = n_rows + i when input row j is destination i (the skip term; any other value, a null self_t or
 * skip_at < 0: none) — HopGraph.transposed's self_t.  No atomics: the same bits from run to run. */
int wgamd_transformer_layer_supported(int F_src, int F_dst, int D, int H, int N);
int wgamd_transformer_block_width(int F_src, int D);
wholememory_error_code_t wgamd_transformer_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                     int F_src, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                     const float* x_dst, int64_t ldx_dst, int F_dst, const int64_t* self_rows,
                                                     int x_dst_ids, const float* edge_attr, int D, const float* u, int64_t ldu,
                                                     const float* w, int64_t ldw, int H, const float* wt, int64_t ldwt, int N,
                                                     const float* bias, int relu, float* out, int64_t ldo, float* alpha, float* a_save,
                                                     void* stream);
wholememory_error_code_t wgamd_transformer_bwd_dst_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                       int F_src, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                       const float* edge_attr, int D, int H, const float* alpha, const float* dA,
                                                       int64_t ldda, const float* A, int64_t lda, float* du, float* dw, float* ds,
                                                       void* stream);
wholememory_error_code_t wgamd_transformer_bwd_src_f32(const int* row_ptr_t, const int* col_t, const int* perm, const int64_t* self_t,
                                                       int64_t n_rows, int64_t n_src, int F_src, int D, int H, int skip_at,
                                                       const float* alpha, const float* ds, const float* dA, int64_t ldda,
                                                       const float* u, int64_t ldu, float* gx, int64_t ldgx, int accumulate,
                                                       void* stream);

/* ---- Heterogeneous SAGE layer (csrc/wg_sage_hetero.hip): HeteroConv({edge type: SAGEConv}, aggr = "sum") over one (hop,
 * destination type) of a call group — the sum over the relations ending in the type as ONE product:
 *   C[i]   = [ REDUCE_0(i) | ... | REDUCE_(n_rel-1)(i) | XD[dst_rows[i]] ]                  K = sum_r F_r + F_dst floats
 *   REDUCE_r(i) = (mean_r ? 1 / deg_r(i) : 1) sum_{e in row i of r} src_scale_r[col_r[e]] X_r[col_r[e]]    (src_scale nullable = 1)
 *   out[out_rows ? out_rows[i] : i] = act( C[i] @ wt^T + bias + acc_in[i] )
 * Every relation has its own CSR over the same n_rows rows, its own input X_r[j] = x[ids_kind ? src_ids[j] : j] (ids_kind 0: by
 * row, 1: int32 node list, 2: int64 node list) and its own width F; col0 is the column of its block in C (blocks back to back
 * from 0, in array order; the root block follows them).  Root block: XD[r] = x_dst[dst_ids_kind ? dst_ids[r] : r], dst_rows
 * nullable = row i itself, x_dst nullable = no root block.  wt [N, ldw] row-major = [ W_l^0 | ... | sum_r W_r^r ]; bias, acc_in
 * ([n_rows, ld_acc]: the running sum of an earlier launch of the same rows) and out_rows nullable.  An empty row reduces to 0.
 * Sums run in CSR order: run-to-run deterministic.  _train also writes C ([n_rows, ldc], 16-B aligned rows; same bits as the
 * operand of the product) for the weight gradient (wgamd_gcn_wgrad_f32 over column blocks of it).
 * Domain: wgamd_hetero_sage_layer_supported (at most WGAMD_HETERO_SAGE_MAX_RELATIONS relations, every F and F_dst a multiple
 * of 4, N <= 256, 0 < K <= 1024; F_dst = 0: no root block); x / x_dst / wt rows 16-B aligned.  The product runs on the exact fp32
 * matrix pipe (v_mfma_f32_16x16x4_f32). */
#define WGAMD_HETERO_SAGE_MAX_RELATIONS 8
#define WGAMD_HETERO_SAGE_RELU 1
typedef struct {
  const int* row_ptr;
  const int* col;
  const float* x;
  int64_t ldx;
  const void* src_ids;
  const float* src_scale;
  int F;
  int ids_kind;
  int mean;
  int col0;
} wgamd_hetero_sage_relation_t;
int wgamd_hetero_sage_layer_supported(const int* F, int n_rel, int F_dst, int N);
wholememory_error_code_t wgamd_hetero_sage_layer_f32(const wgamd_hetero_sage_relation_t* rels, int n_rel, int64_t n_rows,
                                                     const float* x_dst, int64_t ldx_dst, int F_dst, const int64_t* dst_rows,
                                                     const void* dst_ids, int dst_ids_kind, const float* wt, int64_t ldw, int N,
                                                     const float* bias, int flags, const float* acc_in, int64_t ld_acc,
                                                     const int64_t* out_rows, float* out, int64_t ldo, void* stream);
wholememory_error_code_t wgamd_hetero_sage_layer_f32_train(const wgamd_hetero_sage_relation_t* rels, int n_rel, int64_t n_rows,
                                                           const float* x_dst, int64_t ldx_dst, int F_dst, const int64_t* dst_rows,
                                                           const void* dst_ids, int dst_ids_kind, const float* wt, int64_t ldw,
                                                           int N, const float* bias, int flags, const float* acc_in,
                                                           int64_t ld_acc, const int64_t* out_rows, float* out, int64_t ldo,
                                                           float* c_out, int64_t ldc, void* stream);

/* ---- Heterogeneous graph transformer layer (csrc/wg_transformer_hetero.hip): HeteroConv({edge type: TransformerConv}, aggr =
 * "sum") over one (hop, destination type) of a call group — what to_hetero makes of the encoder of the reference's cugraph-pyg
 * example mag_lp_mnmg.py.  The softmax is per relation and the sum over relations is linear, so it is ONE product:
 *   s_r[e, h] = u_r[i, h F_r + :] . X_r[j]  +  w_r[i, h D_r + :] . edge_attr_r[e]     (e = (j -> i) of relation r; u, w scaled)
 *   alpha_r   = softmax over the edges of row i of relation r of s_r[:, h]
 *   A[i]      = [ blk_r0,0 | ... | blk_r0,(H_0 - 1) | blk_r1,0 | ... | XD[dst_rows[i]] ]          K = sum_r H_r W4_r + F_dst floats
 *   blk_r,h   = sum_e alpha_r[e, h] [X_r[j] | edge_attr_r[e] | 1 | 0 ...]            W4_r = wgamd_transformer_block_width(F_r, D_r)
 *   out[out_rows ? out_rows[i] : i] = act( A[i] @ wt^T + bias + acc_in[i] )
 * Every relation has its own CSR over the same n_rows rows, its own input X_r[j] = x[ids_kind ? src_ids[j] : j] (ids_kind 0: by
 * row, 1: int32 node list, 2: int64 node list), its own edge_attr [E_r, D] in CSR order (D = 0: none), per-destination vectors
 * u [n_rows, ldu] and w [n_rows, ldw] (wgamd_transformer_layer_f32's, per relation) and widths F, D, H; col0 is the column of
 * its first block in A (blocks back to back from 0, in array order; the skip block follows them).  A row without edges in a
 * relation leaves that relation's blocks exactly zero.  alpha (nullable; [E_r, H], required by _train) receives the relation's
 * attention weights.  Skip block: XD[r] = x_dst[dst_ids_kind ? dst_ids[r] : r], dst_rows nullable = row i itself, x_dst nullable
 * = no skip block.  wt [N, ldw] row-major = [ Wstack_r0^T | Wstack_r1^T | ... | sum_r lin_skip_r ]; bias, acc_in ([n_rows,
 * ld_acc]: the running sum of an earlier launch of the same rows) and out_rows nullable.  _train also writes A ([n_rows, lda],
 * 16-B aligned rows; the operand of the product): with alpha what wgamd_transformer_bwd_dst_f32 / _bwd_src_f32 read, per
 * relation, through column slices at col0.  No atomics; sums run in CSR order: run-to-run deterministic.
 * Domain: wgamd_hetero_transformer_layer_supported (at most WGAMD_HETERO_TRANSFORMER_MAX_RELATIONS relations, every F and F_dst
 * a multiple of 4 and <= 256, D <= 32, H <= 8, N <= 256, 0 < K <= 1024; F_dst = 0: no skip block); x / x_dst / u / wt rows 16-B
 * aligned.  The product runs on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32). */
#define WGAMD_HETERO_TRANSFORMER_MAX_RELATIONS 8
#define WGAMD_HETERO_TRANSFORMER_RELU 1
typedef struct {
  const int* row_ptr;
  const int* col;
  const float* x;
  int64_t ldx;
  const void* src_ids;
  const float* edge_attr;
  const float* u;
  int64_t ldu;
  const float* w;
  int64_t ldw;
  float* alpha;
  int F;
  int ids_kind;
  int D;
  int H;
  int col0;
} wgamd_hetero_transformer_relation_t;
int wgamd_hetero_transformer_layer_supported(const int* F, const int* D, const int* H, int n_rel, int F_dst, int N);
wholememory_error_code_t wgamd_hetero_transformer_layer_f32(const wgamd_hetero_transformer_relation_t* rels, int n_rel,
                                                            int64_t n_rows, const float* x_dst, int64_t ldx_dst, int F_dst,
                                                            const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind,
                                                            const float* wt, int64_t ldw, int N, const float* bias, int flags,
                                                            const float* acc_in, int64_t ld_acc, const int64_t* out_rows,
                                                            float* out, int64_t ldo, void* stream);
wholememory_error_code_t wgamd_hetero_transformer_layer_f32_train(const wgamd_hetero_transformer_relation_t* rels, int n_rel,
                                                                  int64_t n_rows, const float* x_dst, int64_t ldx_dst, int F_dst,
                                                                  const int64_t* dst_rows, const void* dst_ids, int dst_ids_kind,
                                                                  const float* wt, int64_t ldw, int N, const float* bias,
                                                                  int flags, const float* acc_in, int64_t ld_acc,
                                                                  const int64_t* out_rows, float* out, int64_t ldo, float* a_save,
                                                                  int64_t lda, void* stream);

/* ---- GIN layer (csrc/wg_gin.hip): torch_geometric.nn.GINConv with the GIN paper's MLP over a sampled hop ----------------------
 * The model of the reference's cugraph-pyg example dist_gin_sg.py (GINConv(MLP([in, hidden, hidden])), then global_add_pool):
 *   agg[i]    = sum_{e = (j -> i)} X[j]  +  (1 + eps) XS[i]          (every edge is summed: loop edges and duplicates too)
 *   hidden[i] = act1(agg[i] @ W1^T + b1)                              act1 = ReLU with WGAMD_GIN_RELU_HIDDEN
 *   out[i]    = act2(hidden[i] @ W2^T + b2)                           act2 = ReLU with WGAMD_GIN_RELU_OUT
 * X[r] = x[src_ids ? src_ids[r] : r] (INT, INT64 or WGAMD_IDS_BYTE_OFFSETS).  XS[i] = x_dst[i] when x_dst is given (the
 * bipartite form), else X[self_rows[i]]; self_rows[i] < 0, or both arrays null: row i has no self term.  eps: ONE float on the
 * device, nullable = 0.  W1 [H, ldw1] and W2 [N, ldw2] are row-major (torch.nn.Linear.weight); b1, b2 nullable.  With w2 null
 * and N = 0 the layer ends after the first product: out = hidden [n_rows, H].  Sums run in CSR order: run-to-run deterministic.
 * Layer kernel: wgamd_gin_layer_supported(F, H, N) (F % 4 == 0; F, H, N <= 256; H % 4 == 0 unless N == 0), x / x_dst / w1 / w2
 * rows 16-B aligned; both products run on the exact fp32 matrix pipe (v_mfma_f32_16x16x4_f32), the hidden activation stays in
 * LDS.  _train also writes agg [n_rows, F] and, with a second product, hidden [n_rows, H] (16-B aligned rows; the same bits as
 * the operands of the products) for the weight gradients (wgamd_gcn_wgrad_f32).  wgamd_gin_aggregate_f32: agg alone, any F.
 * wgamd_segment_sum_f32 (global_add_pool over a sorted batch vector): out[g] = sum of rows [offsets[g], offsets[g + 1]) of x,
 * offsets int64 [n_segments + 1] non-decreasing; rows are added in order, no atomics; an empty segment gives a zero row. */
#define WGAMD_GIN_RELU_HIDDEN 1
#define WGAMD_GIN_RELU_OUT 2
int wgamd_gin_layer_supported(int F, int H, int N);
wholememory_error_code_t wgamd_gin_layer_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx, int F,
                                             const void* src_ids, wholememory_dtype_t src_ids_dtype, const int64_t* self_rows,
                                             const float* x_dst, int64_t ldx_dst, const float* eps, const float* w1, int64_t ldw1,
                                             int H, const float* b1, const float* w2, int64_t ldw2, int N, const float* b2,
                                             int flags, float* out, int64_t ldo, void* stream);
wholememory_error_code_t wgamd_gin_layer_f32_train(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                   int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                   const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps,
                                                   const float* w1, int64_t ldw1, int H, const float* b1, const float* w2,
                                                   int64_t ldw2, int N, const float* b2, int flags, float* out, int64_t ldo,
                                                   float* agg_out, int64_t ld_agg, float* hidden_out, int64_t ld_hidden,
                                                   void* stream);
wholememory_error_code_t wgamd_gin_aggregate_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                 int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                 const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps,
                                                 float* out, int64_t ldo, void* stream);
wholememory_error_code_t wgamd_segment_sum_f32(const float* x, int64_t ldx, int F, const int64_t* offsets, int64_t n_segments,
                                               float* out, int64_t ldo, void* stream);

/* ---- Batch norm between the Linears of a GIN layer (csrc/wg_batch_norm.hip, csrc/wg_gin.hip): training mode ----------------------
 * The layer the reference's dist_gin_sg.py trains, GINConv(MLP([in, hidden, hidden])) with PyG's default norm="batch_norm":
 *   z      = agg @ W1^T + b1                                           [n, H]  (agg as in the GIN section above)
 *   hidden = relu((z - mean) rstd gamma + beta)                        mean, biased var over ALL n rows; rstd = 1 / sqrt(var + eps)
 *   out    = act2(hidden @ W2^T + b2)                                  [n, N]
 * The statistics need every row, so the forward is three kinds of launch:
 *  A wgamd_gin_layer_f32_stats, one per hop: the GIN layer kernel's one-product form, z kept in the LDS tile, stored to z_out
 *    (and agg to agg_out, nullable), plus a record per 16-row tile t = tile0 + (row / 16): partials[t][0][:] = the columns' mean
 *    over the tile's valid rows, partials[t][1][:] = M2 (sum of squared distances from that mean, two passes), counts[t] = valid
 *    rows.  tile0 = the tiles of the layer's earlier hops.  Domain: wgamd_gin_layer_supported(F, H, 0) and H % 4 == 0.
 *    wgamd_bn_partials_f32 writes the same records from rows z in memory.
 *  B wgamd_bn_finalize_f32, one per layer: the n_tiles records combined per column with the pairwise update of (count, mean, M2)
 *    (Chan, Golub, LeVeque 1979) in a fixed order (a contiguous chunk of tiles per thread, then a fixed tree) -> mean, var
 *    (biased), rstd, scale = gamma rstd, shift = beta - mean scale (each [H]; all but mean nullable; gamma, beta nullable = 1, 0),
 *    and running_mean / running_var (nullable) updated in place: r = (1 - momentum) r + momentum s, s = mean or the unbiased
 *    variance M2 / (n - 1).  No atomics, no sum of squares.
 *  C wgamd_bn_act_linear_f32, one per layer over all rows: 16-row tiles, hidden = relu(z scale + shift) into LDS (and hidden_out,
 *    nullable), times W2^T on the fp32 matrix pipe with b2 (nullable) and the output ReLU (relu_out).  N <= 256.
 * Backward of the normalisation and its ReLU, given dhidden = dOut W2 [n, H] and the kept hidden, z, mean, rstd:
 *   dy = dhidden [hidden > 0],  x^ = (z - mean) rstd
 *   wgamd_bn_bwd_reduce_f32: dbeta = sum dy, dgamma = sum dy x^ — wgamd_bn_bwd_blocks(n, H) partial rows of 2 H floats (the
 *     caller's workspace), each a workgroup's rows added in a fixed order, then the partial rows added in a fixed order
 *   wgamd_bn_bwd_apply_f32:  dz = gamma rstd (dy - dbeta / n - x^ dgamma / n), one pass; dz may be dhidden itself
 * No atomics: the same bits on every run.  Domain: wgamd_batch_norm_supported(H) (H % 4 == 0, 4 <= H <= 256); float32, every
 * ld >= its width and a multiple of 4, rows and the [H] vectors and partials 16-B aligned (WHOLEMEMORY_LOGIC_ERROR otherwise;
 * null pointers and short leading dimensions WHOLEMEMORY_INVALID_INPUT) — checked on the host before any launch. */
int wgamd_batch_norm_supported(int H);
int64_t wgamd_bn_bwd_blocks(int64_t n_rows, int H);
wholememory_error_code_t wgamd_gin_layer_f32_stats(const int* row_ptr, const int* col, int64_t n_rows, const float* x, int64_t ldx,
                                                   int F, const void* src_ids, wholememory_dtype_t src_ids_dtype,
                                                   const int64_t* self_rows, const float* x_dst, int64_t ldx_dst, const float* eps,
                                                   const float* w1, int64_t ldw1, int H, const float* b1, float* z_out, int64_t ldz,
                                                   float* agg_out, int64_t ld_agg, float* partials, int* counts, int64_t tile0,
                                                   void* stream);
wholememory_error_code_t wgamd_bn_partials_f32(const float* z, int64_t ldz, int64_t n_rows, int H, float* partials, int* counts,
                                               int64_t tile0, void* stream);
wholememory_error_code_t wgamd_bn_finalize_f32(const float* partials, const int* counts, int64_t n_tiles, int H, const float* gamma,
                                               const float* beta, float eps, float momentum, float* running_mean,
                                               float* running_var, float* mean, float* var, float* rstd, float* scale, float* shift,
                                               void* stream);
wholememory_error_code_t wgamd_bn_act_linear_f32(const float* z, int64_t ldz, int64_t n_rows, int H, const float* scale,
                                                 const float* shift, const float* w2, int64_t ldw2, int N, const float* b2,
                                                 int relu_out, float* out, int64_t ldo, float* hidden_out, int64_t ld_hidden,
                                                 void* stream);
wholememory_error_code_t wgamd_bn_bwd_reduce_f32(const float* dhidden, int64_t ld_dh, const float* hidden, int64_t ld_hidden,
                                                 const float* z, int64_t ldz, int64_t n_rows, int H, const float* mean,
                                                 const float* rstd, float* partials, float* dgamma, float* dbeta, void* stream);
wholememory_error_code_t wgamd_bn_bwd_apply_f32(const float* dhidden, int64_t ld_dh, const float* hidden, int64_t ld_hidden,
                                                const float* z, int64_t ldz, int64_t n_rows, int H, const float* mean,
                                                const float* rstd, const float* gamma, const float* dgamma, const float* dbeta,
                                                float* dz, int64_t ld_dz, void* stream);

/* ---- GATv2 attention (csrc/wg_gatv2.hip): torch_geometric.nn.GATv2Conv over a sampled hop, on the TRANSFORMED rows ----------------
 *   e[k, h]  = sum_c att[h C + c] LeakyReLU(XL[j, h C + c] + XR[i, h C + c])       (k = (j -> i), j = col[k] a row of xl)
 *   alpha    = softmax over the edges of row i of e[:, h]
 *   agg[i]   = sum_k alpha[k, h] XL[j, h C : (h + 1) C]  per head                  [n_rows, H C]
 *   out[i]   = act( agg[i] + bias )  [H C wide],  or with mean  act( mean_h agg[i, h C :] + bias )  [C wide]
 * XL[j] = xl[j] (the caller's lin_l(x_src)), XR[i] = xr[xr_rows ? xr_rows[i] : i] (lin_r over the destination rows; with shared
 * weights xr = xl and xr_rows = the destinations' input rows).  The logit is not linear in the neighbour row, so there is no
 * aggregate-first form: the transformed row is read once per edge.  Self loops are ordinary entries of the CSR.  A row without
 * edges gets a zero aggregate (out = act(bias)).  alpha (optional, [E, H]) and agg (optional, [n_rows, H C] row-major) are what
 * the backward reads.  One launch; sums run in CSR order: run-to-run deterministic.  Domain: wgamd_gatv2_supported (answers on
 * the host: 1 <= H <= 8, C % 4 == 0, H C <= 256); float32, unit column stride, xl / xr / out / att / bias / agg rows 16-B aligned.
 * wgamd_gatv2_bwd_dst_f32 (destination-major, given g = dL/d agg [n_rows, ldg] and the kept alpha, agg): per edge and head
 *   dalpha = g[i, h] . XL[j, h],  de = alpha (dalpha - g[i, h] . agg[i, h])                            de [E, H]
 *   dxr[i] = sum_k de att * LeakyReLU'(XL[j] + XR[i])                                                   [n_rows, H C]
 *   datt_part[b] = sum over the 16 rows of workgroup b of de LeakyReLU(XL[j] + XR[i])                   [wgamd_gatv2_bwd_blocks, H C]
 * (datt is the sum of the partial rows, taken by the caller in a fixed order).
 * wgamd_gatv2_bwd_src_f32 (source-major over the hop's transpose: row_ptr_t / col_t = destination rows / perm = CSR edge of
 * every transposed entry, over n_src rows of xl):
 *   gx[j] (+)= sum_k (alpha[k, h] g[i, h C :] + de[k, h] att * LeakyReLU'(XL[j] + XR[i]))
 * entries added in transposed-CSR order.  No atomics in any of the three. */
int wgamd_gatv2_supported(int H, int C);
int64_t wgamd_gatv2_bwd_blocks(int64_t n_rows);
wholememory_error_code_t wgamd_gatv2_attention_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* xl, int64_t ldxl,
                                                   const float* xr, int64_t ldxr, const int64_t* xr_rows, const float* att, int H,
                                                   int C, float negative_slope, const float* bias, int relu, int mean, float* out,
                                                   int64_t ldo, float* alpha, float* agg, void* stream);
wholememory_error_code_t wgamd_gatv2_bwd_dst_f32(const int* row_ptr, const int* col, int64_t n_rows, const float* xl, int64_t ldxl,
                                                 const float* xr, int64_t ldxr, const int64_t* xr_rows, const float* att, int H, int C,
                                                 float negative_slope, const float* alpha, const float* g, int64_t ldg,
                                                 const float* agg, float* dxr, float* de, float* datt_part, void* stream);
wholememory_error_code_t wgamd_gatv2_bwd_src_f32(const int* row_ptr_t, const int* col_t, const int* perm, int64_t n_src,
                                                 const float* xl, int64_t ldxl, const float* xr, int64_t ldxr,
                                                 const int64_t* xr_rows, const float* att, int H, int C, float negative_slope,
                                                 const float* alpha, const float* de, const float* g, int64_t ldg, float* gx,
                                                 int64_t ldgx, int accumulate, void* stream);

/* ---- NormDropoutAct (csrc/wg_norm_act.hip): the row-wise block between two message-passing layers -------------------------------
 * What the reference's models put after a conv (mag_lp_mnmg.py: norm -> dropout -> relu, with the `+ lin1(x)` residual in the
 * encoder; gnn_model.py / rgcn / gin: relu -> dropout), over [n_rows, C] float32, for up to WGAMD_NORM_ACT_MAX_SEGMENTS node types
 * (segments) in ONE launch:
 *   z   = x (+ residual)                                       residual nullable
 *   y   = (z - mean) rstd * weight + bias                      WGAMD_NORM_ACT_NORM: torch.nn.LayerNorm (biased variance,
 *                                                              rstd = 1 / sqrt(var + eps)); weight, bias nullable (1, 0)
 *   y   = keep ? y / (1 - p) : 0                               p > 0 (p = 1: zeros); a dropped element is exactly 0, also
 *                                                              where y is NaN or infinite (torch's dropout: NaN * 0 = NaN)
 *   out = relu(y)                                              WGAMD_NORM_ACT_RELU
 * stats [n_rows][2] = (mean, rstd) per row is written with WGAMD_NORM_ACT_SAVE_STATS (NORM only) and read by the backward.
 * keep(r, c) <=> word (c % 4) of Philox4x32-10(key = segment seed, counter = (c / 4, r low, r high, 0)) >= floor(p 2^32): it
 * depends on (segment seed, row within the segment, c) only — not on strides, flags, the launch's other segments or how rows map
 * to lanes.  The segment seed is wgamd_norm_act_segment_seed(seed, seed_index), or `seed` itself when seed_index < 0
 * (seed_index = the segment's position in the caller's list, which keeps counting when the list is split over launches).
 * wgamd_norm_act_bwd_f32 (same segments, eps, p, seed, flags): from grad_out recomputes z, x^, y, the ReLU sign and the mask —
 * it reads neither out nor a stored mask — and writes grad_in = dz, the gradient of x AND of residual:
 *   gy = grad_out * keep / (1 - p) * [y > 0],   dz = rstd (w gy - mean_c(w gy) - x^ mean_c(w gy x^))      (NORM off: dz = gy)
 * and, with NORM and partials given, partials[b][0][:] = sum gy x^ and partials[b][1][:] = sum gy over the rows of workgroup b
 * (wgamd_norm_act_bwd_blocks(n_rows, C) rows of 2 C floats).  wgamd_norm_act_wgrad_f32 adds the partial rows in a fixed order:
 * dweight, dbias [C] (either nullable; zeros for an empty segment; a segment with neither is skipped and needs no partials).  No atomics: the same bits on every run.
 * Domain: wgamd_norm_act_supported(C) (C % 4 == 0, 4 <= C <= 1024); 1 <= n_segs <= 8, empty segments allowed; every ld >= C and a
 * multiple of 4, rows / weight / bias / partials 16-B aligned, stats 8-B aligned (WHOLEMEMORY_LOGIC_ERROR otherwise). */
#define WGAMD_NORM_ACT_MAX_SEGMENTS 8
#define WGAMD_NORM_ACT_NORM 1
#define WGAMD_NORM_ACT_RELU 2
#define WGAMD_NORM_ACT_SAVE_STATS 4
typedef struct {
  const float* x;
  int64_t ldx;
  const float* residual;
  int64_t ld_res;
  float* out;
  int64_t ldo;
  const float* weight;
  const float* bias;
  float* stats;
  int64_t n_rows;
  int C;
  int seed_index;
  /* the backward's (null / 0 in the forward) */
  const float* grad_out;
  int64_t ldg;
  float* grad_in;
  int64_t ld_gi;
  float* partials;
  /* the weight-gradient launch's */
  float* dweight;
  float* dbias;
} wgamd_norm_act_segment;
int wgamd_norm_act_supported(int C);
uint64_t wgamd_norm_act_segment_seed(uint64_t seed, int k);
int64_t wgamd_norm_act_bwd_blocks(int64_t n_rows, int C);
wholememory_error_code_t wgamd_norm_act_f32(const wgamd_norm_act_segment* segs, int n_segs, float eps, float p, uint64_t seed,
                                            int flags, void* stream);
wholememory_error_code_t wgamd_norm_act_bwd_f32(const wgamd_norm_act_segment* segs, int n_segs, float eps, float p, uint64_t seed,
                                                int flags, void* stream);
wholememory_error_code_t wgamd_norm_act_wgrad_f32(const wgamd_norm_act_segment* segs, int n_segs, void* stream);

/* ---- RowLinear (csrc/wg_row_linear.hip): a Linear over gathered rows with a row-wise epilogue, ONE launch ------------------------
 * The dense products around the reference's layers (mag_lp_mnmg.py: paper_norm(paper_lin(x)), lin1(x) on the output rows,
 * normalize(lin2(x).relu()) + x_paper; taobao / movielens: lin(x)), over n_rows rows:
 *   y   = X[i] @ weight^T + bias                               X[i] = x[ids[i]] (ids nullable: x[i]); weight [N, ldw], bias nullable
 *   y   = relu(y)                                              relu != 0
 *   z   = (y - mean) rstd * gamma + beta                       WGAMD_ROW_LINEAR_NORM_LAYER: biased variance, two-pass,
 *                                                              rstd = 1 / sqrt(var + eps); gamma, beta nullable (1, 0)
 *       = y / max(||y||_2, eps)                                WGAMD_ROW_LINEAR_NORM_L2
 *   out = z + add                                              add nullable, [n_rows, ld_add]
 * x is a table of x_dtype FLOAT, HALF or BF16 with rows ldx ELEMENTS apart; 16-bit values are converted to float32 exactly, so the
 * result is bit for bit that of the float32 table.  ids are INT or INT64 (ids_dtype; ignored when ids is null) and are not
 * range-checked.  kept_x (nullable, [n_rows, ld_kx]) receives the float32 input rows, kept_y (nullable, [n_rows, ld_ky]) the rows
 * after the ReLU and before the norm: what the backward reads.  Rows at or past n_rows are neither read from add nor written.
 * wgamd_row_linear_bwd_f32: dy [n_rows, ld_dy] = grad_out through the norm (statistics recomputed from kept_y), zero where relu
 * and kept_y <= 0; for the L2 norm with ||y|| < eps, dy = grad_out / eps.  kept_y may be null without relu and norm.  With
 * NORM_LAYER and partials given (wgamd_row_linear_bwd_blocks(n_rows, N) rows of 2 N floats) workgroup b writes partials[b][0][:]
 * = sum grad_out x^ and partials[b][1][:] = sum grad_out over its rows; wgamd_row_linear_affine_grad_f32 adds the partial rows in
 * a fixed order into dgamma, dbeta [N] (either nullable; zeros for n_rows = 0).  No atomics: the same bits on every run.
 * Domain: wgamd_row_linear_supported(K, N) (K % 4 == 0, 4 <= K <= 1024, N % 4 == 0, 4 <= N <= 256); every leading dimension a
 * multiple of 4 and at least the width; float32 rows, gamma, beta and partials 16-B aligned, 16-bit table rows 8-B aligned
 * (WHOLEMEMORY_LOGIC_ERROR otherwise; null pointers, small leading dimensions, other dtypes: WHOLEMEMORY_INVALID_INPUT).  All
 * checks come before any device call; n_rows = 0 is success without a launch. */
#define WGAMD_ROW_LINEAR_NORM_NONE 0
#define WGAMD_ROW_LINEAR_NORM_LAYER 1
#define WGAMD_ROW_LINEAR_NORM_L2 2
int wgamd_row_linear_supported(int K, int N);
int64_t wgamd_row_linear_bwd_blocks(int64_t n_rows, int N);
wholememory_error_code_t wgamd_row_linear_f32(const void* x, wholememory_dtype_t x_dtype, int64_t ldx, const void* ids,
                                              wholememory_dtype_t ids_dtype, int64_t n_rows, int K, const float* weight,
                                              int64_t ldw, int N, const float* bias, int relu, int norm, const float* gamma,
                                              const float* beta, float eps, const float* add, int64_t ld_add, float* out,
                                              int64_t ldo, float* kept_x, int64_t ld_kx, float* kept_y, int64_t ld_ky,
                                              void* stream);
wholememory_error_code_t wgamd_row_linear_bwd_f32(const float* kept_y, int64_t ld_ky, const float* grad_out, int64_t ldg,
                                                  int64_t n_rows, int N, int relu, int norm, const float* gamma, float eps,
                                                  float* dy, int64_t ld_dy, float* partials, void* stream);
wholememory_error_code_t wgamd_row_linear_affine_grad_f32(const float* partials, int64_t n_rows, int N, float* dgamma,
                                                          float* dbeta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WGAMD_EXT_H_ */
