"""Call-group iteration of a ``LinkNeighborLoader`` epoch: G mini-batches of seed EDGES at a time as one block-diagonal graph.

``LinkNeighborLoader`` samples in call groups already — negatives per batch, the endpoints of all batches de-duplicated row-wise
(``_batched_first_unique``), ONE walk over the ragged per-batch seed lists — and then cuts the result into one ``Data`` per
mini-batch.  ``loader.call_groups()`` hands the group out whole instead: a ``LinkCallGroup`` is a ``CallGroup`` (``x``,
``layer_graph(j)``, ``batch_ptr``, ... unchanged) over that walk.  The seed rows of the last layer's output are each batch's unique
endpoints in first-appearance order, so the group's ``edge_label_index`` is the batch-local one shifted by ``batch_ptr[b]`` and
costs nothing to produce; ``wholegraph_amd.nn.link_bce_with_logits(h, h, grp.edge_label_index, grp.edge_label)`` is then the loss
of all G mini-batches in one launch.  Every mini-batch inside is bit for bit what ``for batch in loader`` yields
(``to_data_list()``; tests/test_gpu_link_call_groups.py).

Typed edge seeds of a HETEROGENEOUS graph go the same way through ``loader.hetero_call_groups()``: a ``HeteroLinkCallGroup`` is a
``HeteroCallGroup`` (``x_dict``, ``layer_graph(j)``, ...) whose seeds are the unique source endpoints of the seed edges (node type
``src_t``) and their unique destination endpoints (``dst_t``; one joint list when both are one type), and row 0 / row 1 of its
``edge_label_index`` index the last layer's output of ``src_t`` / ``dst_t`` — ``nn.link_bce_with_logits(h[src_t], h[dst_t], ...)``
or ``nn.EdgeDecoder`` (tests/test_gpu_hetero_link_call_groups.py).
"""
from typing import Optional

import torch

from wholegraph_amd import graph_ops

from .call_group import CallGroup, HeteroCallGroup, _PipelinedGroups, _enqueue_hetero_walk_sizes, _enqueue_walk_sizes


def link_group_index(local: torch.Tensor, batch_ptr: torch.Tensor, n_pos: int, n_neg: int):
    """``(edge_label_index [2, G (n_pos + n_neg)], label_ptr [G + 1])`` of a link call group.  ``local`` [G, 2 (n_pos + n_neg)]:
    per mini-batch the positions of its seed edges' endpoints — sources (positives, then negatives), then destinations — in
    the batch's unique endpoint list; ``batch_ptr`` [G + 1]: the first row of every batch's list in the group numbering.  Pairs
    are batch-major, positives first inside a batch, as the per-batch loader emits them."""
    G, half = local.shape[0], n_pos + n_neg
    assert local.shape[1] == 2 * half and batch_ptr.shape[0] == G + 1
    shifted = local.to(torch.int64) + batch_ptr[:-1].to(torch.int64).view(G, 1)
    index = torch.stack([shifted[:, :half].reshape(-1), shifted[:, half:].reshape(-1)])
    label_ptr = torch.arange(G + 1, dtype=torch.int64, device=local.device) * half
    return index, label_ptr


def hetero_link_group_index(local_src: torch.Tensor, local_dst: torch.Tensor, ptr_src: torch.Tensor, ptr_dst: torch.Tensor,
                            n_pos: int, n_neg: int):
    """``(edge_label_index [2, G (n_pos + n_neg)], label_ptr [G + 1])`` of a HETEROGENEOUS link call group.  ``local_src`` /
    ``local_dst`` [G, n_pos + n_neg]: per mini-batch the positions of its seed edges' source / destination endpoints (positives,
    then negatives) in the batch's unique endpoint list of the source / destination type; ``ptr_src`` / ``ptr_dst`` [G + 1]: the
    first row of every batch's list in the group numbering of that type (one joint list when both are one type: the same
    offsets twice).  Row 0 indexes rows of the source type, row 1 rows of the destination type; pairs are batch-major, positives
    first inside a batch, as the per-batch loader emits them."""
    G, half = local_src.shape[0], n_pos + n_neg
    assert tuple(local_src.shape) == (G, half) == tuple(local_dst.shape) and ptr_src.shape[0] == G + 1 == ptr_dst.shape[0]
    index = torch.stack([(local_src.to(torch.int64) + ptr_src[:-1].to(torch.int64).view(G, 1)).reshape(-1),
                         (local_dst.to(torch.int64) + ptr_dst[:-1].to(torch.int64).view(G, 1)).reshape(-1)])
    label_ptr = torch.arange(G + 1, dtype=torch.int64, device=local_src.device) * half
    return index, label_ptr


def hetero_group_data(feature_store, outs, ctx, seed_types):
    """The mini-batches of a heterogeneous call group over per-batch seed lists of ``seed_types`` (``outs``, ``ctx``: what
    ``HeteroPygWalk.finalize_batches`` returns and leaves in ``rec["group_context"]``) as ``HeteroData``, every stored attribute
    fetched once for the group."""
    from .._compat import HeteroSamplerOutput
    from ..sampler.sampler import _group_attribute_views, build_hetero_data
    views = _group_attribute_views(feature_store, ctx)
    for j, (node, row, col, edge, nn, ne) in enumerate(outs):
        out = HeteroSamplerOutput(node=node, row=row, col=col, edge=edge,
                                  batch={t: node[t][:nn[t][0]] for t in seed_types},
                                  num_sampled_nodes={k: torch.tensor(v) for k, v in nn.items()},
                                  num_sampled_edges={k: torch.tensor(v) for k, v in ne.items()}, metadata=None)
        yield build_hetero_data(feature_store, out, views, j)


def hetero_link_data(data, edge_type, inv_src, inv_dst, input_id, n_pos: int, edge_label, mode):
    """The link keys of one heterogeneous mini-batch, on the seed edge type's store of ``data``: ``edge_label_index`` (local ids
    into ``n_id`` of the endpoint types), ``input_id``, ``batch_size``, ``edge_label`` where there is one, PyG's triplet view."""
    st = data[edge_type]
    st.edge_label_index = torch.stack([inv_src, inv_dst])
    st.input_id = input_id
    st.batch_size = n_pos
    if edge_label is not None:
        st.edge_label = edge_label
    if mode == "triplet":
        st.src_index, st.dst_pos_index, st.dst_neg_index = inv_src[:n_pos], inv_dst[:n_pos], inv_dst[n_pos:]
    return data


class LinkCallGroup(CallGroup):
    """G consecutive mini-batches of a ``LinkNeighborLoader`` epoch.  A ``CallGroup`` whose seeds are the mini-batches' unique
    seed-edge endpoints; on top of it:

    ``edge_label_index`` int64 [2, P]: the pairs of all mini-batches, batch-major, positives first inside a batch, as rows of
    the last layer's output (the ``batch_ptr`` numbering) — ``batch[edge_label_index]`` are the global endpoint ids;
    ``edge_label`` [P] (None where the per-batch loader gives none): the per-batch labels back to back;
    ``label_ptr`` int64 [G + 1]: the pairs of mini-batch b; ``input_id``: the seed-edge ids, ``n_pos`` per mini-batch;
    ``seed_time`` int64, one per seed row, batch-major (a TEMPORAL loader; None otherwise): the time every unique endpoint
    starts the walk at — the ``edge_label_time`` of the first pair of its mini-batch that names it."""

    def __init__(self, walk_result, feature_store, graph, first_batch, input_id, sizes_h, event, walk_stream, local, n_pos, n_neg,
                 edge_label_index, label_ptr, edge_label, mode, seed_time=None):
        super().__init__(walk_result, feature_store, graph, first_batch, input_id, sizes_h, event, walk_stream)
        self._local, self.n_pos, self.n_neg, self._mode, self._seed_time = local, n_pos, n_neg, mode, seed_time
        self.edge_label_index, self.label_ptr, self.edge_label = edge_label_index, label_ptr, edge_label

    def _wait(self):
        if self._ready:
            return
        super()._wait()
        if self._walk_stream is not None:     # the negatives and the de-duplication ran on the walk stream too
            main = torch.cuda.current_stream()
            for t in (self._local, self.edge_label_index, self.label_ptr, self.edge_label, self.input_id, self._seed_time):
                if t is not None:
                    t.record_stream(main)

    @property
    def seed_time(self):
        if self._seed_time is None:
            return None
        self._wait()
        return self._seed_time[:self.num_seeds]

    def to_data_list(self):
        """The G mini-batches as the ``Data`` objects ``for batch in loader`` yields (same tensors, bit for bit)."""
        from ..sampler.sampler import filter_store_from_group, group_attribute_views
        self._wait()
        outs = self._res.finalize_batches(self._graph.edge_id)
        views = group_attribute_views(self._fs, self._res.group_context)
        n_pos, n_neg = self.n_pos, self.n_neg
        half = n_pos + n_neg
        datas = []
        for j, (node, row, col, edge, nn, ne) in enumerate(outs):
            d = filter_store_from_group(self._fs, views, j, node, row, col, edge)
            d.n_id, d.e_id = node, edge
            d.num_sampled_nodes, d.num_sampled_edges = torch.tensor(nn), torch.tensor(ne)
            d.input_id = self.input_id[j * n_pos:(j + 1) * n_pos]
            d.batch_size = n_pos
            inverse = self._local[j]
            d.edge_label_index = torch.stack([inverse[:half], inverse[half:]])
            if self.edge_label is not None:
                d.edge_label = self.edge_label[j * half:(j + 1) * half]
            if self._mode == "triplet":
                d.src_index, d.dst_pos_index = inverse[:n_pos], inverse[half:half + n_pos]
                neg = inverse[half + n_pos:]
                d.dst_neg_index = neg.view(-1, n_pos).t() if n_neg % n_pos == 0 and n_neg > n_pos else neg
            datas.append(d)
        return datas


class LinkCallGroupIterator(_PipelinedGroups):
    """The call groups of a ``LinkNeighborLoader`` epoch.  ``batch_edges(b)`` is the loader's own per-batch recipe — the seed-edge
    ids of mini-batch b, its endpoints with the negatives drawn by the batch's generator, its labels — so the epoch is the one
    ``iter(loader)`` walks; with ``overlap`` the negatives, the de-duplication and the walk of group g + 1 are enqueued on the
    iterator's own stream before group g is handed out."""

    def __init__(self, data, sampler, batch_edges, n_edges: int, batch_size: int, batches_per_group: int, num_nodes: int,
                 random_state: int, mode: Optional[str], device, overlap: bool = True):
        self._fs, self._gs = data
        self._smp, self._batch_edges, self._B, self._rs = sampler, batch_edges, int(batch_size), int(random_state)
        self._num_nodes, self._mode = int(num_nodes), mode
        n_full, G = n_edges // self._B, max(1, int(batches_per_group))
        # (first batch, batches): the full batches in groups of G, then the ragged last batch as a one-batch group over its own list
        plan = [(b, min(G, n_full - b)) for b in range(0, n_full, G)]
        if n_edges % self._B:
            plan.append((n_full, 1))
        self._pipeline(plan, device, overlap)

    def _launch(self, i):
        from ..sampler.sampler import hop_seed
        from .link_loader import _batched_first_unique
        if i >= len(self._plan):
            return None
        b0, g = self._plan[i]
        smp = self._smp
        rs = [[hop_seed(self._rs + b0 + j, k) for j in range(g)] for k in range(len(smp.fanout))]

        def enqueue():
            ids, ends, labels, times, n_pos, n_neg = [], [], [], [], 0, 0
            for j in range(g):
                input_id, src_all, dst_all, n_neg, label, t_all = self._batch_edges(b0 + j, self._rs + b0 + j)
                n_pos = input_id.numel()
                ids.append(input_id)
                ends.append(torch.cat([src_all, dst_all]))
                labels.append(label)
                times.append(t_all)
            ends = torch.stack(ends)                  # [g, 2 (n_pos + n_neg)]: the batches of a group are equally long
            S = ends.shape[1]
            uniq, seg, batch, local = _batched_first_unique(ends, self._num_nodes)
            seed_time = None
            if smp.temporal:   # both endpoints of pair i start at time i; a unique endpoint at the time of its first pair
                t = torch.stack(times)
                seed_time = graph_ops.rows_first_values(local, seg, torch.cat([t, t], 1))
            walk = smp._call_group_walk(S, g)
            res = walk.run(uniq.to(smp.graph.col.dtype).contiguous(), rs, seg, batch, seed_time=seed_time)
            edge_label = None if labels[0] is None else torch.cat(labels)
            index, label_ptr = link_group_index(local, seg, n_pos, n_neg)
            return (res,) + _enqueue_walk_sizes(res) + (torch.cat(ids), local, n_pos, n_neg, index, label_ptr, edge_label, seed_time)

        res, sizes_h, ev, input_id, local, n_pos, n_neg, index, label_ptr, edge_label, seed_time = self._on_walk_stream(enqueue)
        return LinkCallGroup(res, self._fs, smp.graph, b0, input_id, sizes_h, ev, self._stream, local, n_pos, n_neg, index, label_ptr,
                             edge_label, self._mode, seed_time)


class HeteroLinkCallGroup(HeteroCallGroup):
    """G consecutive mini-batches of a ``LinkNeighborLoader`` epoch over a HETEROGENEOUS graph.  A ``HeteroCallGroup`` (``n_id``,
    ``node_ptr``, ``x_dict``, ``edge_attr``, ``layer_graph(j)``, ``num_sampled_*`` unchanged) whose seeds are the mini-batches'
    unique seed-edge endpoints: the sources seed ``src_t``, the destinations ``dst_t`` (one joint list when both are one type).

    ``edge_type``; ``seed_types`` = (src_t, dst_t); ``seed_type`` = src_t;
    ``batch_ptr_dict`` {t: int32 [G + 1]} for the seed types: the rows of mini-batch b's unique endpoints of type t in the last
    layer's output of type t (level 0 of the walk, batch-major); ``batch_ptr`` is the source type's; ``num_seeds_dict``;
    ``edge_label_index`` int64 [2, P]: row 0 indexes rows of ``out[src_t]``, row 1 rows of ``out[dst_t]`` — batch-major, positives
    first inside a batch; ``n_id[t][edge_label_index[i]]`` are the global endpoint ids;
    ``edge_label`` [P] (None where the per-batch loader gives none), ``label_ptr`` int64 [G + 1], ``input_id``, ``n_pos``, ``n_neg``;
    ``seed_time_dict`` {t: int64, one per seed row of type t, batch-major} (a TEMPORAL loader; None otherwise): the time every
    unique endpoint starts the walk at — the ``edge_label_time`` of the first pair of its mini-batch that names it."""

    def __init__(self, rec, walk, feature_store, edge_type, first_batch, input_id, sizes_h, event, walk_stream, cseg, batch_ptr_dict,
                 local_src, local_dst, n_pos, n_neg, edge_label_index, label_ptr, edge_label, mode, seed_time=None):
        super().__init__(rec, walk, feature_store, edge_type[0], first_batch, input_id, sizes_h, event, walk_stream, cseg)
        self.edge_type, self.seed_types = tuple(edge_type), (edge_type[0], edge_type[2])
        self.batch_ptr_dict = batch_ptr_dict
        self._local_src, self._local_dst, self.n_pos, self.n_neg, self._mode = local_src, local_dst, n_pos, n_neg, mode
        self.edge_label_index, self.label_ptr, self.edge_label = edge_label_index, label_ptr, edge_label
        self._seed_time = seed_time

    @property
    def seed_time_dict(self):
        if self._seed_time is None:
            return None
        self._wait()
        return {t: v[:self.num_seeds_dict[t]] for t, v in self._seed_time.items()}

    def _wait(self):
        if self._ready:
            return
        super()._wait()
        self.num_seeds_dict = {t: self._n_level[0][t] for t in self.seed_types}
        if self._walk_stream is not None:     # the negatives and the de-duplications ran on the walk stream too
            main = torch.cuda.current_stream()
            for t in (self._local_src, self._local_dst, self.edge_label_index, self.label_ptr, self.edge_label, self.input_id,
                      *self.batch_ptr_dict.values(), *(self._seed_time or {}).values()):
                if t is not None:
                    t.record_stream(main)

    def to_data_list(self):
        """The G mini-batches as the ``HeteroData`` objects ``for batch in loader`` yields (same tensors, bit for bit)."""
        self._wait()
        outs = self._walk.finalize_batches(self._rec)
        n_pos, half = self.n_pos, self.n_pos + self.n_neg
        datas = []
        for j, d in enumerate(hetero_group_data(self._fs, outs, self._rec["group_context"], list(self.batch_ptr_dict))):
            label = None if self.edge_label is None else self.edge_label[j * half:(j + 1) * half]
            datas.append(hetero_link_data(d, self.edge_type, self._local_src[j], self._local_dst[j],
                                          self.input_id[j * n_pos:(j + 1) * n_pos], n_pos, label, self._mode))
        return datas


class HeteroLinkCallGroupIterator(_PipelinedGroups):
    """The call groups of a ``LinkNeighborLoader`` epoch over a heterogeneous graph (``LinkCallGroupIterator`` for typed edge
    seeds): per group the negatives of its batches, one row-wise de-duplication per endpoint type (one over the joint list when
    both are one type) and ONE walk over the ragged per-batch seed lists — ``HeteroNeighborSampler.sample_seed_lists``'s walk and
    seeds — all on the iterator's own stream with ``overlap``."""

    def __init__(self, data, sampler, batch_edges, n_edges: int, batch_size: int, batches_per_group: int, edge_type, num_src: int,
                 num_dst: int, random_state: int, mode: Optional[str], device, overlap: bool = True):
        self._fs, self._gs = data
        self._smp, self._batch_edges, self._B, self._rs = sampler, batch_edges, int(batch_size), int(random_state)
        self._etype, self._num_src, self._num_dst, self._mode = tuple(edge_type), int(num_src), int(num_dst), mode
        n_full, G = n_edges // self._B, max(1, int(batches_per_group))
        plan = [(b, min(G, n_full - b)) for b in range(0, n_full, G)]
        if n_edges % self._B:       # the ragged last batch: a one-batch group over its own lists
            plan.append((n_full, 1))
        self._pipeline(plan, device, overlap)

    def _launch(self, i):
        from ..sampler.sampler import _as_i64, hop_seed
        from .link_loader import _batched_first_unique
        if i >= len(self._plan):
            return None
        b0, g = self._plan[i]
        smp, (src_t, _, dst_t) = self._smp, self._etype
        H, n_et = len(next(iter(smp.fanout.values()))), len(smp.graphs)
        rs = torch.tensor([[_as_i64(hop_seed(self._rs + b0 + j, k)) for j in range(g)] for k in range(H * n_et)], dtype=torch.int64)

        def enqueue():
            ids, srcs, dsts, labels, times, n_pos, n_neg = [], [], [], [], [], 0, 0
            for j in range(g):
                input_id, src_all, dst_all, n_neg, label, t_all = self._batch_edges(b0 + j, self._rs + b0 + j)
                n_pos = input_id.numel()
                ids.append(input_id)
                srcs.append(src_all)
                dsts.append(dst_all)
                labels.append(label)
                times.append(t_all)
            srcs, dsts = torch.stack(srcs), torch.stack(dsts)       # [g, n_pos + n_neg] each: the batches of a group are equally long
            half = srcs.shape[1]
            if src_t == dst_t:
                uniq, seg, batch, local = _batched_first_unique(torch.cat([srcs, dsts], 1), self._num_src)
                lists = {src_t: (uniq, seg, batch)}
                local_src, local_dst = local[:, :half], local[:, half:]
            else:
                us, sseg, sbatch, local_src = _batched_first_unique(srcs, self._num_src)
                ud, dseg, dbatch, local_dst = _batched_first_unique(dsts, self._num_dst)
                lists = {src_t: (us, sseg, sbatch), dst_t: (ud, dseg, dbatch)}
            seed_time = None
            if smp.temporal:   # both endpoints of pair i start at time i; a unique endpoint at the time of its first pair
                t = torch.stack(times)
                if src_t == dst_t:
                    seed_time = {src_t: graph_ops.rows_first_values(local, seg, torch.cat([t, t], 1))}
                else:
                    seed_time = {src_t: graph_ops.rows_first_values(local_src, sseg, t),
                                 dst_t: graph_ops.rows_first_values(local_dst, dseg, t)}
                lists = {k: v + (seed_time[k],) for k, v in lists.items()}
            walk = smp._call_group_walk(max(int(v[0].shape[0]) for v in lists.values()) // g or 1, g)
            rec = walk.run(None, None, rs, seed_lists=lists)
            sizes_h, ev, cseg = _enqueue_hetero_walk_sizes(rec, walk, src_t)
            ptrs = {t: v[1] for t, v in lists.items()}
            index, label_ptr = hetero_link_group_index(local_src, local_dst, ptrs[src_t], ptrs[dst_t], n_pos, n_neg)
            edge_label = None if labels[0] is None else torch.cat(labels)
            return (rec, walk, sizes_h, ev, cseg, ptrs, torch.cat(ids), local_src, local_dst, n_pos, n_neg, index, label_ptr, edge_label,
                    seed_time)

        rec, walk, sizes_h, ev, cseg, ptrs, input_id, local_src, local_dst, n_pos, n_neg, index, label_ptr, edge_label, seed_time = \
            self._on_walk_stream(enqueue)
        return HeteroLinkCallGroup(rec, walk, self._fs, self._etype, b0, input_id, sizes_h, ev, self._stream, cseg, ptrs, local_src,
                                   local_dst, n_pos, n_neg, index, label_ptr, edge_label, self._mode, seed_time)
