"""The conv layers of a mini-batch GNN on the sampler's per-hop CSR (HIP kernels of ``include/wgamd_ext.h``), with PyG's class
names, parameter names and maths, so they drop into the reference's models (pylibwholegraph/torch/gnn_model.py:25-59,119-125,
178-199 builds ``SAGEConv`` / ``GATConv`` and feeds them ``(x, x_target)`` plus the hop's ``[csr_row_ptr, csr_col_ind]`` or COO)
and into its cugraph-pyg examples.  Six layers run ONE kernel per hop of a call group's ``LayerGraph``, forward and backward
(each an autograd Function over the hops): ``SAGEConv``, ``GCNConv``, ``RGCNConv``, ``TransformerConv``, ``GINConv``, and
``HeteroConv`` over SAGEConv relations (one kernel per hop and destination type).  ``GATConv`` and ``HeteroConv`` over GATConv
relations are aggregate kernels with a dense tail.  ``GATv2Conv`` is two library GEMMs and ONE attention kernel per hop on
the transformed rows (its logit is not linear in the neighbour row: no aggregate-first form).  ``NormDropoutAct`` /
``HeteroNormDropoutAct`` are what the reference's models put BETWEEN two layers (residual add, LayerNorm, dropout, ReLU): one
launch forward and two backward for all node types of a layer.  ``RowLinear`` is the dense product AROUND the layers (input
projection over the stored features, skip term, normalised tail, plain heads): gathered rows times a weight with a row-wise
epilogue, one launch.

Order of the file: ctypes helpers and the plumbing the one-kernel layers share; the SAGE-era kernel wrappers, derived-weight
caches and GAT kernel wrappers; graph forms (``_single_hop``, ``LazyRows``, ``HopGraph``, ``LayerGraph``) and the helpers that
walk a layer graph; then a section per layer — SAGE and GAT, GCN, RGCN, transformer, GIN, GATv2, heterogeneous, NormDropoutAct, RowLinear —
each with its kernel wrappers, its autograd Function(s) and its module.

Shared by the one-kernel layers, so that they cannot drift apart: ``_hop_args`` (the eight leading arguments of a launch over a
hop, with their checks), ``_out_rows`` (a launch's output: the caller's or a fresh one), ``_hops`` / ``_sum_over_hops`` (a layer
graph's hops with their row and edge slices; the sum of the hops' input gradients), ``_layer_input`` / ``_kernel_rows_ok`` (a
tensor or ``LazyRows`` input as the kernels read it), ``_padded_wt`` / ``_pad_cols`` (the operands of an input gradient run as
the layer kernel over ``HopGraph.transposed``), ``_dense_wgrad`` (``gcn_wgrad`` per hop: dW, db of a dense product), and
``_released`` (the RuntimeError of a second backward through a layer whose kept tensors the first one released).

Shared by ``GATConv`` and the routes of ``HeteroConv`` over a call group: ``_table_through_ids`` (a ``LazyRows`` input the kernels
may read in place through its node list) with ``_terms_by_id`` (whose attention terms are then the table's rows') and
``_refuse_lazy_table_grad``; ``_sum_of`` (the relations' biases or root weights added up); ``_relation_groups`` /
``_group_outputs`` / ``_place_rows`` (a heterogeneous layer graph's relations per (hop, destination type), the per-type float32
outputs and a group's rows placed in them).  Shared by every layer: ``_derived`` (every derived form of the weights, keyed on the
parameters it is built from).
"""
import ctypes
import math
from typing import Optional, Tuple, Union

import torch

from . import _lib as L
from .env import get_stream, torch_dtype_to_wm


_X16 = (torch.float16, torch.bfloat16)      # feature tables the bf16x3 SAGE layer kernel reads as they are (wgamd_sage_layer_fused_bf16x3_x)


def _ids_code(x, src_ids) -> int:
    """``src_ids_dtype`` of the layer kernels: the ids' integer type, or WGAMD_IDS_BYTE_OFFSETS when ``x`` is the address space of
    a peer-mapped table (``MappedTable``) and ``src_ids`` holds byte offsets into it."""
    return L.IDS_BYTE_OFFSETS if getattr(x, "byte_offset_ids", False) else torch_dtype_to_wm(src_ids.dtype)


def _ids_args(x, src_ids):
    """``(src_ids, src_ids_dtype)`` arguments of the layer kernels: null when ``x`` is read by row."""
    ids_ptr, ids_dt = None, 0
    if src_ids is not None:
        assert src_ids.is_contiguous()
        ids_ptr, ids_dt = src_ids.data_ptr(), _ids_code(x, src_ids)
    return ids_ptr, ids_dt


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nonempty(t, dtype):
    """``t``, or a one-element buffer when ``t`` is empty (the kernels take no null pointer for a hop's edge arrays)."""
    return t if t.numel() > 0 else torch.zeros(1, dtype=dtype, device=t.device)


def _check_csr(row_ptr, col):
    assert row_ptr.dtype == torch.int32 and col.dtype == torch.int32, "per-hop CSR is int32 (sampler output)"
    assert row_ptr.is_cuda and col.is_cuda and row_ptr.is_contiguous() and col.is_contiguous()


def _hop_args(row_ptr, col, x, src_ids):
    """The eight leading arguments of a layer kernel over one hop: ``row_ptr, col, n_rows, x, ldx, F, src_ids, src_ids_dtype``
    (``x`` float32 rows with unit column stride, read by row or through ``src_ids``; an empty ``col`` goes in as one element)."""
    _check_csr(row_ptr, col)
    assert x.dtype == torch.float32 and x.stride(1) == 1
    return (row_ptr.data_ptr(), _nonempty(col, torch.int32).data_ptr(), row_ptr.shape[0] - 1, x.data_ptr(), x.stride(0),
            x.shape[1]) + _ids_args(x, src_ids)


def _out_rows(out, n_rows: int, width: int, device):
    """A launch's float32 ``[n_rows, width]`` output: the caller's ``out`` (checked), or a fresh buffer."""
    if out is None:
        out = torch.empty((n_rows, width), dtype=torch.float32, device=device)
    assert out.shape == (n_rows, width) and out.stride(1) == 1
    return out


def _padded_wt(weight, Nq: int):
    """``weight^T`` ([N, F] -> [F, Nq]), zero columns from N up: the weight of a layer kernel run over the transposed hop."""
    N, F_ = weight.shape
    wt = torch.zeros((F_, Nq), dtype=torch.float32, device=weight.device)
    wt[:, :N] = weight.detach().t()
    return wt


def _pad_cols(g, Nq: int):
    """``g`` [n, N] with zero columns up to ``Nq`` (``g`` itself when it is that wide already)."""
    N = g.shape[1]
    if Nq == N:
        return g
    gq = torch.zeros((g.shape[0], Nq), dtype=torch.float32, device=g.device)
    gq[:, :N] = g
    return gq


def _released(kept, layer_name: str, what: str, advice: str = ""):
    """RuntimeError on a second backward through a one-kernel layer: what its forward kept (``kept``: None once it is gone) is
    released by the first backward pass whatever retain_graph says, and autograd's own message covers saved tensors only."""
    if kept is None:
        raise RuntimeError("wholegraph_amd.nn.%s: backward through this layer a second time — its kept %s were released by the first "
                           "backward pass (retain_graph=True is not supported by the one-kernel layer%s)" % (layer_name, what, advice))


def spmm_csr_forward(row_ptr, col, x, mean=True, src_ids=None, out=None):
    """out[i] = mean/sum_{e in row i} x[src(e)], src(e) = col[e] or src_ids[col[e]] (fused fetch)."""
    _check_csr(row_ptr, col)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    n_rows = row_ptr.shape[0] - 1
    if out is None:
        out = torch.empty((n_rows, x.shape[1]), dtype=torch.float32, device=x.device)
    ids_ptr, ids_dt = None, 0
    if src_ids is not None:
        assert src_ids.is_contiguous()
        ids_ptr, ids_dt = src_ids.data_ptr(), torch_dtype_to_wm(src_ids.dtype)
    L.check(L.lib().wgamd_spmm_csr_f32(row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0),
                                       x.shape[1], ids_ptr, ids_dt, int(bool(mean)), out.data_ptr(),
                                       out.stride(0), get_stream()), "wgamd_spmm_csr_f32")
    return out


def sage_aggregate_forward(row_ptr, col, x, self_rows, mean=True):
    """-> [n_rows, 2F] = [ mean_{e in row i} x[col[e]] | x[self_rows[i]] ]  (one kernel; feeds ONE GEMM with
    the concatenated weight [W_l | W_r])."""
    _check_csr(row_ptr, col)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    assert self_rows.dtype == torch.int64 and self_rows.is_contiguous()
    n_rows, F_ = row_ptr.shape[0] - 1, x.shape[1]
    assert self_rows.shape[0] == n_rows
    out = torch.empty((n_rows, 2 * F_), dtype=torch.float32, device=x.device)
    L.check(L.lib().wgamd_sage_aggregate_f32(row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0), F_,
                                             self_rows.data_ptr(), int(bool(mean)), out.data_ptr(), out.stride(0),
                                             get_stream()), "wgamd_sage_aggregate_f32")
    return out


def sage_aggregate_fetch_forward(row_ptr, col, table, src_ids, self_rows, mean=True):
    """``sage_aggregate_forward`` with the feature fetch fused in: ``table`` is the global feature table and
    ``src_ids`` the batch's local->global map, so ``x = table[src_ids]`` is never written to HBM."""
    _check_csr(row_ptr, col)
    assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
    assert self_rows.dtype == torch.int64 and self_rows.is_contiguous() and src_ids.is_contiguous()
    n_rows, F_ = row_ptr.shape[0] - 1, table.shape[1]
    out = torch.empty((n_rows, 2 * F_), dtype=torch.float32, device=table.device)
    L.check(L.lib().wgamd_sage_aggregate_fetch_f32(
        row_ptr.data_ptr(), col.data_ptr(), n_rows, table.data_ptr(), table.stride(0), F_, src_ids.data_ptr(),
        torch_dtype_to_wm(src_ids.dtype), self_rows.data_ptr(), int(bool(mean)), out.data_ptr(), out.stride(0),
        get_stream()), "wgamd_sage_aggregate_fetch_f32")
    return out


_FUSED_PRECISION = "bf16x3"      # "bf16x3": 3-way bf16 split of both operands on the bf16 matrix pipe (fp32-class accuracy,
#                                  HBM-bound); "f32": exact fp32 MFMA (v_mfma_f32_16x16x4_f32, bound by the fp32 matrix rate)


def sage_layer_fused_precision() -> str:
    return _FUSED_PRECISION


def set_sage_layer_fused_precision(mode: str) -> None:
    global _FUSED_PRECISION
    assert mode in ("bf16x3", "f32")
    _FUSED_PRECISION = mode


def _pick_precision(F_: int, N: int, precision) -> str:
    mode = precision or _FUSED_PRECISION
    if mode == "bf16x3" and not L.lib().wgamd_sage_layer_bf16x3_supported(F_, _padded_width(N)):
        mode = "f32"
    return mode


def _padded_width(N: int) -> int:
    """Output width the one-kernel layer runs at: its consumer waves own 64 columns each, so N is rounded up to 64, 128 or
    256 with zero weight columns (a 47-class head runs as N = 64; the caller sees the first N columns)."""
    return 64 if N <= 64 else 128 if N <= 128 else 256


def sage_layer_fused_supported(F_: int, N: int) -> bool:
    """Shapes the one-kernel SAGE layer is built for (include/wgamd_ext.h); N is padded to 64 / 128 / 256 on the way in."""
    return F_ % 4 == 0 and 0 < F_ <= 256 and 0 < N <= 256


def sage_layer_fused_preferred(F_: int, N: int) -> bool:
    """Shapes where the one-kernel layer beats aggregate kernel + library GEMM.  bf16x3 kernel: every shape it supports,
    a padded head included (the 47-class layer of the products model runs as N = 64, since round 12 with four multiplying
    waves of one 32 x 32 accumulator each; with one multiplying wave per CU the round-3 half-tile kernel took 0.38 ms
    against 0.54 ms for aggregate + GEMM at 196 k rows, 256 -> 64; 0.043 against 0.052 at 16 k rows; the round-2 kernel lost there, 0.46 against 0.20 at 65 k rows).  fp32-MFMA kernel: only when two operand
    tiles fit the 160 KB of LDS and the width needs no padding."""
    if not sage_layer_fused_supported(F_, N):
        return False
    if _FUSED_PRECISION == "bf16x3" and L.lib().wgamd_sage_layer_bf16x3_supported(F_, _padded_width(N)):
        return True
    return N == _padded_width(N) and F_ <= 152


# ---- derived-weight caches and HIP-graph capture ---------------------------------------------------------------------------
# The transposed / padded / stacked / folded / bf16-split forms of a layer's weights all come from `_derived`, the one place
# that knows the rule: a form is kept for as long as every parameter it is built from has the version, address and device it had,
# and no `bump_weight_generation` happened since.  A captured training step (cugraph_pyg_amd.loader.PerBatchStep) updates the
# weights INSIDE the graph: Python does not run on a replay, so (a) while a stream is capturing the derived forms are rebuilt
# unconditionally — their kernels become part of the graph and run on every replay — and nothing is read or stored, and (b)
# every replay bumps `_weights_gen`, which is part of every key, so eager code that follows a replay never sees a form derived
# from the weights of an earlier step.  The per-graph forms of a hop (`HopGraph.with_self_loops`, `.transposed`) are keyed on
# `_graph_epoch()` instead.
_weights_gen = 0
_capture_epoch = 0       # bumped by begin_capture(): per-capture caches (a hop's transpose) are keyed on it


def begin_capture():
    """Call right before capturing a HIP graph that runs layers over fixed, refilled graph buffers."""
    global _capture_epoch
    _capture_epoch += 1


def bump_weight_generation():
    """Invalidate every cached derived weight (call after the weights changed behind autograd's back, e.g. a graph replay)."""
    global _weights_gen
    _weights_gen += 1


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _refuse_capture(layer, caches: str):
    """RuntimeError under HIP-graph capture for a layer (a module, or its name) that keeps ``caches`` in Python (derived weights against the parameters'
    versions, or per-graph forms against the graph object): a replayed graph would keep using the ones of the capture."""
    if _capturing():
        raise RuntimeError("wholegraph_amd.nn.%s is not supported under HIP-graph capture (loader.PerBatchStep): its %s are not "
                           "capture-safe; SAGEConv layers are" % (layer if isinstance(layer, str) else type(layer).__name__, caches))


def _graph_epoch() -> int:
    """Key of a hop's per-graph forms: under HIP-graph capture the hop's arrays are fixed buffers refilled before every replay,
    so the forms are made once per capture (``begin_capture``) and become part of the graph; 0 in eager code."""
    return _capture_epoch if _capturing() else 0


def _detached(value):
    """``value`` without autograd history and never a ``Parameter``: tensors detached, also inside a tuple or list."""
    if torch.is_tensor(value):
        return value.detach()
    if isinstance(value, (tuple, list)):
        return type(value)(_detached(v) for v in value)
    return value


def _derived(holder, name, params, build, extra=(), grad=False):
    """``build()``: a form of the tensors ``params`` (None entries allowed) that the kernels read, kept on ``holder`` (a module
    or a tensor) under ``name`` — the rule of the comment above.  A hit returns the stored object itself.  A miss runs ``build``
    without autograd and stores the detached result; under capture it is built, never read or stored.  ``grad``: ``build()``
    under autograd, nothing kept.  A holder that takes no attribute (a tensor subclass without ``__dict__``) builds on every call."""
    if grad:
        with torch.enable_grad():
            return build()
    eager = not _capturing()
    if eager:
        key = (tuple(None if p is None else (p._version, p.data_ptr(), p.device) for p in params), extra, _weights_gen)
        store = getattr(holder, "_wgamd_derived", None)
        if store is not None:
            hit = store.get(name)
            if hit is not None and hit[0] == key:
                return hit[1]
    with torch.no_grad():
        value = _detached(build())
    if eager:
        if store is None:
            store = {}
            try:
                holder._wgamd_derived = store
            except AttributeError:
                pass
        store[name] = (key, value)
    return value


def _padded_head(w_t: torch.Tensor, bias, Np: int):
    """``w_t`` [2F, N] and ``bias`` [N] with zero columns up to Np, kept on the weight tensor like its planes."""
    def build():
        wp = torch.zeros((w_t.shape[0], Np), dtype=w_t.dtype, device=w_t.device)
        wp[:, :w_t.shape[1]] = w_t
        bp = None
        if bias is not None:
            bp = torch.zeros(Np, dtype=bias.dtype, device=bias.device)
            bp[:bias.shape[0]] = bias
        return wp, bp
    return _derived(w_t, "padded", (w_t, bias), build, extra=Np)


def sage_weight_planes(w_t: torch.Tensor) -> torch.Tensor:
    """``w_t`` [2F, N] fp32 -> the three bf16 planes ``wgamd_sage_layer_fused_bf16x3`` multiplies with (exact 3-way split:
    hi + mid + lo == w).  Kept ON the weight tensor object (``_derived``), so a layer pays for the split once per optimizer
    step and the cache can never outlive (or be confused with another tensor at) the same address."""
    def build():
        K, N = w_t.shape
        planes = torch.empty(L.lib().wgamd_sage_weight_planes_bytes(K, N), dtype=torch.uint8, device=w_t.device)
        L.check(L.lib().wgamd_sage_split_weight_bf16x3(w_t.data_ptr(), w_t.stride(0), K, N, planes.data_ptr(), get_stream()),
                "wgamd_sage_split_weight_bf16x3")
        return planes
    return _derived(w_t, "planes", (w_t,), build)


SAGE_FULL_TILES = 2          # WGAMD_SAGE_FULL_TILES (include/wgamd_ext.h): or-ed into the relu argument of a small launch
_SAGE_SMALL_ROWS = 8192


def sage_layer_small_launch(F_: int, n_rows: int) -> bool:
    """A launch of one mini-batch's rows at a width whose throughput shape is 64-row half tiles (F > 148): whole 32-row tiles
    give it twice the workgroups, each with half the serial chain of row fetches (47 -> 30 us for 1.2 k rows at F = 256)."""
    return 0 < n_rows <= _SAGE_SMALL_ROWS and bool(L.lib().wgamd_sage_layer_uses_half_tiles(int(F_)))


def sage_layer_planes(w_l: torch.Tensor, w_r: torch.Tensor, bias, Np: int, full_tiles: bool = False):
    """``(planes, padded bias, N, full_tiles)`` of a layer straight from its ``torch.nn.Linear`` parameters in ONE launch
    (``wgamd_sage_layer_weight_planes``) — what ``sage_layer_fused_forward(prepared=...)`` takes instead of deriving the
    transposed / padded / split forms with half a dozen framework launches.  Not cached: made for captured training steps,
    whose weights change on every replay."""
    N, F_ = w_l.shape
    planes = torch.empty(L.lib().wgamd_sage_weight_planes_bytes(2 * F_, Np), dtype=torch.uint8, device=w_l.device)
    bias_p = torch.empty(Np, dtype=torch.float32, device=w_l.device) if (bias is not None or Np != N) else None
    L.check(L.lib().wgamd_sage_layer_weight_planes(w_l.data_ptr(), w_l.stride(0), w_r.data_ptr(), w_r.stride(0),
                                                   None if bias is None else bias.data_ptr(), F_, N, Np, planes.data_ptr(),
                                                   None if bias_p is None else bias_p.data_ptr(), int(bool(full_tiles)), get_stream()),
            "wgamd_sage_layer_weight_planes")
    return planes, bias_p, N, bool(full_tiles)


def sage_layer_fused_forward(row_ptr, col, x, self_rows, w_t, bias=None, relu=False, mean=True, src_ids=None, out=None,
                             precision=None, agg_out=None, prepared=None):
    """A whole SAGEConv layer over a sampled hop in ONE kernel: ``act([mean_j X[col_j] | X[self_i]] @ w_t + bias)`` with
    ``X[r] = x[src_ids[r]]`` when ``src_ids`` is given (``x`` is then the global feature table: the feature fetch is fused
    in too).  ``w_t`` = ``cat([W_l, W_r], 1).t()`` ([2F, N], contiguous).  The ``[n_rows, 2F]`` operand never leaves LDS.
    ``precision``: "bf16x3" (default where the shape allows) or "f32" — see ``_FUSED_PRECISION``.
    ``agg_out`` ([n_rows, F] fp32, training): the launch also keeps the aggregate half of its operand there
    (``wgamd_sage_layer_fused_bf16x3_train``; same bits in ``out``) — needs ``sage_layer_train_supported``.
    ``x`` may be ``torch.float16`` / ``torch.bfloat16`` on the bf16x3 route (``wgamd_sage_layer_fused_bf16x3_x``: rows 8-B
    aligned, read by row or through int32 / int64 ids): every stored value becomes fp32 exactly as it is read, ``out`` and
    ``agg_out`` are float32 and bit for bit those of the same call on ``x.float()``.  The fp32-MFMA route refuses such an ``x``."""
    _check_csr(row_ptr, col)
    x16 = x.dtype in _X16
    assert (x.dtype == torch.float32 or x16) and x.dim() == 2 and x.stride(1) == 1
    assert self_rows.dtype == torch.int64 and self_rows.is_contiguous()
    if prepared is not None:      # (planes, padded bias, N) of sage_layer_planes: the bf16x3 kernel's operand, ready made
        n_rows, F_, N = row_ptr.shape[0] - 1, x.shape[1], prepared[2]
        bias = prepared[1]
    else:
        assert w_t.dtype == torch.float32 and w_t.dim() == 2 and w_t.stride(1) == 1 and w_t.shape[0] == 2 * x.shape[1]
        n_rows, F_, N = row_ptr.shape[0] - 1, x.shape[1], w_t.shape[1]
    Np = _padded_width(N) if sage_layer_fused_supported(F_, N) else N
    user_out = None
    if Np != N:
        # zero weight columns / bias entries up to the width the kernel runs at (kept on the weight like its planes; a
        # ``prepared`` operand is padded already); the kernel then WRITES Np columns per row.  A caller's `out` is written in
        # place only when it is the [:, :N] view of an explicit [n_rows, Np] scratch (row stride == Np: columns N..Np-1 are the
        # caller's padding by construction); any other `out` is filled from a temporary, so neither a wider buffer's own
        # columns are overwritten nor a narrower one silently dropped.
        if prepared is None:
            w_t, bias = _padded_head(w_t, bias, Np)
        if out is not None and out.stride(0) != Np:
            assert out.shape == (n_rows, N) and out.dtype == torch.float32, "out must be float32 [n_rows, N]"
            user_out, out = out, None
    if out is None:
        out = torch.empty((n_rows, Np), dtype=torch.float32, device=x.device)[:, :N]
    assert out.shape == (n_rows, N) and out.dtype == torch.float32 and out.stride(1) == 1

    N = Np
    ids_ptr, ids_dt = _ids_args(x, src_ids)
    # (an edge-less hop: an empty tensor's null pointer is refused by the entry points; every row is empty, so the stand-in is not read)
    col_ptr = _nonempty(col, torch.int32).data_ptr()
    # the route, decided once (the bf16x3 kernel's epilogue stores 16 B per lane: rows of `out` 16-B aligned)
    bf16x3 = (sage_layer_fused_supported(F_, N) and _pick_precision(F_, N, precision) == "bf16x3"
              and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0)
    if x16 and ids_dt == L.IDS_BYTE_OFFSETS:
        raise ValueError("a peer-mapped table (byte-offset ids) is read as float32 rows only, not as %s" % x.dtype)
    if prepared is not None and not bf16x3:
        raise ValueError("prepared: the operand of sage_layer_planes is read by the bf16x3 layer kernel only (precision=%r, F=%d, "
                         "N=%d), which needs the rows of out 16-B aligned (out.stride(0) %% 4 == 0 and out.data_ptr() %% 16 == 0)"
                         % (precision or _FUSED_PRECISION, F_, N))
    if x16 and not bf16x3:
        raise ValueError("a %s x is read by the bf16x3 layer kernel only (precision=%r, F=%d, N=%d): pass x.float()"
                         % (x.dtype, precision or _FUSED_PRECISION, F_, N))
    assert ids_dt != L.IDS_BYTE_OFFSETS or bf16x3, "a peer-mapped table is read by the bf16x3 layer kernel only"
    if bf16x3:
        planes = prepared[0] if prepared is not None else sage_weight_planes(w_t)
        flags = int(bool(relu)) | (SAGE_FULL_TILES if prepared is not None and prepared[3] else 0)
        assert agg_out is None or (agg_out.shape == (n_rows, F_) and agg_out.dtype == torch.float32 and agg_out.stride(1) == 1)
        L.check(L.lib().wgamd_sage_layer_fused_bf16x3_x_train(
            row_ptr.data_ptr(), col_ptr, n_rows, x.data_ptr(), torch_dtype_to_wm(x.dtype), x.stride(0), x.shape[0], F_, ids_ptr,
            ids_dt, self_rows.data_ptr(), int(bool(mean)), planes.data_ptr(), N, _ptr(bias), flags, out.data_ptr(), out.stride(0),
            _ptr(agg_out), 0 if agg_out is None else agg_out.stride(0), get_stream()), "wgamd_sage_layer_fused_bf16x3_x_train")
    else:
        assert agg_out is None, "agg_out: only the bf16x3 layer kernel keeps the aggregate (sage_layer_train_supported)"
        L.check(L.lib().wgamd_sage_layer_fused_f32(
            row_ptr.data_ptr(), col_ptr, n_rows, x.data_ptr(), x.stride(0), x.shape[0], F_, ids_ptr, ids_dt, self_rows.data_ptr(),
            int(bool(mean)), w_t.data_ptr(), w_t.stride(0), N, _ptr(bias), int(bool(relu)), out.data_ptr(), out.stride(0),
            get_stream()), "wgamd_sage_layer_fused_f32")
    if user_out is None:
        return out
    user_out.copy_(out)
    return user_out


def sage_layer_train_supported(F_: int, N: int) -> bool:
    """Shapes whose one-kernel layer has a backward pass on the HIP kernels: the bf16x3 layer kernel (it is the one that keeps
    the aggregate for the backward) and ``wgamd_sage_wgrad_bf16x3``."""
    return (sage_layer_fused_supported(F_, N) and _FUSED_PRECISION == "bf16x3"
            and bool(L.lib().wgamd_sage_layer_bf16x3_supported(F_, _padded_width(N)))
            and L.lib().wgamd_sage_wgrad_workspace_bytes(1, F_, N) > 0)


_WGRAD_WS = {}


def _wgrad_workspace(n_rows: int, F_: int, N: int, device) -> torch.Tensor:
    """Scratch of the weight-gradient launches (the workgroups' partial sums + the composed self rows), grown on demand and
    kept per device: every use is stream-ordered on the caller's stream."""
    need = L.lib().wgamd_sage_wgrad_workspace_bytes(int(n_rows), F_, N)
    if _capturing():       # a captured graph must own its scratch: the shared buffer may be re-allocated by a later eager call
        return torch.empty(int(need) + 4096, dtype=torch.uint8, device=device)
    ws = _WGRAD_WS.get(device)
    if ws is None or ws.numel() < need:
        ws = torch.empty(int(need * 1.15) + 4096, dtype=torch.uint8, device=device)
        _WGRAD_WS[device] = ws
    return ws


def sage_wgrad(agg, x, self_rows, grad_out, grad_w_l, grad_w_r, grad_bias=None, act_out=None, src_ids=None, accumulate=False):
    """Weight gradient of the one-kernel SAGE layer over one hop (``wgamd_sage_wgrad_bf16x3``):
    ``grad_w_l (+)= dZ^T agg``, ``grad_w_r (+)= dZ^T X[self_rows]``, ``grad_bias (+)= sum_i dZ[i]`` with
    ``dZ = grad_out * (act_out > 0)`` (``act_out`` = the layer's ReLU output, None = no activation) and
    ``X[r] = x[src_ids[r]]`` when ``src_ids`` is given.  ``grad_w_*`` are [N, F] contiguous fp32."""
    n, F_ = agg.shape
    N = grad_out.shape[1]
    assert agg.dtype == torch.float32 and agg.stride(1) == 1 and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] == F_
    assert grad_out.dtype == torch.float32 and grad_out.stride(1) == 1 and grad_out.shape[0] == n
    assert self_rows.dtype == torch.int64 and self_rows.is_contiguous() and self_rows.shape[0] == n
    assert grad_w_l.shape == (N, F_) and grad_w_l.is_contiguous() and grad_w_r.shape == (N, F_) and grad_w_r.is_contiguous()
    assert act_out is None or (act_out.shape == grad_out.shape and act_out.stride(1) == 1)
    assert grad_bias is None or (grad_bias.shape == (N,) and grad_bias.is_contiguous())
    ids_ptr, ids_dt = _ids_args(x, src_ids)
    ws = _wgrad_workspace(n, F_, N, agg.device)
    L.check(L.lib().wgamd_sage_wgrad_bf16x3(
        agg.data_ptr(), agg.stride(0), x.data_ptr(), x.stride(0), F_, ids_ptr, ids_dt, self_rows.data_ptr(), n,
        grad_out.data_ptr(), grad_out.stride(0), None if act_out is None else act_out.data_ptr(),
        0 if act_out is None else act_out.stride(0), N, grad_w_l.data_ptr(), grad_w_r.data_ptr(),
        None if grad_bias is None else grad_bias.data_ptr(), int(bool(accumulate)), ws.data_ptr(), ws.numel(), get_stream()),
        "wgamd_sage_wgrad_bf16x3")


def _csr_transpose(row_ptr, col, n_src, want_perm=False, want_dst=False, want_col_t=False):
    """wgamd_csr_transpose_i32: (row_ptr_t, edge_perm | None, edge_dst | None, col_t | None)."""
    _check_csr(row_ptr, col)
    n_dst, E, dev = row_ptr.shape[0] - 1, col.shape[0], col.device
    i32 = dict(dtype=torch.int32, device=dev)
    row_ptr_t = torch.empty(n_src + 1, **i32)
    perm = torch.empty(E, **i32) if want_perm else None
    dst = torch.empty(E, **i32) if want_dst else None
    col_t = torch.empty(E, **i32) if want_col_t else None
    need = L.lib().wgamd_csr_transpose_workspace_bytes(E, n_src)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.lib().wgamd_csr_transpose_i32(row_ptr.data_ptr(), col.data_ptr(), n_dst, E, n_src, row_ptr_t.data_ptr(),
                                            _ptr(perm), _ptr(dst), _ptr(col_t), ws.data_ptr(), need, get_stream()),
            "wgamd_csr_transpose_i32")
    return row_ptr_t, perm, dst, col_t


def csr_transpose(row_ptr, col, n_src):
    """Destination-major hop CSR -> source-major CSR (rows = sources, entries = destination rows, in edge order: a
    stable radix sort over the bits a source row needs, so the gradient sums below are run-to-run deterministic)."""
    row_ptr_t, _, _, col_t = _csr_transpose(row_ptr, col, n_src, want_col_t=True)
    return row_ptr_t, col_t


def spmm_csr_backward(row_ptr, col, grad_out, n_src, mean=True, atomic=False):
    """grad_x[j] = sum_{edges (i, j)} grad_out[i] / (deg(i) if mean).  Default: transpose the hop CSR once and run the
    forward gather kernel over it (no atomics, deterministic; 7x faster than the scatter-add at products sizes);
    ``atomic=True`` keeps the one-kernel ``wgamd_spmm_csr_bwd_f32`` scatter-add."""
    g = grad_out.contiguous()
    if atomic:
        gx = torch.zeros((n_src, g.shape[1]), dtype=torch.float32, device=g.device)
        L.check(L.lib().wgamd_spmm_csr_bwd_f32(row_ptr.data_ptr(), col.data_ptr(), row_ptr.shape[0] - 1,
                                               g.data_ptr(), g.stride(0), g.shape[1], int(bool(mean)),
                                               gx.data_ptr(), gx.stride(0), get_stream()),
                "wgamd_spmm_csr_bwd_f32")
        return gx
    if mean:
        deg = (row_ptr[1:] - row_ptr[:-1]).clamp_(min=1)
        g = g / deg.unsqueeze(1)
    return _spmm_csr_segmented(*csr_transpose(row_ptr, col, n_src), n_src, g)


def _spmm_csr_segmented(row_ptr_t, col_t, n_src: int, g):
    """``out[j] = sum_{e in row j} g[col_t[e]]`` over a transposed hop.  The transposed hop is power-law (a hub is a neighbour of
    thousands of sampled rows) while the gather kernel walks a row with one lane group: the launch would last as long as its
    longest row.  wgamd_spmm_csr_segmented_f32 sums rows in pieces of 64 entries and adds the pieces of a row up in order
    (deterministic, nothing read back)."""
    E, F_ = col_t.shape[0], g.shape[1]
    out = torch.empty((n_src, F_), dtype=torch.float32, device=g.device)
    need = L.lib().wgamd_spmm_csr_segmented_workspace_bytes(E, F_)
    ws = torch.empty(need, dtype=torch.uint8, device=g.device)
    L.check(L.lib().wgamd_spmm_csr_segmented_f32(row_ptr_t.data_ptr(), col_t.data_ptr(), n_src, E, g.data_ptr(), g.stride(0), F_,
                                                 out.data_ptr(), out.stride(0), ws.data_ptr(), need, get_stream()),
            "wgamd_spmm_csr_segmented_f32")
    return out


class _SpmmCsr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, row_ptr, col, mean):
        ctx.save_for_backward(row_ptr, col)
        ctx.mean, ctx.n_src = mean, x.shape[0]
        return spmm_csr_forward(row_ptr, col, x.contiguous(), mean)

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col = ctx.saved_tensors
        return spmm_csr_backward(row_ptr, col, grad_out, ctx.n_src, ctx.mean), None, None, None


class _SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, row_weight):
        n, C = logits.shape
        lib, dev = L.lib(), logits.device
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        state = torch.zeros((lib.wgamd_softmax_xent_state_bytes(n) + 3) // 4, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        L.check(lib.wgamd_softmax_xent_forward_f32(logits.data_ptr(), logits.stride(0), n, C, target.data_ptr(),
                                                   row_weight.data_ptr() if row_weight is not None else None, lse.data_ptr(),
                                                   state.data_ptr(), 1, loss.data_ptr(), get_stream()), "wgamd_softmax_xent_forward_f32")
        ctx.save_for_backward(logits, target, lse, state)
        ctx.row_weight = row_weight
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, target, lse, state = ctx.saved_tensors
        n, C = logits.shape
        g = grad_loss.to(torch.float32).contiguous()
        gx = torch.empty((n, C), dtype=torch.float32, device=logits.device)
        w = ctx.row_weight
        L.check(L.lib().wgamd_softmax_xent_backward_f32(logits.data_ptr(), logits.stride(0), n, C, target.data_ptr(),
                                                        w.data_ptr() if w is not None else None, lse.data_ptr(), state.data_ptr(),
                                                        g.data_ptr(), gx.data_ptr(), gx.stride(0), get_stream()),
                "wgamd_softmax_xent_backward_f32")
        return gx, None, None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, row_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``torch.nn.functional.cross_entropy(logits, target)`` (mean over the rows whose target is not negative — torch's
    ``ignore_index``), optionally with a float weight per ROW (``loader.StagedBatch.seed_mask``: the padding of a ragged last
    mini-batch) — as two launches, forward and backward, instead of torch's seven: the loss of the reference's training loops
    (pylibwholegraph/torch/gnn_model.py:119-125) inside a per-mini-batch step whose every launch sits on its latency floor.
    fp32 logits [n, C] with unit column stride, int64 targets; anything else goes to torch."""
    if (logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda or logits.stride(1) != 1 or logits.shape[0] == 0
            or target.dtype != torch.int64 or target.shape != logits.shape[:1]):
        loss = torch.nn.functional.cross_entropy(logits, target, reduction="none", ignore_index=-100)
        w = (target >= 0).to(loss.dtype) if row_weight is None else row_weight * (target >= 0)
        return (loss * w).sum() / w.sum()
    target = target.contiguous()
    if row_weight is not None:
        row_weight = row_weight.to(torch.float32).contiguous()
    return _SoftmaxXent.apply(logits, target, row_weight)


# ---- link-prediction head (csrc/wg_link.hip) ---------------------------------------------------------------------------------
_LINK_STATE = {}      # (device index, stream) -> the reusable state of wgamd_pair_bce_forward_f32


def _pair_side_grad(index_row, index_other, n_rows: int, x_other, coef, scale_num, scale_den, acc=None):
    """One side's gradient of the pair head: ``out[r] = scale * sum_{p: index_row[p] = r} coef[p] x_other[index_other[p]]``
    (``+ acc[r]``, in place) — the side's incidence list from the stable ``wgamd_coo_to_csr_i64`` over the indices clamped into
    range (a row's pairs stay in pair order), then ONE ``wgamd_pair_grad_f32`` launch: no float atomics, bit-reproducible."""
    lib, dev = L.lib(), x_other.device
    P, C = index_row.shape[0], x_other.shape[1]
    out = acc if acc is not None else torch.empty((n_rows, C), dtype=torch.float32, device=dev)
    if n_rows == 0:
        return out
    rows = index_row.clamp(0, n_rows - 1)
    other = index_other.clamp(0, max(x_other.shape[0] - 1, 0))
    i32 = dict(dtype=torch.int32, device=dev)
    row_ptr, col, pair = torch.empty(n_rows + 1, **i32), torch.empty(P, **i32), torch.empty(P, **i32)
    need = lib.wgamd_coo_to_csr_workspace_bytes(P, n_rows)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(lib.wgamd_coo_to_csr_i64(other.data_ptr(), rows.data_ptr(), P, n_rows, row_ptr.data_ptr(), col.data_ptr(), pair.data_ptr(),
                                     ws.data_ptr(), need, get_stream()), "wgamd_coo_to_csr_i64")
    need = lib.wgamd_pair_grad_workspace_bytes(P, C)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(lib.wgamd_pair_grad_f32(row_ptr.data_ptr(), pair.data_ptr(), n_rows, P, index_row.data_ptr(), index_other.data_ptr(),
                                    coef.data_ptr(), x_other.data_ptr(), x_other.stride(0), x_other.shape[0], C, _ptr(scale_num),
                                    _ptr(scale_den), _ptr(acc), 0 if acc is None else acc.stride(0), out.data_ptr(), out.stride(0),
                                    ws.data_ptr(), need, 0, get_stream()), "wgamd_pair_grad_f32")
    return out


def _pair_grads(ctx, x_src, x_dst, index, coef, scale_num, scale_den):
    """(grad x_src, grad x_dst) of the pair head; one table on both sides: the two sides summed into the first, in a fixed order."""
    i_src, i_dst = index[0], index[1]
    if ctx.shared:
        if not ctx.needs_input_grad[0]:
            return None, None
        g = _pair_side_grad(i_dst, i_src, x_dst.shape[0], x_src, coef, scale_num, scale_den)
        return _pair_side_grad(i_src, i_dst, x_src.shape[0], x_dst, coef, scale_num, scale_den, acc=g), None
    g_src = _pair_side_grad(i_src, i_dst, x_src.shape[0], x_dst, coef, scale_num, scale_den) if ctx.needs_input_grad[0] else None
    g_dst = _pair_side_grad(i_dst, i_src, x_dst.shape[0], x_src, coef, scale_num, scale_den) if ctx.needs_input_grad[1] else None
    return g_src, g_dst


def _pair_args(x_src, x_dst, index):
    return (x_src.data_ptr(), x_src.stride(0), x_src.shape[0], x_dst.data_ptr(), x_dst.stride(0), x_dst.shape[0], x_src.shape[1],
            index[0].data_ptr(), index[1].data_ptr(), index.shape[1])


class _PairDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_src, x_dst, index, shared):
        score = torch.empty(index.shape[1], dtype=torch.float32, device=x_src.device)
        L.check(L.lib().wgamd_pair_dot_forward_f32(*_pair_args(x_src, x_dst, index), score.data_ptr(), get_stream()),
                "wgamd_pair_dot_forward_f32")
        ctx.save_for_backward(x_src, x_dst, index)
        ctx.shared = shared
        return score

    @staticmethod
    def backward(ctx, grad_score):
        x_src, x_dst, index = ctx.saved_tensors
        g = grad_score.to(torch.float32).contiguous()
        return _pair_grads(ctx, x_src, x_dst, index, g, None, None) + (None, None)


class _LinkBce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_src, x_dst, index, label, weight, mean, shared):
        lib, dev = L.lib(), x_src.device
        P = index.shape[1]
        key = (dev.index, get_stream().value)
        state = _LINK_STATE.get(key)
        if state is None:
            state = _LINK_STATE[key] = torch.zeros((lib.wgamd_pair_bce_state_bytes(P) + 3) // 4, dtype=torch.float32, device=dev)
        coef = torch.empty(P + 1, dtype=torch.float32, device=dev)       # [P]: the sum of weights
        loss = torch.empty((), dtype=torch.float32, device=dev)
        L.check(lib.wgamd_pair_bce_forward_f32(*_pair_args(x_src, x_dst, index), label.data_ptr(), _ptr(weight), int(mean), None,
                                               coef.data_ptr(), state.data_ptr(), 1, loss.data_ptr(), get_stream()),
                "wgamd_pair_bce_forward_f32")
        ctx.save_for_backward(x_src, x_dst, index, coef)
        ctx.mean, ctx.shared = mean, shared
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        x_src, x_dst, index, coef = ctx.saved_tensors
        g = grad_loss.to(torch.float32).contiguous()
        den = coef[index.shape[1]:] if ctx.mean else None
        return _pair_grads(ctx, x_src, x_dst, index, coef, g, den) + (None, None, None, None, None)


def _pair_kernel_ok(x_src, x_dst, index) -> bool:
    if index.dim() != 2 or index.shape[0] != 2 or x_src.dim() != 2 or x_dst.dim() != 2 or x_src.shape[1] != x_dst.shape[1]:
        raise ValueError("pair head: index [2, P] over two [rows, C] tables of one width")
    return (all(t.dtype == torch.float32 and t.is_cuda and t.stride(1) == 1 and t.shape[1] >= 1 for t in (x_src, x_dst))
            and index.is_cuda and index.dtype == torch.int64 and index.shape[1] > 0)


def pair_dot(x_src: torch.Tensor, x_dst: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """``(x_src[index[0]] * x_dst[index[1]]).sum(-1)`` — the inner-product decoder of link prediction (the reference's
    examples/mag_lp_mnmg.py, GAE's ``InnerProductDecoder``), and the score AUC / MRR are computed from — in ONE launch that
    never forms the two gathered [P, C] copies, differentiable in both tables with an atomic-free, bit-reproducible backward
    (one launch per side over its incidence list).  ``x_src is x_dst`` is the homogeneous case.  A pair whose index is outside its
    table scores NaN and reads nothing.  float32 tables with unit column stride on the device; anything else goes to torch."""
    if not _pair_kernel_ok(x_src, x_dst, index):
        return (x_src[index[0]] * x_dst[index[1]]).sum(-1)
    return _PairDot.apply(x_src, x_dst, index.contiguous(), x_src is x_dst)


def link_bce_with_logits(x_src: torch.Tensor, x_dst: torch.Tensor, index: torch.Tensor, label: torch.Tensor,
                         pair_weight: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
    """``F.binary_cross_entropy_with_logits(pair_dot(x_src, x_dst, index), label, pair_weight)`` in ONE launch forward (score,
    loss term and the backward's coefficient ``w (sigmoid(s) - y)`` per pair; the loss added up in a fixed order) and one launch
    per side backward.  ``reduction``: "mean" = ``sum(w l) / sum(w)``, "sum" = ``sum(w l)`` (GAE's ``recon_loss`` is "sum" with
    weights 1 / n_pos and 1 / n_neg).  ``label`` in [0, 1], soft labels allowed.  A pair whose index is outside its table makes
    the loss NaN.  Weights that sum to zero give NaN under "mean", as the torch formulation does (nothing is read back to find
    out).  float32 tables with unit column stride on the device and P > 0; anything else goes to torch."""
    if reduction not in ("mean", "sum"):
        raise ValueError("link_bce_with_logits: reduction is 'mean' or 'sum'")
    if not _pair_kernel_ok(x_src, x_dst, index) or label.shape != index.shape[1:]:
        s = (x_src[index[0]] * x_dst[index[1]]).sum(-1)
        y = label.to(s.dtype)
        if pair_weight is None:
            return torch.nn.functional.binary_cross_entropy_with_logits(s, y, reduction=reduction)
        w = pair_weight.to(s.dtype)
        total = torch.nn.functional.binary_cross_entropy_with_logits(s, y, weight=w, reduction="sum")
        return total / w.sum() if reduction == "mean" else total
    label = label.to(device=x_src.device, dtype=torch.float32).contiguous()
    if pair_weight is not None:
        pair_weight = pair_weight.to(device=x_src.device, dtype=torch.float32).contiguous()
        if pair_weight.shape != label.shape:
            raise ValueError("link_bce_with_logits: one weight per pair")
    return _LinkBce.apply(x_src, x_dst, index.contiguous(), label, pair_weight, reduction == "mean", x_src is x_dst)


# ---- MLP edge decoder (csrc/wg_link_mlp.hip) ---------------------------------------------------------------------------------
_LINK_MLP_WS = {}     # (device index, stream) -> the reusable workspace of wgamd_pair_mlp_backward_f32
_ONES = {}            # device -> a grow-only float32 vector of ones (the coefficients of a plain sum over an incidence list)


def _ones(n: int, device) -> torch.Tensor:
    buf = _ONES.get(device)
    if buf is None or buf.shape[0] < n:
        buf = _ONES[device] = torch.ones(max(n * 2, 1 << 16), dtype=torch.float32, device=device)
    return buf[:n]


def pair_mlp_supported(C_src: int, C_dst: int, H: int) -> bool:
    """Shapes of the one-kernel MLP edge decoder (``wgamd_pair_mlp_forward_f32``): both widths multiples of 4, their sum <= 1024,
    1 <= H <= 256."""
    return bool(L.lib().wgamd_pair_mlp_supported(int(C_src), int(C_dst), int(H)))


_LINK_WGRAD_SPLIT = 1024      # row ranges of the split-K over a whole table (a hop's 128 leave most of the chip idle there)


def _wgrad_blocks(x, G):
    """``G^T x`` ([H, C]) by ``gcn_wgrad`` over column blocks of x no wider than its 256, and ``colsum(G)`` from the first."""
    H, C = G.shape[1], x.shape[1]
    gb = torch.empty(H, dtype=torch.float32, device=G.device)
    blocks = []
    for c0 in range(0, C, 256):
        gw = torch.empty((H, min(256, C - c0)), dtype=torch.float32, device=G.device)
        gcn_wgrad(x[:, c0:c0 + 256], G, gw, gb if c0 == 0 else None, max_split=_LINK_WGRAD_SPLIT)
        blocks.append(gw)
    return (blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)), gb


class _PairMlp(torch.autograd.Function):
    """The one-kernel MLP edge decoder, with (``label`` given) or without its binary cross-entropy.  Backward: ONE launch turns
    the kept hidden rows into dZ and sums dw2 / db2; the concatenation is linear, so each side's ``G[r] = sum of dZ over the pairs
    of row r`` is ``wgamd_pair_grad_f32`` over that side's incidence list (dZ as the other table, read by pair), and
    ``dx = G @ W1[:, side]`` (a library GEMM), ``dW1[:, side] = G^T x``, ``db1 = colsum(G_src)`` (``gcn_wgrad``).  No float
    atomics anywhere."""

    @staticmethod
    def forward(ctx, x_src, x_dst, w1, b1, w2, b2, index, label, weight, mean, shared, keep):
        lib, dev = L.lib(), x_src.device
        P, H = index.shape[1], w1.shape[0]
        bce = label is not None
        w1k = w1.detach()
        if w1k.stride(1) != 1 or w1k.stride(0) % 4 or w1k.data_ptr() % 16:
            w1k = w1k.contiguous()
        w2k = w2.detach().reshape(-1).contiguous()
        b1k = None if b1 is None else b1.detach().contiguous()
        hidden = torch.empty((P, (H + 3) // 4 * 4), dtype=torch.float32, device=dev) if keep else None
        score = coef = state = loss = None
        if bce:
            key = (dev.index, get_stream().value)
            state = _LINK_STATE.get(key)
            if state is None:
                state = _LINK_STATE[key] = torch.zeros((lib.wgamd_pair_bce_state_bytes(P) + 3) // 4, dtype=torch.float32, device=dev)
            coef = torch.empty(P + 1, dtype=torch.float32, device=dev)       # [P]: the sum of weights
            loss = torch.empty((), dtype=torch.float32, device=dev)
        else:
            score = torch.empty(P, dtype=torch.float32, device=dev)
        L.check(lib.wgamd_pair_mlp_forward_f32(
            x_src.data_ptr(), x_src.stride(0), x_src.shape[0], x_dst.data_ptr(), x_dst.stride(0), x_dst.shape[0], x_src.shape[1],
            x_dst.shape[1], index[0].data_ptr(), index[1].data_ptr(), P, w1k.data_ptr(), w1k.stride(0), H,
            _ptr(b1k), w2k.data_ptr(), None if b2 is None else b2.detach().data_ptr(), _ptr(label), _ptr(weight), int(mean),
            _ptr(score), _ptr(coef), _ptr(state), 1, _ptr(loss), _ptr(hidden), 0 if hidden is None else hidden.stride(0),
            get_stream()),
            "wgamd_pair_mlp_forward_f32")
        if keep:
            ctx.save_for_backward(x_src, x_dst, w1, w2, index, coef)
            ctx.kept = hidden
            ctx.mean, ctx.shared, ctx.bce = mean, shared, bce
        return loss if bce else score

    @staticmethod
    def backward(ctx, g):
        _released(ctx.kept, "EdgeDecoder", "hidden rows")
        x_src, x_dst, w1, w2, index, coef = ctx.saved_tensors
        hidden, ctx.kept = ctx.kept, None
        lib, dev = L.lib(), hidden.device
        need_xs, need_xd, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:6]
        P, (H, K), Cs = index.shape[1], w1.shape, x_src.shape[1]
        g = g.to(torch.float32).contiguous()
        if ctx.bce:      # g_p = grad_loss * c_p (/ sum w): the scale stays on the device
            per_pair, num, den = coef, g, (coef[P:] if ctx.mean else None)
        else:
            per_pair, num, den = g, None, None
        key = (dev.index, get_stream().value)
        ws = _LINK_MLP_WS.get(key)
        if ws is None:
            ws = _LINK_MLP_WS[key] = torch.zeros(lib.wgamd_pair_mlp_backward_workspace_bytes(H), dtype=torch.uint8, device=dev)
        gw2 = torch.empty(H, dtype=torch.float32, device=dev) if need_w2 else None
        gb2 = torch.empty(1, dtype=torch.float32, device=dev) if need_b2 else None
        w2k = w2.detach().reshape(-1).contiguous()
        L.check(lib.wgamd_pair_mlp_backward_f32(
            hidden.data_ptr(), hidden.stride(0), P, H, w2k.data_ptr(), per_pair.data_ptr(),
            _ptr(num), _ptr(den), index[0].data_ptr(), x_src.shape[0], index[1].data_ptr(), x_dst.shape[0], _ptr(gw2), _ptr(gb2),
            ws.data_ptr(), ws.numel(), 1, get_stream()), "wgamd_pair_mlp_backward_f32")
        dz = hidden[:, :H]
        want_src = need_xs or need_w1 or need_b1
        want_dst = need_xd or need_w1 or (ctx.shared and need_xs)
        by_pair, one = _arange(P, dev), _ones(P, dev)
        G_src = _pair_side_grad(index[0], by_pair, x_src.shape[0], dz, one, None, None) if want_src else None
        G_dst = _pair_side_grad(index[1], by_pair, x_dst.shape[0], dz, one, None, None) if want_dst else None
        w1d = w1.detach()
        gxs = G_src @ w1d[:, :Cs] if need_xs else None
        gxd = None
        if ctx.shared and need_xs:      # one table on both sides: source side first, then destination side
            gxs = torch.addmm(gxs, G_dst, w1d[:, Cs:])
        elif need_xd:
            gxd = G_dst @ w1d[:, Cs:]
        gw1 = gb1 = None
        if need_w1 or need_b1:
            gw_src, gb1 = _wgrad_blocks(x_src.detach(), G_src)
            if need_w1:
                gw1 = torch.cat([gw_src, _wgrad_blocks(x_dst.detach(), G_dst)[0]], dim=1)
            gb1 = gb1 if need_b1 else None
        if gw2 is not None:
            gw2 = gw2.reshape(w2.shape)
        return gxs, gxd, gw1, gb1, gw2, gb2, None, None, None, None, None, None


def _pair_mlp_check(x_src, x_dst, index, w1, b1, w2, b2, name):
    """Shape checks of the MLP edge decoder (ValueError), then whether the kernel takes the call."""
    if index.dim() != 2 or index.shape[0] != 2 or x_src.dim() != 2 or x_dst.dim() != 2:
        raise ValueError("%s: index [2, P] over two [rows, C] tables" % name)
    if w1.dim() != 2 or w1.shape[1] != x_src.shape[1] + x_dst.shape[1]:
        raise ValueError("%s: w1 is [H, C_src + C_dst]" % name)
    H = w1.shape[0]
    if w2.numel() != H or (b1 is not None and b1.shape != (H,)) or (b2 is not None and b2.numel() != 1):
        raise ValueError("%s: b1 [H], w2 [H] (or [1, H]), b2 one element" % name)
    params = [t for t in (w1, b1, w2, b2) if t is not None]
    return (all(t.dtype == torch.float32 and t.is_cuda for t in [x_src, x_dst] + params)
            and all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (x_src, x_dst))
            and index.is_cuda and index.dtype == torch.int64 and index.shape[1] > 0 and index.shape[1] < 2 ** 31
            and x_src.shape[0] < 2 ** 31 and x_dst.shape[0] < 2 ** 31 and H >= 1
            and pair_mlp_supported(x_src.shape[1], x_dst.shape[1], H))


def _pair_mlp_keeps(*tensors) -> bool:
    """Whether a backward pass may follow: only then does the forward write the hidden rows out ([P, H])."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _pair_mlp_torch(x_src, x_dst, index, w1, b1, w2, b2):
    z = torch.cat([x_src[index[0]], x_dst[index[1]]], dim=-1)
    h = torch.nn.functional.linear(z, w1, b1).relu()
    return torch.nn.functional.linear(h, w2.reshape(1, -1), None if b2 is None else b2.reshape(1)).view(-1)


def pair_mlp(x_src: torch.Tensor, x_dst: torch.Tensor, index: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor],
             w2: torch.Tensor, b2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``lin2(relu(lin1(cat([x_src[index[0]], x_dst[index[1]]], -1)))).view(-1)`` — the MLP edge decoder of link prediction (the
    ``EdgeDecoder`` of the reference's examples/movielens_mnmg.py and taobao_mnmg.py): ``w1`` [H, C_src + C_dst] and ``b1`` [H]
    are ``lin1``'s, ``w2`` [1, H] (or [H]) and ``b2`` [1] ``lin2``'s; either bias may be None.  ONE launch forward that forms
    neither the gathered rows, nor their concatenation, nor (without grad mode) the hidden activation in memory; differentiable
    in the tables and the four parameters with an atomic-free, bit-reproducible backward.  ``x_src is x_dst`` is the homogeneous
    case.  A pair whose index is outside its table scores NaN, reads nothing and adds nothing to any gradient.  Kernel domain
    (``pair_mlp_supported``): float32 on the device, unit column stride, 16-byte aligned rows, both widths multiples of 4 with
    C_src + C_dst <= 1024, H <= 256; anything else goes to the torch formulation."""
    if not _pair_mlp_check(x_src, x_dst, index, w1, b1, w2, b2, "pair_mlp"):
        return _pair_mlp_torch(x_src, x_dst, index, w1, b1, w2, b2)
    return _PairMlp.apply(x_src, x_dst, w1, b1, w2, b2, index.contiguous(), None, None, False, x_src is x_dst,
                          _pair_mlp_keeps(x_src, x_dst, w1, b1, w2, b2))


def link_mlp_bce_with_logits(x_src: torch.Tensor, x_dst: torch.Tensor, index: torch.Tensor, label: torch.Tensor, w1: torch.Tensor,
                             b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor] = None,
                             pair_weight: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
    """``F.binary_cross_entropy_with_logits(pair_mlp(x_src, x_dst, index, w1, b1, w2, b2), label, pair_weight)`` with the loss in
    the decoder's ONE forward launch (score, loss term and the backward's coefficient per pair; the loss added up in a fixed
    order).  ``reduction``, ``label``, ``pair_weight``, out-of-range pairs (the loss is NaN) and the torch fallback as
    ``link_bce_with_logits``; the kernel domain as ``pair_mlp``."""
    if reduction not in ("mean", "sum"):
        raise ValueError("link_mlp_bce_with_logits: reduction is 'mean' or 'sum'")
    kernel = _pair_mlp_check(x_src, x_dst, index, w1, b1, w2, b2, "link_mlp_bce_with_logits")
    if label.shape != index.shape[1:]:
        raise ValueError("link_mlp_bce_with_logits: one label per pair")
    if pair_weight is not None and pair_weight.shape != label.shape:
        raise ValueError("link_mlp_bce_with_logits: one weight per pair")
    if not kernel:
        s = _pair_mlp_torch(x_src, x_dst, index, w1, b1, w2, b2)
        y = label.to(s.dtype)
        if pair_weight is None:
            return torch.nn.functional.binary_cross_entropy_with_logits(s, y, reduction=reduction)
        w = pair_weight.to(s.dtype)
        total = torch.nn.functional.binary_cross_entropy_with_logits(s, y, weight=w, reduction="sum")
        return total / w.sum() if reduction == "mean" else total
    label = label.to(device=x_src.device, dtype=torch.float32).contiguous()
    if pair_weight is not None:
        pair_weight = pair_weight.to(device=x_src.device, dtype=torch.float32).contiguous()
    return _PairMlp.apply(x_src, x_dst, w1, b1, w2, b2, index.contiguous(), label, pair_weight, reduction == "mean", x_src is x_dst,
                          _pair_mlp_keeps(x_src, x_dst, w1, b1, w2, b2))


class EdgeDecoder(torch.nn.Module):
    """The ``EdgeDecoder`` of the reference's examples/movielens_mnmg.py and taobao_mnmg.py on the one-kernel head:
    ``lin2(relu(lin1(cat([z_src[row], z_dst[col]], -1)))).view(-1)`` with ``lin1 = Linear(C_src + C_dst, hidden_channels)`` and
    ``lin2 = Linear(hidden_channels, 1)`` — the reference's parameter names, so its checkpoints load.  ``in_channels``: an int
    or a ``(C_src, C_dst)`` pair; None = ``hidden_channels`` on both sides (the reference's class).  ``forward`` returns the
    scores (``pair_mlp``); ``loss`` their binary cross-entropy in the same launch (``link_mlp_bce_with_logits``)."""

    def __init__(self, hidden_channels: int, in_channels: Union[int, Tuple[int, int], None] = None, bias: bool = True):
        super().__init__()
        if in_channels is None:
            in_channels = hidden_channels
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.hidden_channels = (int(in_channels[0]), int(in_channels[1])), int(hidden_channels)
        self.lin1 = torch.nn.Linear(sum(self.in_channels), self.hidden_channels, bias=bias)
        self.lin2 = torch.nn.Linear(self.hidden_channels, 1, bias=bias)

    def reset_parameters(self):
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def forward(self, z_src: torch.Tensor, z_dst: torch.Tensor, edge_label_index: torch.Tensor) -> torch.Tensor:
        return pair_mlp(z_src, z_dst, edge_label_index, self.lin1.weight, self.lin1.bias, self.lin2.weight, self.lin2.bias)

    def loss(self, z_src: torch.Tensor, z_dst: torch.Tensor, edge_label_index: torch.Tensor, edge_label: torch.Tensor,
             pair_weight: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
        return link_mlp_bce_with_logits(z_src, z_dst, edge_label_index, edge_label, self.lin1.weight, self.lin1.bias,
                                        self.lin2.weight, self.lin2.bias, pair_weight=pair_weight, reduction=reduction)

    def extra_repr(self) -> str:
        return "in_channels=%s, hidden_channels=%d" % (self.in_channels, self.hidden_channels)


def spmm_csr(x, row_ptr, col, reduce: str = "mean"):
    """Differentiable segmented mean/sum aggregation over a destination-major CSR."""
    assert reduce in ("mean", "sum", "add")
    return _SpmmCsr.apply(x, row_ptr, col, reduce == "mean")


def gat_forward(row_ptr, col, x, a_src, a_dst, heads, negative_slope=0.2, need_alpha=True):
    """Edge softmax + weighted aggregation.  x [N_src, H*C], a_src [N_src, H], a_dst [n_rows, H]."""
    _check_csr(row_ptr, col)
    n_rows = row_ptr.shape[0] - 1
    HC = x.shape[1]
    C = HC // heads
    out = torch.empty((n_rows, HC), dtype=torch.float32, device=x.device)
    alpha = torch.empty((col.shape[0], heads), dtype=torch.float32, device=x.device) if need_alpha else None
    L.check(L.lib().wgamd_gat_csr_f32(row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0),
                                      a_src.data_ptr(), a_dst.data_ptr(), heads, C, float(negative_slope),
                                      alpha.data_ptr() if need_alpha else None, out.data_ptr(), out.stride(0),
                                      get_stream()), "wgamd_gat_csr_f32")
    return out, alpha


def gat_forward_rows(row_ptr, col, x, a_src, a_dst, heads, out, dst_rows=None, accumulate=False, negative_slope=0.2):
    """``gat_forward`` for the rows of ONE hop and edge type of a heterogeneous call group: row i of the launch reads
    ``a_dst[dst_rows[i]]`` and writes (``accumulate``: adds to) ``out[dst_rows[i]]`` — see wgamd_gat_csr_rows_f32."""
    _check_csr(row_ptr, col)
    n_rows = row_ptr.shape[0] - 1
    C = x.shape[1] // heads
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[1] == x.shape[1]
    assert dst_rows is None or (dst_rows.dtype == torch.int64 and dst_rows.is_contiguous() and dst_rows.shape[0] >= n_rows)
    L.check(L.lib().wgamd_gat_csr_rows_f32(row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0),
                                           a_src.data_ptr(), a_dst.data_ptr(), heads, C, float(negative_slope),
                                           None if dst_rows is None else dst_rows.data_ptr(), int(bool(accumulate)), None,
                                           out.data_ptr(), out.stride(0), get_stream()), "wgamd_gat_csr_rows_f32")
    return out


def _gat_ids(src_ids, dst_ids, a_src, src_terms_by_id, dst_terms_by_id):
    """(src_ids pointer, dst_ids pointer, terms_by_id) of a fetch-in-the-layer GAT launch: int64 contiguous lists; without
    ``src_terms_by_id`` the attention terms have one row per listed id."""
    if src_ids is None:
        assert not src_terms_by_id and not dst_terms_by_id
        return None, None, 0
    assert src_ids.dtype == torch.int64 and src_ids.is_contiguous() and (src_terms_by_id or src_ids.shape[0] == a_src.shape[0])
    assert not dst_terms_by_id or (dst_ids is not None and dst_ids.dtype == torch.int64 and dst_ids.is_contiguous())
    return src_ids.data_ptr(), dst_ids.data_ptr() if dst_terms_by_id else None, int(bool(src_terms_by_id)) | 2 * int(bool(dst_terms_by_id))


def gat_aggregate_heads(row_ptr, col, x, a_src, a_dst, heads, dst_rows=None, negative_slope=0.2, out=None, src_ids=None, dst_ids=None,
                        src_terms_by_id=False, dst_terms_by_id=False):
    """Aggregate-first GAT (wgamd_gat_aggregate_heads_f32): ``agg[i, h, :] = sum_e alpha_e^h x[col[e], :]`` with x
    untransformed ([N_src, F]); returns ``[n_rows, heads * F]``.  ``gat_transform_heads`` applies the per-head weights.
    ``src_ids`` (int64 [N_src]): the rows are read THROUGH the list, ``x[src_ids[col[e]]]`` — x the feature table, src_ids the
    call group's node list (``LazyRows``); the attention terms stay indexed by ``col`` — unless ``src_terms_by_id``: ``a_src`` then
    holds the terms of the TABLE's rows, read at ``src_ids[col[e]]`` (``dst_terms_by_id``: ``a_dst`` at ``dst_ids[dst row]``)."""
    _check_csr(row_ptr, col)
    ids_p, dids_p, by_id = _gat_ids(src_ids, dst_ids, a_src, src_terms_by_id, dst_terms_by_id)
    n_rows, F_ = row_ptr.shape[0] - 1, x.shape[1]
    if out is None:
        out = torch.empty((n_rows, heads * F_), dtype=torch.float32, device=x.device)
    assert a_src.is_contiguous() and a_dst.is_contiguous() and a_src.shape[1] == heads
    L.check(L.lib().wgamd_gat_aggregate_heads_ids_f32(row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0),
                                                      ids_p, dids_p, by_id, F_, a_src.data_ptr(), a_dst.data_ptr(), heads,
                                                      float(negative_slope), None if dst_rows is None else dst_rows.data_ptr(),
                                                      out.data_ptr(), out.stride(0), get_stream()), "wgamd_gat_aggregate_heads_ids_f32")
    return out


def gat_transform_heads(agg, w, heads, out=None, overwrite=False, fused=True):
    """``out[i, h*C:(h+1)*C] (+)= agg[i, h, :] @ w[:, h*C:(h+1)*C]`` — the H small GEMMs after ``gat_aggregate_heads``.
    ``out`` given: accumulated into (HeteroConv's sum), or written (``overwrite``).  Shapes
    ``wgamd_gat_transform_heads_bf16x3`` is built for (C = 64, F in {64, 128, 256}) run on it (``gat_transform_heads_fused``:
    the bf16 matrix pipe at fp32 accuracy, one pass); ``fused=False`` or any other shape: one strided batched library GEMM
    (fp32 MFMA through hipBLASLt)."""
    n, F_ = agg.shape[0], agg.shape[1] // heads
    C = w.shape[1] // heads
    if fused and n > 0 and agg.is_cuda and agg.stride(1) == 1 and w.stride(1) == 1 and gat_transform_supported(F_, heads, C) \
            and (out is None or out.stride(1) == 1):
        return gat_transform_heads_fused(agg, w, heads, acc_in=None if (out is None or overwrite) else out, out=out)
    a, b = agg.view(n, heads, F_).permute(1, 0, 2), w.view(F_, heads, C).permute(1, 0, 2)
    if out is None:
        return torch.bmm(a, b).permute(1, 0, 2).reshape(n, heads * C)                                    # [H, n, C] -> [n, H C]
    # accumulate in place through the strided view (beta = 1): no [H, n, C] temporary and no separate add pass — same bits,
    # 1.48 -> 1.15 ms at 1 M rows, 4 x 128 -> 4 x 64
    # ``overwrite``: beta = 0 — ``out`` need not be initialised (the first relation of HeteroConv's sum: no zero-fill, no read)
    acc = out.view(n, heads, C).permute(1, 0, 2)
    torch.baddbmm(acc, a, b, beta=0 if overwrite else 1, out=acc)
    return out


def gat_transform_supported(F_: int, heads: int, C: int) -> bool:
    return bool(L.lib().wgamd_gat_transform_heads_supported(int(F_), int(heads), int(C)))


def _gat_weight_tiles(w: torch.Tensor, heads: int) -> torch.Tensor:
    """``w`` [F, H C] in the order ``wgamd_gat_transform_heads_bf16x3`` reads it; kept on the weight like ``sage_weight_planes``."""
    def build():
        F_, C = w.shape[0], w.shape[1] // heads
        tiles = torch.empty(L.lib().wgamd_gat_transform_weight_bytes(F_, heads, C), dtype=torch.uint8, device=w.device)
        L.check(L.lib().wgamd_gat_transform_weight_tiles(w.data_ptr(), w.stride(0), F_, heads, C, tiles.data_ptr(), get_stream()),
                "wgamd_gat_transform_weight_tiles")
        return tiles
    return _derived(w, "gat_tiles", (w,), build, extra=heads)


def gat_transform_heads_fused(agg, w, heads, acc_in=None, bias=None, relu=False, out_rows=None, out=None):
    """``out[out_rows[i]] = act(agg[i, h, :] @ w[:, h C:(h+1) C] + acc_in[i] + bias)`` in ONE kernel
    (``wgamd_gat_transform_heads_bf16x3``: the per-head GEMMs on the bf16 matrix pipe at fp32 accuracy, HeteroConv's running sum,
    bias, ReLU and the row placement).  ``acc_in`` may be ``out`` itself when ``out_rows`` is None."""
    n, F_ = agg.shape[0], agg.shape[1] // heads
    C = w.shape[1] // heads
    assert agg.dtype == torch.float32 and agg.stride(1) == 1 and w.dtype == torch.float32 and w.stride(1) == 1 and w.shape[0] == F_
    if out is None:
        assert out_rows is None
        out = torch.empty((n, heads * C), dtype=torch.float32, device=agg.device)
    assert out.stride(1) == 1 and (acc_in is None or acc_in.stride(1) == 1)
    L.check(L.lib().wgamd_gat_transform_heads_bf16x3(
        agg.data_ptr(), agg.stride(0), n, F_, heads, C, _gat_weight_tiles(w, heads).data_ptr(),
        None if acc_in is None else acc_in.data_ptr(), 0 if acc_in is None else acc_in.stride(0),
        None if bias is None else bias.data_ptr(), int(bool(relu)), None if out_rows is None else out_rows.data_ptr(),
        out.data_ptr(), out.stride(0), get_stream()), "wgamd_gat_transform_heads_bf16x3")
    return out


def gat_layer_fused_supported(F_: int, heads: int, C: int) -> bool:
    return bool(L.lib().wgamd_gat_layer_fused_supported(int(F_), int(heads), int(C)))


def gat_layer_fused(row_ptr, col, x, a_src, a_dst, w, heads, dst_rows=None, negative_slope=0.2, acc_in=None, bias=None, relu=False,
                    out_rows=None, out=None, src_ids=None, dst_ids=None, src_terms_by_id=False, dst_terms_by_id=False):
    """``gat_aggregate_heads`` + ``gat_transform_heads_fused`` as ONE kernel (``wgamd_gat_layer_fused_bf16x3``): the
    [n_rows, heads * F] aggregate never leaves the CU.  For hops with a fan-out of at most 10 (longer rows are correct, slow).
    ``src_ids`` / ``dst_ids`` / ``*_terms_by_id``: as in ``gat_aggregate_heads``."""
    _check_csr(row_ptr, col)
    ids_p, dids_p, by_id = _gat_ids(src_ids, dst_ids, a_src, src_terms_by_id, dst_terms_by_id)
    n_rows, F_ = row_ptr.shape[0] - 1, x.shape[1]
    C = w.shape[1] // heads
    assert x.dtype == torch.float32 and x.stride(1) == 1 and a_src.is_contiguous() and a_dst.is_contiguous() and a_src.shape[1] == heads
    if out is None:
        assert out_rows is None
        out = torch.empty((n_rows, heads * C), dtype=torch.float32, device=x.device)
    assert col.numel() > 0 and out.stride(1) == 1 and (acc_in is None or acc_in.stride(1) == 1)
    L.check(L.lib().wgamd_gat_layer_fused_ids_bf16x3(
        row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0), ids_p, dids_p, by_id, F_, a_src.data_ptr(),
        a_dst.data_ptr(), heads, C,
        float(negative_slope), None if dst_rows is None else dst_rows.data_ptr(), _gat_weight_tiles(w, heads).data_ptr(),
        None if acc_in is None else acc_in.data_ptr(), 0 if acc_in is None else acc_in.stride(0),
        None if bias is None else bias.data_ptr(), int(bool(relu)), None if out_rows is None else out_rows.data_ptr(),
        out.data_ptr(), out.stride(0), get_stream()), "wgamd_gat_layer_fused_ids_bf16x3")
    return out


def gather_terms_supported(F_: int, T: int) -> bool:
    return bool(L.lib().wgamd_gather_terms_supported(int(F_), int(T)))


def gather_with_terms(table: torch.Tensor, ids: torch.Tensor, v: torch.Tensor, out: torch.Tensor = None, heads: int = 0):
    """``-> (x, terms)``: ``x = table[ids]`` and ``terms = x @ v`` (``v`` [F, T], T <= 32) in ONE pass over the gathered rows
    (``wgamd_gather_terms_f32``: the row gather feeds an exact-fp32 MFMA).  For GATConv's attention logits, whose folded
    [F, H] matrices of every relation end of a node type are concatenated into ``v``.  ``heads=4``: ``terms`` comes back as
    [T / 4, n, 4] — one contiguous [n, 4] slab per relation end — instead of [n, T]."""
    assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1 and v.dtype == torch.float32
    assert ids.dim() == 1 and ids.is_contiguous() and ids.dtype in (torch.int32, torch.int64)
    n, F_, T = int(ids.shape[0]), int(table.shape[1]), int(v.shape[1])
    assert v.shape[0] == F_ and v.is_contiguous()
    if out is None:
        out = torch.empty((n, F_), dtype=torch.float32, device=table.device)
    assert heads in (0, 4) and (heads == 0 or T % 4 == 0)
    terms = torch.empty((T // 4, n, 4) if heads else (n, T), dtype=torch.float32, device=table.device)
    L.check(L.lib().wgamd_gather_terms_f32(table.data_ptr(), table.stride(0), ids.data_ptr(), torch_dtype_to_wm(ids.dtype), n, F_,
                                           v.data_ptr(), T, out.data_ptr(), out.stride(0), terms.data_ptr(), T, heads,
                                           get_stream()), "wgamd_gather_terms_f32")
    return out, terms


def lazy_rows_terms(table: torch.Tensor, ids: torch.Tensor, v: torch.Tensor, heads: int = 0):
    """``terms = table[ids] @ v`` WITHOUT writing the gathered rows (``wgamd_gather_terms_f32`` with no row output): the attention
    logits of a ``LazyRows`` input whose rows the relation kernels then read through ``ids`` themselves."""
    assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1 and v.dtype == torch.float32 and v.is_contiguous()
    assert ids.dim() == 1 and ids.is_contiguous() and ids.dtype in (torch.int32, torch.int64)
    n, F_, T = int(ids.shape[0]), int(table.shape[1]), int(v.shape[1])
    assert v.shape[0] == F_ and heads in (0, 4) and (heads == 0 or T % 4 == 0)
    terms = torch.empty((T // 4, n, 4) if heads else (n, T), dtype=torch.float32, device=table.device)
    L.check(L.lib().wgamd_gather_terms_f32(table.data_ptr(), table.stride(0), ids.data_ptr(), torch_dtype_to_wm(ids.dtype), n, F_,
                                           v.data_ptr(), T, None, 0, terms.data_ptr(), T, heads, get_stream()), "wgamd_gather_terms_f32")
    return terms


def gather_term_slabs(slabs: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """``out[k, i] = slabs[k, ids[i]]`` for attention-term slabs [K, n_table, 4] (``wgamd_gather_term_slabs_f32``): the terms of a
    call group's rows from the terms of the table's rows."""
    assert slabs.dtype == torch.float32 and slabs.dim() == 3 and slabs.shape[2] == 4 and slabs.is_contiguous()
    assert ids.dim() == 1 and ids.is_contiguous() and ids.dtype in (torch.int32, torch.int64)
    K, n_in, n = int(slabs.shape[0]), int(slabs.shape[1]), int(ids.shape[0])
    out = torch.empty((K, n, 4), dtype=torch.float32, device=slabs.device)
    L.check(L.lib().wgamd_gather_term_slabs_f32(slabs.data_ptr(), n_in, K, ids.data_ptr(), torch_dtype_to_wm(ids.dtype), n,
                                                out.data_ptr(), get_stream()), "wgamd_gather_term_slabs_f32")
    return out


def rows_terms(x: torch.Tensor, v: torch.Tensor, heads: int = 0):
    """``terms = x @ v`` for a resident [n, F] matrix and a narrow ``v`` [F, T] (T <= 32) in ONE streaming pass over ``x``
    (``wgamd_gather_terms_f32`` without an id list and without a row copy: exact-fp32 MFMA, rows through registers once).
    ``heads=4``: [T / 4, n, 4] slabs — one contiguous [n, 4] block per relation end, what the GAT kernels read — instead of
    [n, T]: no transposing copy after a library GEMM."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and v.dtype == torch.float32 and v.is_contiguous()
    n, F_, T = int(x.shape[0]), int(x.shape[1]), int(v.shape[1])
    assert v.shape[0] == F_ and heads in (0, 4) and (heads == 0 or T % 4 == 0)
    terms = torch.empty((T // 4, n, 4) if heads else (n, T), dtype=torch.float32, device=x.device)
    L.check(L.lib().wgamd_gather_terms_f32(x.data_ptr(), x.stride(0), None, torch_dtype_to_wm(torch.int64), n, F_, v.data_ptr(), T,
                                           None, 0, terms.data_ptr(), T, heads, get_stream()), "wgamd_gather_terms_f32")
    return terms


def bias_act_rows(x, bias=None, relu=True, dst_rows=None, out=None):
    """``out[dst_rows[i]] = act(x[i] + bias)`` in one pass (wgamd_bias_act_rows_f32); ``out`` defaults to a fresh [n, C]."""
    n, C = x.shape
    if out is None:
        assert dst_rows is None
        out = torch.empty((n, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().wgamd_bias_act_rows_f32(x.data_ptr(), x.stride(0), n, C, None if bias is None else bias.data_ptr(), int(bool(relu)),
                                            None if dst_rows is None else dst_rows.data_ptr(), out.data_ptr(), out.stride(0),
                                            get_stream()), "wgamd_bias_act_rows_f32")
    return out


def gat_backward_supported(H: int, C: int) -> bool:
    """Shapes ``wgamd_gat_csr_bwd_f32`` is built for (include/wgamd_ext.h)."""
    return C % 4 == 0 and ((C // 4) & (C // 4 - 1)) == 0 and H * C <= 256


def gat_backward(row_ptr, col, x, a_src, a_dst, alpha, grad_out, heads, negative_slope=0.2):
    """(grad_x, grad_a_src, grad_a_dst) of ``gat_forward`` on the HIP kernels: a destination-major pass (per-head dot
    products, softmax backward, grad_a_dst) and a source-major pass over the transposed hop CSR (grad_x, grad_a_src)."""
    _check_csr(row_ptr, col)
    n_rows, n_src, E = row_ptr.shape[0] - 1, x.shape[0], col.shape[0]
    C = x.shape[1] // heads
    g = grad_out.contiguous()
    row_ptr_t, edge_perm, edge_dst, _ = _csr_transpose(row_ptr, col, n_src, want_perm=True, want_dst=True)
    de = torch.empty((E, heads), dtype=torch.float32, device=x.device)
    gx = torch.empty_like(x)
    ga_src, ga_dst = torch.empty_like(a_src), torch.empty_like(a_dst)
    need = L.lib().wgamd_gat_csr_bwd_workspace_bytes(E, heads, C)      # pieces of long source rows (hubs of the hop)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    L.check(L.lib().wgamd_gat_csr_bwd_f32_v2(
        row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0), a_src.data_ptr(), a_dst.data_ptr(), heads, C,
        float(negative_slope), alpha.data_ptr(), g.data_ptr(), g.stride(0), row_ptr_t.data_ptr(), edge_perm.data_ptr(),
        edge_dst.data_ptr(), n_src, de.data_ptr(), gx.data_ptr(), gx.stride(0), ga_src.data_ptr(), ga_dst.data_ptr(),
        E, ws.data_ptr(), need, get_stream()), "wgamd_gat_csr_bwd_f32_v2")
    return gx, ga_src, ga_dst


class _GatCsr(torch.autograd.Function):
    """Forward: fused HIP kernel.  Backward: edge-wise torch ops on the saved attention (the
    training-time gradient path is not on the north-star hot path)."""

    @staticmethod
    def forward(ctx, x, a_src, a_dst, row_ptr, col, heads, slope):
        x, a_src, a_dst = x.contiguous(), a_src.contiguous(), a_dst.contiguous()
        out, alpha = gat_forward(row_ptr, col, x, a_src, a_dst, heads, slope, need_alpha=True)
        ctx.save_for_backward(x, a_src, a_dst, row_ptr, col, alpha)
        ctx.heads, ctx.slope = heads, slope
        return out

    @staticmethod
    def backward(ctx, g):
        x, a_src, a_dst, row_ptr, col, alpha = ctx.saved_tensors
        H = ctx.heads
        C = x.shape[1] // H
        n_rows = row_ptr.shape[0] - 1
        if gat_backward_supported(H, C) and col.shape[0] > 0:
            return gat_backward(row_ptr, col, x, a_src, a_dst, alpha, g, H, ctx.slope) + (None, None, None, None)
        deg = (row_ptr[1:] - row_ptr[:-1]).long()
        dst = torch.repeat_interleave(torch.arange(n_rows, device=x.device), deg)
        src = col.long()
        g3 = g.reshape(n_rows, H, C)[dst]                      # [E,H,C]
        x3 = x.reshape(-1, H, C)[src]                          # [E,H,C]
        gx = torch.zeros_like(x).reshape(-1, H, C).index_add_(0, src, alpha.unsqueeze(-1) * g3)
        dalpha = (g3 * x3).sum(-1)                             # [E,H]
        dot = torch.zeros((n_rows, H), device=x.device).index_add_(0, dst, alpha * dalpha)
        ds = alpha * (dalpha - dot[dst])
        s = a_src[src] + a_dst[dst]
        ds = torch.where(s > 0, ds, ds * ctx.slope)
        ga_src = torch.zeros_like(a_src).index_add_(0, src, ds)
        ga_dst = torch.zeros_like(a_dst).index_add_(0, dst, ds)
        return gx.reshape(x.shape), ga_src, ga_dst, None, None, None, None


def _single_hop(graph, n_dst, *edge_arrays):
    """A layer's ``graph`` argument as a one-hop ``LayerGraph`` whose destinations are the first rows of the layer's input:
    ``(lg, order, *edge_arrays)`` with every per-edge array (None passes through) in the hop's CSR order.

    ``graph`` is a ``[csr_row_ptr, csr_col_ind]`` pair (``n_dst`` is then its row count) or a COO ``edge_index`` [2, E] (row 0 =
    source j, row 1 = destination i; PyG) over ``n_dst`` destinations.  ``order`` (CSR edge k is COO edge ``order[k]``) is None
    when the edges are destination-major already: a CSR pair, or a loader's edge list; otherwise it is the order of a stable sort
    on the destination, so the CSR is the same on every route (edge order kept inside a destination).  int64 ids on the device
    go through ``wgamd_coo_to_csr_i64`` (one radix sort over the bits a destination id needs), anything else through the torch
    formulation of the same."""
    order = None
    ready = getattr(graph, "_wgamd_csr", None)      # (version, n_dst, row_ptr, col): made by the loader for its call group
    if isinstance(graph, (tuple, list)):
        row_ptr, col = graph[0], graph[1]
        _check_csr(row_ptr, col)
    elif ready is not None and ready[0] == graph._version and ready[1] == n_dst:
        row_ptr, col = ready[2], ready[3]
    # (the flag is the tensor's version counter at the time the loader vouched for the order: an in-place edit of the
    #  edge list afterwards — a permutation, self loops written into the same storage — bumps the counter and the sort runs)
    elif getattr(graph, "_wgamd_dst_sorted", None) == graph._version and graph.is_cuda:
        # the loaders' own edge lists are destination-major already (hop after hop, a hop's edges in the CSR order of its
        # frontier, every hop's destinations after the previous hop's): the CSR is a search for the run boundaries and a cast
        # — no sort (0.77 ms per 88 k-edge mini-batch through the radix sort below, most of it launch latency)
        dst = graph[1].contiguous()
        row_ptr = torch.searchsorted(dst, torch.arange(n_dst + 1, device=dst.device, dtype=dst.dtype)).to(torch.int32)
        col = graph[0].to(torch.int32).contiguous()
    elif graph.dtype == torch.int64 and graph.is_cuda:
        src, dst = graph[0].contiguous(), graph[1].contiguous()
        E, dev = dst.shape[0], dst.device
        row_ptr = torch.empty(n_dst + 1, dtype=torch.int32, device=dev)
        col = torch.empty(E, dtype=torch.int32, device=dev)
        order = torch.empty(E, dtype=torch.int32, device=dev)
        need = L.lib().wgamd_coo_to_csr_workspace_bytes(E, n_dst)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        L.check(L.lib().wgamd_coo_to_csr_i64(src.data_ptr(), dst.data_ptr(), E, n_dst, row_ptr.data_ptr(), col.data_ptr(),
                                             order.data_ptr(), ws.data_ptr(), need, get_stream()), "wgamd_coo_to_csr_i64")
    else:
        src, dst = graph[0], graph[1]
        order = torch.sort(dst, stable=True).indices
        col = src[order].to(torch.int32).contiguous()
        row_ptr = torch.zeros(n_dst + 1, dtype=torch.int32, device=dst.device)
        row_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n_dst), 0)
    lg = LayerGraph([HopGraph(row_ptr, col, _arange(row_ptr.shape[0] - 1, row_ptr.device))])
    return (lg, order) + tuple(t if t is None or order is None else t[order] for t in edge_arrays)


def _to_csr(edge_index, n_dst):
    """The destination-major CSR ``(row_ptr, col)`` of a COO ``edge_index`` (``_single_hop``)."""
    hop = _single_hop(edge_index, n_dst)[0].hops[0]
    return hop.row_ptr, hop.col


_ARANGE = {}


_HEADS_WGRAD_MIN_ROWS = 16384


class _HeadsTransform(torch.autograd.Function):
    """``y[n, h, :] = agg[n, h, :] @ w3[:, h, :]`` — the dense tail of the aggregate-first GAT layer (per-head weights on the
    destination rows).  Forward and the gradient of ``agg`` are library products of ordinary shapes; the WEIGHT gradient
    ``agg_h^T dY_h`` is a [F, n] x [n, C] product with n in the hundreds of thousands and a 128 x 64 result, which the library
    runs at 0.16 TB/s (2.07 ms per mag relation, 6 % of the whole mag run) — it goes to the split-K bf16x3 kernel of the SAGE
    layer's weight gradient instead (``wgamd_sage_wgrad_bf16x3``: ``dZ^T [A | B]`` with A, B = the two halves of agg_h's columns,
    so nothing is read twice), one launch + its partial-sum reduction per head."""

    @staticmethod
    def forward(ctx, agg3, w3, acc3=None):
        # one product per head, written straight into its columns of the [n, H, C] result: the batched form (einsum -> bmm)
        # leaves [H, n, C] and pays a 450 MB permute-copy per mag relation to bring it back (10 % of the mag training step).
        # ``acc3`` (the sum of the relations before this one, HeteroConv's aggregation): the products are added INTO it (beta =
        # 1) instead of a separate 3 x 450 MB addition per relation.
        ctx.save_for_backward(agg3, w3)
        n, H, F_ = agg3.shape
        C = w3.shape[2]
        if acc3 is not None:
            ctx.mark_dirty(acc3)
        if gat_transform_supported(F_, H, C) and agg3.is_contiguous() and (acc3 is None or acc3.is_contiguous()):
            # the inference route's kernel: all heads in ONE pass on the bf16 matrix pipe at fp32 accuracy, the running sum read and
            # written in place (the library's four [n, 128] x [128, 64] products run at 0.9 TB/s: 1.45 ms per mag relation)
            y = acc3 if acc3 is not None else torch.empty((n, H, C), dtype=torch.float32, device=agg3.device)
            gat_transform_heads_fused(agg3.view(n, H * F_), w3.reshape(F_, H * C).contiguous(), H,
                                      acc_in=None if acc3 is None else acc3.view(n, H * C), out=y.view(n, H * C))
            return y
        if acc3 is None:
            y = torch.empty((n, H, C), dtype=torch.float32, device=agg3.device)
            for h in range(H):
                torch.mm(agg3[:, h, :], w3[:, h, :], out=y[:, h, :])
            return y
        for h in range(H):
            acc3[:, h, :].addmm_(agg3[:, h, :], w3[:, h, :])
        return acc3

    @staticmethod
    def backward(ctx, g):
        agg3, w3 = ctx.saved_tensors
        g = g.contiguous()
        d_agg = None
        if ctx.needs_input_grad[0]:
            d_agg = torch.empty_like(agg3)
            for h in range(agg3.shape[1]):
                torch.mm(g[:, h, :], w3[:, h, :].t(), out=d_agg[:, h, :])
        d_w3 = None
        if ctx.needs_input_grad[1]:
            n, H, F_ = agg3.shape
            C = g.shape[2]
            split = F_ % 8 == 0                  # the halves of a row must start 16-byte aligned
            Fk = F_ // 2 if split else F_
            rows = _arange(n, g.device)
            buf = torch.empty((H, 2, C, Fk), dtype=torch.float32, device=g.device)
            for h in range(H):
                a_h = agg3[:, h, :]
                sage_wgrad(a_h[:, :Fk], a_h[:, Fk:] if split else a_h, rows, g[:, h, :], buf[h, 0], buf[h, 1])
            # buf[h, s, c, k] = d w3[s Fk + k, h, c]
            d_w3 = (buf.permute(1, 3, 0, 2).reshape(F_, H, C) if split else buf[:, 0].permute(2, 0, 1)).contiguous()
        return d_agg, d_w3, (g if len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2] else None)


def _heads_transform(agg3: torch.Tensor, w3: torch.Tensor, acc3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[acc3 +] agg3 @ w3`` per head; ``acc3`` ([n, H, C], the sum so far) may be updated in place and returned."""
    n, H, F_ = agg3.shape
    C = w3.shape[2]
    if (agg3.is_cuda and agg3.dtype == torch.float32 and agg3.is_contiguous() and n >= _HEADS_WGRAD_MIN_ROWS and F_ % 4 == 0
            and (H * F_) % 4 == 0 and (C % 4 == 0 or H == 1) and torch.is_grad_enabled() and w3.requires_grad
            and L.lib().wgamd_sage_wgrad_workspace_bytes(1, F_ // 2 if F_ % 8 == 0 else F_, C) > 0):
        if acc3 is not None and acc3.is_contiguous() and acc3.requires_grad and not acc3.is_leaf:
            return _HeadsTransform.apply(agg3, w3, acc3)
        y = _HeadsTransform.apply(agg3, w3)
        return y if acc3 is None else acc3 + y
    y = torch.einsum("nhf,fhc->nhc", agg3, w3)
    return y if acc3 is None else acc3 + y


def _arange(n: int, device) -> torch.Tensor:
    """``arange(n)`` int64 on ``device`` as a view of one grow-only buffer (the "self rows" of a mini-batch graph whose
    destinations are the first rows of x)."""
    buf = _ARANGE.get(device)
    if buf is None or buf.shape[0] < n:
        buf = torch.arange(max(n * 2, 1 << 16), dtype=torch.int64, device=device)
        _ARANGE[device] = buf
    return buf[:n]


def _split_graph(graph, n_dst):
    if isinstance(graph, (tuple, list)) and len(graph) == 2 and graph[0].dim() == 1:
        return graph[0], graph[1]          # [csr_row_ptr, csr_col_ind] as the sampler emits them
    return _to_csr(graph, n_dst)           # COO edge_index


class LazyRows:
    """``table[ids]`` that has not been gathered: what ``batch.x`` of a loader call group is when the feature table lives
    whole on this device (single GPU, or replicated).  ``nn.SAGEConv`` consumes it as it is — its first-layer kernel reads
    the table through ``ids`` (``src_ids`` of ``wgamd_sage_layer_fused_*``), so the ``[n, F]`` copy of the rows, the
    largest tensor of a mini-batch, is never written to HBM nor read back.  Anything else calls ``materialize()`` (one
    ``wholememory_gather``) or just uses it as a tensor: ``torch`` functions receive the gathered rows.

    A ``torch.float16`` / ``torch.bfloat16`` table (features stored in 16 bits, as the reference's examples store them): the
    values are converted to float32 exactly on the way out, as the reference's WholeMemory gather does, and the model runs in
    float32.  ``nn.SAGEConv`` reads the 16-bit rows in its layer kernel (half the bytes of the row fetch, bit for bit the result
    over ``table.float()``); ``materialize()`` returns **float32** rows (one converting gather, kept), which is what every other
    layer works on — it takes the route of a float32 tensor input holding ``table.float()[ids]``, so its result is that input's;
    ``dtype`` keeps returning the TABLE's dtype — the dtype of what is stored, not of what a layer computes on."""

    def __init__(self, table: torch.Tensor, ids: torch.Tensor):
        assert table.dim() == 2 and ids.dim() == 1 and ids.dtype in (torch.int32, torch.int64)
        self.table, self.ids, self._rows = table, ids.contiguous(), None

    @property
    def shape(self):
        return torch.Size((self.ids.shape[0], self.table.shape[1]))

    @property
    def dtype(self):
        return self.table.dtype

    @property
    def device(self):
        return self.table.device

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 2

    def materialize(self) -> torch.Tensor:
        if self._rows is None and getattr(self, "_gather", None) is not None:
            self._rows = self._gather()           # (a peer-mapped table: wholememory_gather over the mapping)
        if self._rows is None:
            from .tensor import local_gather
            dtype = torch.float32 if self.table.dtype in _X16 else self.table.dtype      # (a 16-bit store: converted once, here)
            self._rows = local_gather(self.table, self.ids, torch.empty(tuple(self.shape), dtype=dtype, device=self.table.device))
        return self._rows

    def __getitem__(self, index):
        return self.materialize()[index]

    def __len__(self):
        return int(self.ids.shape[0])

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        conv = lambda v: v.materialize() if isinstance(v, LazyRows) else v   # noqa: E731
        return func(*[conv(a) for a in args], **{k: conv(v) for k, v in (kwargs or {}).items()})


class MappedTable:
    """The address space of a PEER-MAPPED feature table (CHUNKED / CONTINUOUS handle whose partitions live on several GPUs of a
    node, each mapped into this process) as the layer kernels take it: a base pointer, the row width, and rows given as BYTE
    offsets from the base (``wgamd_mapped_row_offsets``).  Quacks like the [rows, F] float32 tensor the wrappers expect; it is
    never indexed from Python."""
    byte_offset_ids = True
    dtype, is_cuda, requires_grad = torch.float32, True, False

    def __init__(self, base_ptr: int, width: int, device):
        self._ptr, self.shape, self.device = int(base_ptr), torch.Size((0, int(width))), device

    def data_ptr(self):
        return self._ptr

    def dim(self):
        return 2

    def stride(self, d=None):
        st = (int(self.shape[1]), 1)
        return st if d is None else st[d]


def mapped_lazy_rows(wm_tensor, ids: torch.Tensor) -> LazyRows:
    """``table[ids]`` of a peer-mapped ``DistributedWholeMemoryTensor`` (float32 [rows, F]) as ``LazyRows`` the first SAGE layer
    reads through: one small launch turns the ids into byte offsets over this process's mapping of every rank's partition, the
    layer kernel then loads remote rows over xGMI itself (the reference's mapped gather addresses the partitions the same way,
    gather_scatter_func.cuh:242-505) — the gathered ``[n, F]`` copy never exists.  Anything else that touches it gathers."""
    import ctypes
    assert wm_tensor.dtype == torch.float32 and wm_tensor.dim() == 2 and ids.dim() == 1 and ids.dtype in (torch.int32, torch.int64)
    ids = ids.contiguous()
    offs = torch.empty(ids.shape[0], dtype=torch.int64, device=ids.device)
    base = ctypes.c_void_p()
    L.check(L.lib().wgamd_mapped_row_offsets(wm_tensor.c, ids.data_ptr(), torch_dtype_to_wm(ids.dtype), int(ids.shape[0]),
                                             offs.data_ptr(), ctypes.byref(base), get_stream()), "wgamd_mapped_row_offsets")
    lazy = LazyRows(MappedTable(base.value, wm_tensor.shape[1], ids.device), offs)
    lazy._gather = lambda: wm_tensor.gather(ids)
    return lazy


class _Transposed:
    """What ``HopGraph.transposed`` / ``input_dst`` keep of a hop seen from its input rows, under ``key`` = (n_src, capture epoch)."""
    __slots__ = ("key", "row_ptr_t", "col_t", "self_t", "perm", "input_dst")

    def __init__(self, key):
        self.key = key
        self.row_ptr_t = self.col_t = self.self_t = self.perm = self.input_dst = None


class HopGraph:
    """One sampled hop as a layer consumes it: CSR over the hop's destination rows (``row_ptr`` int32 [n + 1]), ``col`` int32
    = row of every edge's source IN THE LAYER'S INPUT, ``self_rows`` int64 [n] = input row of every destination itself."""

    def __init__(self, row_ptr, col, self_rows):
        self.row_ptr, self.col, self.self_rows = row_ptr, col, self_rows
        self._t = None
        self.inv_deg = None     # float32 [n] = 1 / max(degree, 1) when whoever built the hop has it (loader.StagedBatch)

    @property
    def n_rows(self):
        return int(self.row_ptr.shape[0]) - 1

    def with_self_loops(self):
        """``(row_ptr, col)`` of the hop with every destination's own input row in front of its sampled neighbours — what
        ``csr_add_self_loop`` (graph_op.h:44-48) does for a square CSR, here with ``self_rows`` as the diagonal; made once."""
        epoch = _graph_epoch()
        if getattr(self, "_loops", None) is None or self._loops_key != epoch:
            self._loops_key = epoch
            from . import graph_ops
            n = self.n_rows
            rp, col = graph_ops.add_csr_self_loop(self.row_ptr, self.col)     # row i = [i] ++ row i (csr_add_self_loop) ...
            col[rp[:n].long()] = self.self_rows.to(torch.int32)              # ... with the destination's own input row as i
            self._loops = (rp, col)
        return self._loops

    def transposed(self, n_src: int, need_self: bool = True, need_perm: bool = False):
        """The hop seen from its ``n_src`` input rows, for the backward pass — computed once per hop and kept, whichever layers
        and however many backward calls use it: ``(row_ptr_t, col_t, self_t)`` with the source-major CSR of
        ``wgamd_csr_transpose_i32`` (entries = destination rows, hop order inside a source: deterministic sums) and
        ``self_t[j]`` = ``n_rows + i`` where input row j is destination i itself (``self_rows`` is injective: every
        destination is a different vertex of its mini-batch), ``2 n_rows`` otherwise — the row indices ``_sage_dx`` reads its
        stacked gradient through; ``self_t`` is None without ``need_self``.  With ``need_perm`` a fourth entry, ``perm`` int32:
        the hop's CSR edge of every transposed entry (how per-edge arrays are read source-major; one element when the hop
        has no edges)."""
        # (under HIP-graph capture the hop's arrays are fixed buffers REFILLED before every replay: the transpose must be part
        #  of the graph, once per capture)
        key = (n_src, _graph_epoch())
        t = self._t
        if t is None or t.key != key:
            t = self._t = _Transposed(key)
        if t.row_ptr_t is None or (need_perm and t.perm is None):      # (a perm asked for later: the transpose runs again)
            dev = self.row_ptr.device
            if self.col.shape[0] > 0:
                t.row_ptr_t, t.perm, _, t.col_t = _csr_transpose(self.row_ptr, self.col, n_src, want_perm=need_perm, want_col_t=True)
            else:
                t.row_ptr_t, t.col_t = torch.zeros(n_src + 1, dtype=torch.int32, device=dev), self.col
                t.perm = torch.zeros(1, dtype=torch.int32, device=dev) if need_perm else None
        if need_self and t.self_t is None:     # (only the layer kernel over the transposed hop reads it: three launches)
            n, dev = self.n_rows, self.row_ptr.device
            t.self_t = torch.full((n_src,), 2 * n, dtype=torch.int64, device=dev)
            t.self_t[self.self_rows] = torch.arange(n, 2 * n, dtype=torch.int64, device=dev)
        res = (t.row_ptr_t, t.col_t, t.self_t)
        return res + (t.perm,) if need_perm else res

    def input_dst(self, n_src: int):
        """int64 [n_src]: the destination row that input row j is itself, -1 where there is none — the ``self_rows`` of a
        GCN / RGCN layer kernel run over the transposed hop; kept with ``transposed``."""
        self.transposed(n_src, need_self=False)
        t = self._t
        if t.input_dst is None:
            dev = self.row_ptr.device
            t.input_dst = torch.full((n_src,), -1, dtype=torch.int64, device=dev)
            t.input_dst[self.self_rows] = torch.arange(self.n_rows, dtype=torch.int64, device=dev)
        return t.input_dst


class LayerGraph:
    """The hops ONE layer of a trimmed GNN runs over (``cugraph_pyg_amd.loader.CallGroup.layer_graph``): the layer's output
    is the hops' destination lists back to back — hop h's rows start at ``sum(n_rows of the hops before it)``."""

    def __init__(self, hops):
        self.hops = list(hops)
        # GCNConv's degrees of the layer's INPUT rows: a callable -> (hops, out_base, n_in), the hops whose destination rows are
        # those input rows (out_base[h] = input row of hop h's row 0, or -1: row i is input row self_rows[i]); set by the
        # loader (CallGroup.layer_graph), None for a user-built graph
        self.degree_source = None

    @property
    def n_rows(self):
        return sum(h.n_rows for h in self.hops)


def _hops(lg: LayerGraph):
    """``(hop, rows, edges)`` for every hop of ``lg``: the hop with the slices of the layer's output rows and of its hop-major
    per-edge arrays that are the hop's."""
    at = eat = 0
    for h in lg.hops:
        n, E = h.n_rows, int(h.col.shape[0])
        yield h, slice(at, at + n), slice(eat, eat + E)
        at += n
        eat += E


def _sum_over_hops(lg: LayerGraph, zeros_shape, device, per_hop):
    """The sum, in hop order, of the tensors ``per_hop(hop, rows, edges, k)`` returns for the hops of ``lg`` that have rows (hop k
    with its ``_hops`` slices; the first tensor is added to in place).  Every hop empty: float32 zeros of ``zeros_shape``."""
    total = None
    for k, (h, rows, edges) in enumerate(_hops(lg)):
        if h.n_rows > 0:
            part = per_hop(h, rows, edges, k)
            total = part if total is None else total.add_(part)
    return torch.zeros(zeros_shape, dtype=torch.float32, device=device) if total is None else total


def _edge_dst(row_ptr, n_edges: int, first: int = 0):
    """int64 [n_edges]: the destination row of every CSR edge, rows numbered from ``first``."""
    n = row_ptr.shape[0] - 1
    return torch.repeat_interleave(torch.arange(first, first + n, device=row_ptr.device), (row_ptr[1:] - row_ptr[:-1]).long(),
                                   output_size=int(n_edges))


def _kernel_rows_ok(t) -> bool:
    """``t`` [rows, F] is what the layer kernels read in place: float32 on the device, unit column stride, 16-B aligned rows."""
    return (t.dtype == torch.float32 and t.is_cuda and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)


def _table_through_ids(x):
    """``(table, ids)`` when the kernels may read the ``LazyRows`` input ``x`` in place through its node list — a tensor table
    that is ``_kernel_rows_ok``, int64 ids, rows not gathered yet —, None otherwise (the caller works on ``materialize()``)."""
    if isinstance(x, LazyRows) and isinstance(x.table, torch.Tensor) and x.ids.dtype == torch.int64 and _kernel_rows_ok(x.table) \
            and x._rows is None:
        return x.table, x.ids
    return None


def _terms_by_id(rows_of_table: int, listed_rows: int) -> bool:
    """The attention terms of a table read through a node list are those of the TABLE's rows, which the relation kernels read
    through the list, when the table is at most half as long as the list: a call group lists a table row once per mini-batch
    that sampled it, so a short table's terms cost fewer rows than the list's (made in every call, nothing kept between calls)."""
    return 2 * rows_of_table <= listed_rows


def _lazy_table_grad_error():
    """What a gradient into a feature table read through ids is refused with."""
    return NotImplementedError("gradient w.r.t. a feature table read through ids (LazyRows): trainable node "
                               "embeddings go through wholegraph_amd.embedding, or pass x = emb[n_id]")


def _refuse_lazy_table_grad(table):
    """NotImplementedError when autograd is on and ``table``, the table of a ``LazyRows`` input, requires a gradient."""
    if torch.is_grad_enabled() and getattr(table, "requires_grad", False):
        raise _lazy_table_grad_error()


def _sum_of(tensors):
    """The sum of same-shaped tensors (the biases or root weights of the relations ending in a node type): None for none, the
    tensor itself for one, ``torch.stack(..).sum(0)`` otherwise — one reduction, not chained adds: the bits depend on it."""
    if len(tensors) < 2:
        return tensors[0] if tensors else None
    return torch.stack(tensors).sum(0)


def _layer_input(layer, x, lg: LayerGraph, F_: int):
    """The input of a layer over ``lg`` as the one-kernel layers take it: ``(src, ids, n_src, n_edges)`` — the rows the kernel
    reads (a ``LazyRows`` input: its table), the node list it reads them through (None: by row), the input's row count, and the
    edge count the layer's per-edge arrays cover (a call group's layer graph: the whole group's, every layer reads the prefix
    of its hops; any other: its hops').  ValueError when x is not ``F_`` wide; NotImplementedError for a gradient through a
    lazy table."""
    lazy = isinstance(x, LazyRows)
    if x.shape[1] != F_:
        raise ValueError("%s: x has %d features, the layer takes %d" % (type(layer).__name__, x.shape[1], F_))
    src = x.table if lazy else x
    if lazy:
        _refuse_lazy_table_grad(src)
    total = getattr(lg, "num_group_edges", None)
    n_edges = total if total is not None else sum(int(h.col.shape[0]) for h in lg.hops)
    return src, (x.ids if lazy else None), (len(x) if lazy else x.shape[0]), n_edges


def _x16_as_rows(x):
    """``x``, or — for a ``LazyRows`` over a float16 / bfloat16 table — its float32 rows (``materialize()``: one converting
    gather, kept): the layers other than ``SAGEConv`` then take whatever route a float32 tensor input takes."""
    if isinstance(x, LazyRows) and x.table.dtype in _X16:
        _refuse_lazy_table_grad(x.table)
        return x.materialize()
    return x


def _refuse_featureless(layer, x):
    """ValueError unless ``x`` holds node features (a floating tensor or ``LazyRows``)."""
    if not isinstance(x, LazyRows) and not (torch.is_tensor(x) and x.is_floating_point()):
        raise ValueError("%s: featureless input (x = None or node indices) is not supported; pass node features"
                         % type(layer).__name__)


_SAGE_DX_SMALL_ROWS = 16384


def _sage_dx(hop: HopGraph, gz: torch.Tensor, w_l: torch.Tensor, w_r: torch.Tensor, w_bwd, mean: bool, n_src: int):
    """Gradient of one hop of the SAGE layer w.r.t. its input rows:
    ``dX[j] = sum_{edges (i, j)} dZ[i] W_l / (deg_i if mean) + [j == self(i)] dZ[i] W_r``.
    This is the one-kernel layer itself run over the TRANSPOSED hop — sum aggregation of the destination gradients an input
    row feeds, "self" = its own destination's gradient, weight ``[W_l ; W_r]`` — so it runs on the same kernel
    (``wgamd_sage_layer_fused_*``): the stacked operand ``[dZ / deg ; dZ ; 0]`` is the only tensor built for it.  Shapes
    that kernel does not take go through the segmented transposed SpMM + library GEMMs."""
    n, N = gz.shape
    F_ = w_l.shape[1]
    Nq = (N + 3) // 4 * 4
    # A SMALL hop (one mini-batch: PerBatchStep) goes through the dense products + the segmented transposed SpMM instead: in the
    # transposed hop a popular source is a row of hundreds of entries, which one lane group of the layer kernel walks as a
    # chain of dependent loads — hidden inside a call group's millisecond launch, 250 us of a mini-batch's step when exposed
    # (profiles/r06); the segmented SpMM cuts long rows into pieces.
    if w_bwd is not None and sage_layer_fused_supported(Nq, F_) and n > _SAGE_DX_SMALL_ROWS:
        row_ptr_t, col_t, self_t = hop.transposed(n_src)
        xs = torch.zeros((2 * n + 1, Nq), dtype=torch.float32, device=gz.device)
        if mean:
            deg = (hop.row_ptr[1:] - hop.row_ptr[:-1]).clamp_(min=1).unsqueeze(1)
            torch.div(gz, deg, out=xs[:n, :N])
        else:
            xs[:n, :N] = gz
        xs[n:2 * n, :N] = gz
        return sage_layer_fused_forward(row_ptr_t, col_t, xs, self_t, w_bwd, None, relu=False, mean=False)
    if n <= _SAGE_DX_SMALL_ROWS and n > 0 and hop.col.shape[0] > 0:
        # the hop's own (kept) transpose + the segmented SpMM; self_rows is injective, so the W_r term is a plain indexed add
        row_ptr_t, col_t, _ = hop.transposed(n_src, need_self=False)
        g = gz
        if mean:
            g = gz * hop.inv_deg.unsqueeze(1) if hop.inv_deg is not None \
                else gz / (hop.row_ptr[1:] - hop.row_ptr[:-1]).clamp_(min=1).unsqueeze(1)
        return _spmm_csr_segmented(row_ptr_t, col_t, n_src, g @ w_l).index_add_(0, hop.self_rows, gz @ w_r)
    gx = spmm_csr_backward(hop.row_ptr, hop.col, gz @ w_l, n_src, mean)
    return gx.index_add_(0, hop.self_rows, gz @ w_r)


def _sage_layer_launch(ctx, src, w_l, w_r, bias, conv, graph, ids, relu, mean):
    """The layer's launches (one per hop of ``graph``); ``ctx`` = the autograd context of ``_SageLayer`` (then the aggregate is
    kept wherever a gradient is needed) or None."""
    N, F_ = w_l.shape
    Np = _padded_width(N)
    keep = ctx is not None and any(ctx.needs_input_grad[:4])
    buf = torch.empty((graph.n_rows, Np), dtype=torch.float32, device=src.device)
    # under HIP-graph capture (a per-mini-batch training step: the weights change on every replay) the kernel's operand is made
    # from the parameters by ONE launch; otherwise the cached transposed / padded / split forms
    prepared = None
    if _capturing() and sage_layer_fused_supported(F_, Np) and _pick_precision(F_, Np, None) == "bf16x3" \
            and w_l.stride(1) == 1 and w_r.stride(1) == 1:
        # (a mini-batch's few thousand rows at a width of half tiles: whole 32-row tiles — sage_layer_small_launch)
        prepared = sage_layer_planes(w_l, w_r, bias, Np, full_tiles=all(sage_layer_small_launch(F_, h.n_rows) for h in graph.hops))
    w_t, aggs = (None if prepared is not None else conv._weight_t()), []
    for h, rows, _ in _hops(graph):
        n = h.n_rows
        agg = torch.empty((n, F_), dtype=torch.float32, device=src.device) if keep and n > 0 else None
        if n > 0:
            sage_layer_fused_forward(h.row_ptr, h.col, src, h.self_rows, w_t, bias, relu=relu, mean=mean, src_ids=ids,
                                     out=buf[rows, :N], agg_out=agg, prepared=prepared)
        aggs.append(agg)
    out = buf[:, :N]
    if keep:
        if ctx.needs_input_grad[0] and ids is not None:
            raise _lazy_table_grad_error()
        if isinstance(src, torch.Tensor):
            ctx.save_for_backward(src, w_l, w_r, out)
        else:                                     # (a MappedTable: an address space, not a tensor)
            ctx.save_for_backward(w_l, w_r, out)
            ctx.src_obj = src
        ctx.conv, ctx.graph, ctx.ids, ctx.relu, ctx.mean, ctx.aggs, ctx.has_bias = conv, graph, ids, relu, mean, aggs, bias is not None
    return out


class _SageLayer(torch.autograd.Function):
    """The one-kernel SAGE layer over a ``LayerGraph`` with its backward pass on the HIP kernels.  Forward: the inference
    launch (``wgamd_sage_layer_fused_bf16x3``), which under autograd also keeps the aggregate half of its operand (same
    bits in the output).  Backward: ``sage_wgrad`` per hop (ReLU mask folded in when the input needs no gradient) and, when
    the input rows need a gradient (every layer but the one that reads the features), ``_sage_dx`` over the hop's
    transpose — computed once per hop (``HopGraph.transposed``)."""

    @staticmethod
    def forward(ctx, src, w_l, w_r, bias, conv, graph, ids, relu, mean):
        return _sage_layer_launch(ctx, src, w_l, w_r, bias, conv, graph, ids, relu, mean)

    @staticmethod
    def backward(ctx, g):
        _released(ctx.aggs, "SAGEConv", "aggregates", "; run the forward again, or sum the losses before calling backward")
        src, w_l, w_r, out = ctx.saved_tensors if len(ctx.saved_tensors) == 4 else (ctx.src_obj,) + tuple(ctx.saved_tensors)
        graph, ids, relu, mean = ctx.graph, ctx.ids, ctx.relu, ctx.mean
        N, F_ = w_l.shape
        need_x = ctx.needs_input_grad[0]
        if g.stride(1) != 1 or g.dtype != torch.float32:
            g = g.contiguous().float()
        act = out if relu else None
        if relu and need_x:
            g, act = torch.ops.aten.threshold_backward(g, out, 0), None      # dZ once, read by both gradients
        gwl, gwr = torch.empty_like(w_l, memory_format=torch.contiguous_format), torch.empty_like(w_r, memory_format=torch.contiguous_format)
        gb = torch.empty(N, dtype=torch.float32, device=g.device) if ctx.has_bias else None
        w_bwd = ctx.conv._weight_bwd() if need_x and any(h.n_rows > _SAGE_DX_SMALL_ROWS for h in graph.hops) else None
        # (not _sum_over_hops: a hop's weight gradient launch goes right before its input gradient, and x may need none)
        gx, first = None, True
        for (h, rows, _), agg in zip(_hops(graph), ctx.aggs):
            if h.n_rows > 0:
                xs, self_rows, xs_ids = src, h.self_rows, ids
                if src.dtype in _X16:
                    # a 16-bit table: the weight-gradient kernel reads float32 rows — the hop's self rows, one converting gather
                    from .tensor import local_gather
                    xs = local_gather(src, h.self_rows if ids is None else ids[h.self_rows],
                                      torch.empty((h.n_rows, F_), dtype=torch.float32, device=g.device))
                    self_rows, xs_ids = _arange(h.n_rows, g.device), None
                sage_wgrad(agg, xs, self_rows, g[rows], gwl, gwr, gb, None if act is None else act[rows], src_ids=xs_ids,
                           accumulate=not first)
                first = False
                if need_x:
                    gh = _sage_dx(h, g[rows], w_l, w_r, w_bwd, mean, src.shape[0])
                    gx = gh if gx is None else gx.add_(gh)
        if first:
            gwl.zero_(), gwr.zero_()
            if gb is not None:
                gb.zero_()
        if need_x and gx is None:
            gx = torch.zeros_like(src)
        ctx.aggs = None
        return gx, gwl, gwr, gb, None, None, None, None, None


class SAGEConv(torch.nn.Module):
    """``out = lin_l(mean_{j in N(i)} x_j) + lin_r(x_i)`` (PyG ``SAGEConv``, aggr mean|sum).

    ``forward(x, graph)``: ``graph`` = the hop's ``[csr_row_ptr, csr_col_ind]`` or a COO ``edge_index`` (the reference's call
    shapes, gnn_model.py:178-199), or a ``LayerGraph`` of a loader call group — then the whole layer (feature fetch when
    ``x`` is a ``LazyRows``, aggregation, both linear maps, bias and the optional ``act="relu"``) is ONE kernel per hop
    (``wgamd_sage_layer_fused_*``) where the shape allows it, aggregation kernel + library GEMM otherwise.

    A ``LazyRows`` over a ``torch.float16`` / ``torch.bfloat16`` table takes the one-kernel route wherever a float32 table
    would: the kernel loads the 16-bit rows (2 bytes per feature instead of 4 on the launch's largest stream) and converts them
    to float32 exactly, so output, kept aggregate and gradients are those of the float32 layer over ``table.float()`` — the
    forward bit for bit.  The weight gradient gets the hop's self rows as float32 from one converting gather.  Every other
    route (an unsupported shape, ``root_weight=False``, aggregate + GEMM) receives float32 rows from one converting gather.  A
    gradient into the table stays refused."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, aggr: str = "mean",
                 root_weight: bool = True, bias: bool = True):
        super().__init__()
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels, self.aggr, self.root_weight = in_channels, out_channels, aggr, root_weight
        self.lin_l = torch.nn.Linear(in_channels[0], out_channels, bias=bias)
        self.lin_r = torch.nn.Linear(in_channels[1], out_channels, bias=False) if root_weight else None
        self._wgamd_derived = {}       # (``_derived``'s store, here from the start: a forward adds no attribute to the module)

    def _weight_bwd(self):
        """``[W_l ; W_r]`` ([2 Nq, F], Nq = N rounded up to 4, zero rows between) — the weight of the layer kernel when it runs
        the input gradient over the transposed hop (``_sage_dx``); None when that kernel does not take the shape."""
        wl, wr = self.lin_l.weight, self.lin_r.weight
        N, F_ = wl.shape
        Nq = (N + 3) // 4 * 4
        if not sage_layer_fused_supported(Nq, F_):
            return None

        def build():
            w = torch.zeros((2 * Nq, F_), dtype=torch.float32, device=wl.device)
            w[:N], w[Nq:Nq + N] = wl, wr
            return w
        return _derived(self, "w_bwd", (wl, wr), build)

    def _weight_t(self):
        """``cat([W_l, W_r], 1).t()`` ([2F, N]) for the one-kernel layer, rebuilt when a weight changed (``_derived``)."""
        wl, wr = self.lin_l.weight, self.lin_r.weight
        return _derived(self, "w_t", (wl, wr), lambda: torch.cat([wl, wr], dim=1).t().contiguous())

    def _forward_layer(self, x, graph: LayerGraph, act=None):
        lazy = isinstance(x, LazyRows)
        src = x.table if lazy else x
        F_, N = src.shape[1], self.out_channels
        relu = act == "relu"
        assert act in (None, "relu"), "act: None or 'relu'"
        x16 = lazy and src.dtype in _X16
        if x16 and not (self.lin_r is not None and self.aggr in ("mean", "sum") and isinstance(src, torch.Tensor) and src.is_cuda
                        and src.stride(1) == 1 and src.stride(0) % 4 == 0 and src.data_ptr() % 8 == 0
                        and sage_layer_fused_supported(F_, N) and _FUSED_PRECISION == "bf16x3"
                        and L.lib().wgamd_sage_layer_x16_supported(F_, _padded_width(N), torch_dtype_to_wm(src.dtype))):
            # a 16-bit table on a route that is not the bf16x3 layer kernel's: float32 rows from ONE converting gather, then
            # whatever a float32 tensor input takes
            _refuse_lazy_table_grad(src)
            x = src = x.materialize()
            lazy = x16 = False
        one_kernel = (self.lin_r is not None and self.aggr in ("mean", "sum") and (src.dtype == torch.float32 or x16) and src.is_cuda
                      and src.stride(1) == 1 and sage_layer_fused_preferred(F_, N))
        if one_kernel and not sage_layer_train_supported(F_, N):
            # (a shape only the fp32-MFMA layer kernel takes has no backward kernels: under autograd it runs as aggregation
            #  kernel + library GEMM, whose autograd pieces exist for every shape)
            one_kernel = not (torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                                           or (not lazy and x.requires_grad)))
        if one_kernel:
            args = (src, self.lin_l.weight, self.lin_r.weight, self.lin_l.bias, self, graph, x.ids if lazy else None, relu,
                    self.aggr == "mean")
            if not (torch.is_grad_enabled() and (self.lin_l.weight.requires_grad or self.lin_r.weight.requires_grad
                                                 or (not lazy and x.requires_grad))):
                return _sage_layer_launch(None, *args)       # same launches; no autograd node to build (~10 us per call)
            return _SageLayer.apply(*args)
        # aggregation kernel(s) + library GEMM: every hop's [mean | self] rows, then lin_l / lin_r as torch modules
        xd = x.materialize() if lazy else x
        outs = []
        for h in graph.hops:
            agg = spmm_csr(xd, h.row_ptr, h.col, self.aggr)
            o = self.lin_l(agg)
            if self.lin_r is not None:
                o = o + self.lin_r(xd[h.self_rows])
            outs.append(o)
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        return torch.relu_(out) if relu else out

    def forward(self, x, graph, act=None):
        if isinstance(graph, LayerGraph):
            return self._forward_layer(x, graph, act)
        if isinstance(x, LazyRows):
            x = x.materialize()
        x_src, x_dst = (x, x) if isinstance(x, torch.Tensor) else x
        row_ptr, col = _split_graph(graph, x_dst.shape[0])
        # ((x, x_target) with x_target = x[:n], the reference's call shape gnn_model.py:178-199: the same rows)
        same = x_src is x_dst or (x_dst.data_ptr() == x_src.data_ptr() and x_dst.stride() == x_src.stride())
        if (same and x_src.is_cuda and x_src.dtype == torch.float32
                and self.lin_r is not None and self.aggr in ("mean", "sum") and act in (None, "relu")
                and x_src.stride(1) == 1 and sage_layer_fused_preferred(x_src.shape[1], self.out_channels)):
            # one sampled (sub)graph whose destinations are the first rows of x: the whole layer as ONE kernel, forward and
            # backward (no library GEMM — whose shape heuristics alone cost ~1 ms for every new row count a mini-batch brings)
            n = row_ptr.shape[0] - 1
            # the hop (and with it its transpose, for the backward pass) belongs to the GRAPH, not to the layer: every layer a
            # model runs over one edge_index shares it
            keep = getattr(graph, "_wgamd_hop", None) if isinstance(graph, torch.Tensor) else None
            if keep is not None and keep[0] == graph._version and keep[1] == n and keep[2].row_ptr is row_ptr:
                lg = keep[3]
            else:
                lg = LayerGraph([HopGraph(row_ptr, col, _arange(n, x_src.device))])
                if isinstance(graph, torch.Tensor):
                    try:
                        graph._wgamd_hop = (graph._version, n, lg.hops[0], lg)
                    except AttributeError:
                        pass
            return self._forward_layer(x_src, lg, act)
        out = self.lin_l(spmm_csr(x_src, row_ptr, col, self.aggr))
        if self.lin_r is not None:
            out = out + self.lin_r(x_dst[: out.shape[0]])
        return torch.relu_(out) if act == "relu" else out


class GATConv(torch.nn.Module):
    """PyG ``GATConv`` (shared ``lin``, ``att_src``/``att_dst``, LeakyReLU 0.2, per-destination
    softmax, concat or mean over heads, optional self loops)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, add_self_loops: bool = True, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.add_self_loops = concat, negative_slope, add_self_loops
        self.lin = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels)) if bias else None
        bound = math.sqrt(6.0 / (heads + out_channels))
        torch.nn.init.uniform_(self.att_src, -bound, bound)
        torch.nn.init.uniform_(self.att_dst, -bound, bound)

    def _forward_layer(self, x, lg: LayerGraph, act=None):
        """A trimmed layer of a loader call group (``CallGroup.layer_graph(j)``), AGGREGATE-FIRST: per hop one
        ``_GatAggregateHeads`` launch over the untransformed input rows (a ``LazyRows`` input is read through its node list, its
        attention terms are those of the table's rows when the table is the shorter side), self loops as an extra leading
        neighbour, then the per-head weights, bias and activation on the hop's destination rows.  Under autograd the same
        code trains (``wgamd_gat_aggregate_heads_bwd_f32``)."""
        assert act in (None, "relu")
        H, C, F_ = self.heads, self.out_channels, self.in_channels
        lazy = _table_through_ids(x)
        if lazy is not None:
            X, ids = lazy
            by_id = _terms_by_id(X.shape[0], len(x))
            rows = X if by_id else x.materialize()
        else:
            X = x.materialize() if isinstance(x, LazyRows) else x
            ids, by_id, rows = None, False, X
        w3 = self.lin.weight.t().reshape(F_, H, C)
        folds = torch.cat([(w3 * self.att_src.view(1, H, C)).sum(-1), (w3 * self.att_dst.view(1, H, C)).sum(-1)], 1)
        terms = _NarrowTerms.apply(rows, folds)
        a_src, a_dst = terms[:, :H], terms[:, H:]
        outs = []
        for hop in lg.hops:
            n = hop.n_rows
            if n == 0:
                continue
            rp, col = hop.with_self_loops() if self.add_self_loops else (hop.row_ptr, hop.col)
            if col.shape[0] == 0:         # (no self loops and nothing sampled: the aggregate of an empty neighbourhood)
                outs.append(torch.zeros((n, H, C), dtype=torch.float32, device=X.device))
                continue
            agg = _GatAggregateHeads.apply(X, a_src, a_dst, rp, col, H, hop.self_rows, ids, ids if by_id else None, by_id, by_id,
                                           self.negative_slope)
            outs.append(_heads_transform(agg.view(n, H, F_), w3))
        out = torch.cat(outs) if outs else torch.zeros((0, H, C), dtype=torch.float32, device=X.device)
        out = out.reshape(out.shape[0], H * C) if self.concat else out.mean(1)
        if self.bias is not None:
            out = out + self.bias
        return torch.relu(out) if act == "relu" else out

    def forward(self, x, graph, act=None):
        # (folded attention vectors, weight tiles, pooled buffers: cached against the parameters' versions)
        _refuse_capture(self, "derived-weight caches")
        from . import graph_ops
        if isinstance(graph, LayerGraph):
            if self.in_channels % 4 == 0 and self.in_channels <= 256 and self.heads in (1, 2, 4, 8):
                return self._forward_layer(x, graph, act)
            raise NotImplementedError("GATConv over a call group's LayerGraph: in_channels % 4 == 0, <= 256; heads 1, 2, 4 or 8")
        assert act is None, "act: only with a call group's LayerGraph"
        x_src, x_dst = (x, x) if isinstance(x, torch.Tensor) else x
        H, C = self.heads, self.out_channels
        n_dst = x_dst.shape[0]
        row_ptr, col = _split_graph(graph, n_dst)
        if self.add_self_loops:
            # destinations are the first n_dst sources (sampler layout), so "self" = own row index
            row_ptr, col = graph_ops.add_csr_self_loop(row_ptr, col)
        h_src = self.lin(x_src)
        h_dst = h_src[:n_dst] if x_dst is x_src or x_dst.data_ptr() == x_src.data_ptr() else self.lin(x_dst)
        a_src = (h_src.view(-1, H, C) * self.att_src).sum(-1)
        a_dst = (h_dst.view(-1, H, C) * self.att_dst).sum(-1)
        out = _GatCsr.apply(h_src, a_src, a_dst, row_ptr, col, H, self.negative_slope)
        if not self.concat:
            out = out.view(-1, H, C).mean(1)
        if self.bias is not None:
            out = out + self.bias
        return out


# ---------------------------------------------------------------------------------------------------------------------
# GCN (torch_geometric.nn.GCNConv; the model of the reference's cugraph-pyg example gcn_dist_mnmg.py) — csrc/wg_gcn.hip
# ---------------------------------------------------------------------------------------------------------------------
GCN_ADD_SELF_LOOPS, GCN_RELU, GCN_MAX_HOPS = 1, 2, 8     # WGAMD_GCN_* (include/wgamd_ext.h)


def gcn_layer_supported(F_: int, N: int) -> bool:
    """Shapes of the one-kernel GCN layer (``wgamd_gcn_layer_f32``): F % 4 == 0, F <= 256, N <= 256."""
    return bool(L.lib().wgamd_gcn_layer_supported(int(F_), int(N)))


def gcn_degrees(hops, out_base, n_out: int, fill: float = 1.0, add_self_loops: bool = True, edge_weights=None, device=None):
    """``dinv`` float32 [n_out] = deg^-1/2 of gcn_norm for the rows the hops' destinations are (``wgamd_gcn_degrees_f32``, one
    launch): row i of hop h is entry ``out_base[h] + i``, or ``self_rows[i]`` when ``out_base[h] < 0``.  Entries no hop reaches
    have in-degree 0: their degree is the added loop alone (``fill``), or 0 without self loops (factor 0)."""
    import ctypes
    hops = list(hops)
    if len(hops) > GCN_MAX_HOPS:
        raise ValueError("gcn_degrees: at most %d hops" % GCN_MAX_HOPS)
    device = device if device is not None else hops[0].row_ptr.device
    default = 1.0 / math.sqrt(fill) if add_self_loops and fill > 0 else 0.0
    dinv = torch.full((int(n_out),), default, dtype=torch.float32, device=device)
    if not hops:
        return dinv
    for h in hops:
        _check_csr(h.row_ptr, h.col)
        assert h.self_rows.dtype == torch.int64 and h.self_rows.is_contiguous()
    n = len(hops)
    P, I = ctypes.c_void_p * n, ctypes.c_int64 * n
    cols = [_nonempty(h.col, torch.int32) for h in hops]
    ew = None
    if edge_weights is not None:
        for w in edge_weights:
            assert w is None or (w.dtype == torch.float32 and w.is_contiguous())
        ew = P(*[_ptr(w) for w in edge_weights])
    L.check(L.lib().wgamd_gcn_degrees_f32(
        n, P(*[h.row_ptr.data_ptr() for h in hops]), P(*[c.data_ptr() for c in cols]), P(*[h.self_rows.data_ptr() for h in hops]),
        ew, I(*[h.n_rows for h in hops]), I(*[int(b) for b in out_base]), float(fill), int(bool(add_self_loops)), dinv.data_ptr(),
        int(n_out), get_stream()), "wgamd_gcn_degrees_f32")
    return dinv


def gcn_layer_forward(row_ptr, col, x, self_rows, weight, bias=None, dinv_src=None, dinv_dst=None, fill=1.0, add_self_loops=False,
                      relu=False, src_ids=None, edge_weight=None, out=None, agg_out=None):
    """A whole GCN layer over one hop in ONE kernel: ``act(agg @ weight^T + bias)`` with the normalised aggregate ``agg`` of
    ``wgamd_gcn_layer_f32`` (include/wgamd_ext.h); ``weight`` is [N, F] (``torch.nn.Linear`` layout).  ``agg_out`` ([n_rows, F]):
    the launch also keeps the aggregate (``_train``)."""
    hop = _hop_args(row_ptr, col, x, src_ids)
    n_rows, F_, N = row_ptr.shape[0] - 1, x.shape[1], weight.shape[0]
    assert weight.dtype == torch.float32 and weight.stride(1) == 1
    assert weight.shape[1] == F_ and self_rows.dtype == torch.int64 and self_rows.is_contiguous()
    out = _out_rows(out, n_rows, N, row_ptr.device)
    flags = (GCN_ADD_SELF_LOOPS if add_self_loops else 0) | (GCN_RELU if relu else 0)
    common = hop + (self_rows.data_ptr(), _ptr(edge_weight), _ptr(dinv_src), _ptr(dinv_dst), float(fill), weight.data_ptr(),
                    weight.stride(0), N, _ptr(bias), flags, out.data_ptr(), out.stride(0))
    if agg_out is not None:
        assert agg_out.shape == (n_rows, F_) and agg_out.stride(1) == 1
        L.check(L.lib().wgamd_gcn_layer_f32_train(*common, agg_out.data_ptr(), agg_out.stride(0), get_stream()),
                "wgamd_gcn_layer_f32_train")
    else:
        L.check(L.lib().wgamd_gcn_layer_f32(*common, get_stream()), "wgamd_gcn_layer_f32")
    return out


def gcn_aggregate(row_ptr, col, x, self_rows, dinv_src=None, dinv_dst=None, fill=1.0, add_self_loops=False, src_ids=None,
                  edge_weight=None, out=None):
    """The normalised aggregate of the GCN layer alone, any F (``wgamd_gcn_aggregate_f32``): what shapes outside the layer
    kernel's domain multiply with a library GEMM."""
    hop = _hop_args(row_ptr, col, x, src_ids)
    assert self_rows.dtype == torch.int64 and self_rows.is_contiguous()
    out = _out_rows(out, row_ptr.shape[0] - 1, x.shape[1], row_ptr.device)
    L.check(L.lib().wgamd_gcn_aggregate_f32(
        *hop, self_rows.data_ptr(), _ptr(edge_weight), _ptr(dinv_src), _ptr(dinv_dst), float(fill),
        GCN_ADD_SELF_LOOPS if add_self_loops else 0, out.data_ptr(), out.stride(0), get_stream()), "wgamd_gcn_aggregate_f32")
    return out


def gcn_wgrad(agg, grad_out, grad_w, grad_bias=None, act_out=None, accumulate=False, max_split=None):
    """``grad_w (+)= dZ^T agg``, ``grad_bias (+)= colsum(dZ)``, ``dZ = grad_out * (act_out > 0)`` (``wgamd_gcn_wgrad_f32``:
    deterministic split-K; ``max_split``: over up to that many row ranges, ``wgamd_gcn_wgrad_split_f32``)."""
    n, F_ = agg.shape
    N = grad_out.shape[1]
    assert agg.stride(1) == 1 and grad_out.stride(1) == 1 and grad_w.shape == (N, F_) and grad_w.is_contiguous()
    assert act_out is None or (act_out.shape == grad_out.shape and act_out.stride(1) == 1)
    lib = L.lib()
    need = (lib.wgamd_gcn_wgrad_workspace_bytes(int(n), F_, N) if max_split is None
            else lib.wgamd_gcn_wgrad_split_workspace_bytes(int(n), F_, N, int(max_split)))
    ws = torch.empty(max(int(need), 4), dtype=torch.uint8, device=agg.device)
    head = (agg.data_ptr(), agg.stride(0), n, F_, grad_out.data_ptr(), grad_out.stride(0), _ptr(act_out),
            0 if act_out is None else act_out.stride(0), N, grad_w.data_ptr(), _ptr(grad_bias), int(bool(accumulate)))
    tail = (ws.data_ptr(), ws.numel(), get_stream())
    if max_split is None:
        L.check(lib.wgamd_gcn_wgrad_f32(*head, *tail), "wgamd_gcn_wgrad_f32")
    else:
        L.check(lib.wgamd_gcn_wgrad_split_f32(*head, int(max_split), *tail), "wgamd_gcn_wgrad_split_f32")


def _dense_wgrad(lg: LayerGraph, a, gz, w, want_b: bool, act):
    """``(dW, db)`` of a dense product ``z = a @ w^T + b`` whose rows are the hops of ``lg`` back to back: ``gz^T a`` and (with
    ``want_b``, else None) ``colsum(gz)``, ``gz`` masked by ``act > 0`` when ``act`` is given — one ``gcn_wgrad`` per hop with rows,
    accumulated in hop order; zeros when no hop has rows."""
    gw = torch.empty_like(w, memory_format=torch.contiguous_format)
    gb = torch.empty(w.shape[0], dtype=torch.float32, device=gz.device) if want_b else None
    first = True
    for h, rows, _ in _hops(lg):
        if h.n_rows > 0:
            gcn_wgrad(a[rows], gz[rows], gw, gb, None if act is None else act[rows], accumulate=not first)
            first = False
    if first:
        gw.zero_()
        if gb is not None:
            gb.zero_()
    return gw, gb


def _gcn_input_grad(hop, g, n_src, dinv_in, conv, edge_weight, weight=None):
    """``A_hat^T g`` over one hop (rows = the layer's input rows), times ``weight`` ([F, Nq], the layer's W^T zero-padded to
    Nq rows) when given: the GCN kernel run over the hop's transpose — destination rows become the summed rows, so the
    per-row factor and the per-edge factor swap places (``dinv_dst`` = the input rows', ``dinv_src`` = the destinations')."""
    if edge_weight is None:
        row_ptr_t, col_t, _ = hop.transposed(n_src, need_self=False)
        w_t = None
    else:
        row_ptr_t, col_t, _, perm = hop.transposed(n_src, need_self=False, need_perm=True)
        w_t = edge_weight[perm[:hop.col.shape[0]]]
    self_t = hop.input_dst(n_src)
    d_out = dinv_in[hop.self_rows] if dinv_in is not None else None
    loops = conv.normalize and conv.add_self_loops
    if weight is None:
        return gcn_aggregate(row_ptr_t, col_t, g, self_t, dinv_src=d_out, dinv_dst=dinv_in, fill=conv._fill, add_self_loops=loops,
                             edge_weight=w_t)
    return gcn_layer_forward(row_ptr_t, col_t, g, self_t, weight, dinv_src=d_out, dinv_dst=dinv_in, fill=conv._fill,
                             add_self_loops=loops, edge_weight=w_t)


def _gcn_launch_args(conv, dinv_in):
    return dict(dinv_src=dinv_in, fill=conv._fill, add_self_loops=conv.normalize and conv.add_self_loops)


class _GcnLayer(torch.autograd.Function):
    """The one-kernel GCN layer over a ``LayerGraph`` (one ``wgamd_gcn_layer_f32`` launch per hop; under autograd the
    ``_train`` form keeps the aggregate).  Backward: ``wgamd_gcn_wgrad_f32`` per hop (dW, db) and, when the input rows need a
    gradient, the same layer kernel over every hop's transpose with ``W^T`` as the weight (dX = A_hat^T dZ W)."""

    @staticmethod
    def forward(ctx, src, weight, bias, conv, graph, dinv_in, ids, relu, edge_weights, n_src):
        N, F_ = weight.shape
        keep = any(ctx.needs_input_grad[:3])
        out = torch.empty((graph.n_rows, N), dtype=torch.float32, device=weight.device)
        w = weight.detach()
        b = bias.detach() if bias is not None else None
        agg = torch.empty((graph.n_rows, F_), dtype=torch.float32, device=weight.device) if ctx.needs_input_grad[1] else None
        for k, (h, rows, _) in enumerate(_hops(graph)):
            if h.n_rows > 0:
                gcn_layer_forward(h.row_ptr, h.col, src, h.self_rows, w, b, relu=relu, src_ids=ids,
                                  edge_weight=None if edge_weights is None else edge_weights[k], out=out[rows],
                                  agg_out=None if agg is None else agg[rows], **_gcn_launch_args(conv, dinv_in))
        if keep:
            ctx.save_for_backward(weight, out)
            # (kept is a 1-tuple: agg is None when the weight needs no gradient, and None itself is what _released reads as released)
            ctx.conv, ctx.graph, ctx.dinv_in, ctx.relu, ctx.edge_weights, ctx.n_src, ctx.kept = \
                conv, graph, dinv_in, relu, edge_weights, n_src, (agg,)
        return out

    @staticmethod
    def backward(ctx, g):
        _released(ctx.kept, "GCNConv", "aggregates")
        weight, out = ctx.saved_tensors
        (agg,) = ctx.kept
        N, F_ = weight.shape
        graph, n_src, dev = ctx.graph, ctx.n_src, g.device
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g = g.contiguous().float()
        act = out if ctx.relu else None
        if ctx.relu and need_x:
            g, act = torch.ops.aten.threshold_backward(g, out, 0), None      # dZ once, read by both gradients
        gx = gw = gb = None
        if need_w:
            gw, gb = _dense_wgrad(graph, agg, g, weight, need_b, act)
        elif need_b:      # (no aggregate was kept: the hops' column sums in torch)
            gb = _sum_over_hops(graph, (N,), dev, lambda h, rows, _, k: (g[rows] if act is None else g[rows] * (act[rows] > 0)).sum(0))
        if need_x:
            Nq = (N + 3) // 4 * 4
            w_bwd, gq, ew = _padded_wt(weight, Nq), _pad_cols(g, Nq), ctx.edge_weights
            gx = _sum_over_hops(graph, (n_src, F_), dev, lambda h, rows, _, k: _gcn_input_grad(
                h, gq[rows], n_src, ctx.dinv_in, ctx.conv, None if ew is None else ew[k], weight=w_bwd))
        ctx.kept = None
        return gx, gw, gb, None, None, None, None, None, None, None


class _GcnAggregate(torch.autograd.Function):
    """The normalised aggregate over every hop of a ``LayerGraph`` (``wgamd_gcn_aggregate_f32``), rows back to back; backward =
    the same kernel over the hops' transposes.  The route of shapes the one-kernel layer does not take."""

    @staticmethod
    def forward(ctx, x, conv, graph, dinv_in, edge_weights):
        aggs = []
        for k, h in enumerate(graph.hops):
            if h.n_rows > 0:
                aggs.append(gcn_aggregate(h.row_ptr, h.col, x, h.self_rows,
                                          edge_weight=None if edge_weights is None else edge_weights[k],
                                          **_gcn_launch_args(conv, dinv_in)))
        ctx.conv, ctx.graph, ctx.dinv_in, ctx.edge_weights, ctx.n_src = conv, graph, dinv_in, edge_weights, x.shape[0]
        if not aggs:
            return torch.zeros((0, x.shape[1]), dtype=torch.float32, device=x.device)
        return aggs[0] if len(aggs) == 1 else torch.cat(aggs)

    @staticmethod
    def backward(ctx, g):
        g, ew = g.contiguous(), ctx.edge_weights
        gx = _sum_over_hops(ctx.graph, (ctx.n_src, g.shape[1]), g.device, lambda h, rows, _, k: _gcn_input_grad(
            h, g[rows], ctx.n_src, ctx.dinv_in, ctx.conv, None if ew is None else ew[k]))
        return gx, None, None, None, None


class GCNConv(torch.nn.Module):
    """PyG ``GCNConv`` (``flow="source_to_target"``, sum aggregation): ``x' = D^-1/2 (A + L) D^-1/2 (x W^T) + b`` with the
    self loops of ``add_remaining_self_loops`` (a node with a loop edge keeps that loop's weight; ``fill`` = 2 when
    ``improved``, else 1).  Parameters as PyG names them (``lin.weight`` glorot, ``bias`` zeros), so a PyG ``state_dict`` loads.

    ``forward(x, graph, act=None, edge_weight=None)``: ``graph`` = a COO ``edge_index`` (the ``for batch in loader`` loop of
    gcn_dist_mnmg.py; output rows = x's rows), a ``[csr_row_ptr, csr_col_ind]`` pair (destinations = the first rows of x), or a
    call group's ``LayerGraph`` with ``x`` a tensor or ``LazyRows`` (degrees from the untrimmed mini-batch graph, which the
    loader attaches).  The layer — feature fetch, normalised aggregation, ``x W^T``, bias, optional ``act="relu"`` — is ONE
    kernel per hop (``wgamd_gcn_layer_f32``) for F % 4 == 0, F <= 256, N <= 256; other shapes run the normalised-aggregate
    kernel and a library GEMM."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False,
                 add_self_loops: bool = True, normalize: bool = True, bias: bool = True):
        super().__init__()
        if cached:
            raise ValueError("GCNConv(cached=True): the graph of a mini-batch changes on every call; nothing can be cached")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops, self.normalize = improved, cached, add_self_loops, normalize
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.lin.weight)     # glorot, as PyG's Linear(weight_initializer="glorot")
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    @property
    def _fill(self) -> float:
        return 2.0 if self.improved else 1.0

    def _dinv(self, lg: LayerGraph, device):
        """dinv of the layer's input rows (None without normalisation), computed once per layer graph and configuration."""
        if not self.normalize:
            return None
        key = (self._fill, bool(self.add_self_loops))
        cache = getattr(lg, "_gcn_dinv", None)
        if cache is None:
            cache = lg._gcn_dinv = {}
        if key not in cache:
            if lg.degree_source is None:
                raise ValueError("GCNConv over a LayerGraph needs the degrees of its input rows in the untrimmed mini-batch "
                                 "graph: use CallGroup.layer_graph(j) (it attaches them), or set LayerGraph.degree_source")
            hops, base, n_in = lg.degree_source()
            cache[key] = gcn_degrees(hops, base, n_in, self._fill, self.add_self_loops,
                                     edge_weights=getattr(lg, "_gcn_edge_weights", None), device=device)
        return cache[key]

    def _forward_layer(self, x, lg: LayerGraph, act=None, edge_weights=None):
        assert act in (None, "relu"), "act: None or 'relu'"
        relu = act == "relu"
        F_, N = self.in_channels, self.out_channels
        x = _x16_as_rows(x)
        src, ids, n_src, _ = _layer_input(self, x, lg, F_)
        dinv = self._dinv(lg, src.device)
        if gcn_layer_supported(F_, N) and _kernel_rows_ok(src):
            return _GcnLayer.apply(src, self.lin.weight, self.bias, self, lg, dinv, ids, relu, edge_weights, n_src)
        xd = x.materialize() if isinstance(x, LazyRows) else x
        agg = _GcnAggregate.apply(xd.contiguous().float(), self, lg, dinv, edge_weights)
        out = torch.nn.functional.linear(agg, self.lin.weight, self.bias)
        return torch.relu(out) if relu else out

    def forward(self, x, graph, act=None, edge_weight=None):
        _refuse_capture(self, "per-graph degree caches")      # (degrees and transposes, cached against the graph object)
        if edge_weight is not None and torch.is_grad_enabled() and edge_weight.requires_grad:
            raise NotImplementedError("GCNConv: no gradient w.r.t. edge_weight")
        if isinstance(graph, LayerGraph):
            if edge_weight is not None:
                raise ValueError("GCNConv: edge_weight is not taken with a call group's LayerGraph (its edges are unweighted)")
            return self._forward_layer(x, graph, act)
        if isinstance(x, LazyRows):
            x = x.materialize()
        n_src = x.shape[0]
        lg, _, w = _single_hop(graph, n_src, edge_weight)
        hop = lg.hops[0]
        lg.degree_source = lambda: ([hop], [0], n_src)
        lg._gcn_edge_weights = None if w is None else [w.to(torch.float32).contiguous()]
        return self._forward_layer(x, lg, act, lg._gcn_edge_weights)


# ---------------------------------------------------------------------------------------------------------------------
# RGCN (torch_geometric.nn.RGCNConv / FastRGCNConv; the model of the reference's cugraph-pyg example
# rgcn_link_class_mnmg.py) — csrc/wg_rgcn.hip
# ---------------------------------------------------------------------------------------------------------------------
_RGCN_PAIRS_PER_ITEM_MIN, _RGCN_MAX_ITEMS = 256, 1024


def rgcn_layer_supported(F_: int, N: int, B: int, has_root: bool = True) -> bool:
    """Shapes of the one-kernel RGCN layer (``wgamd_rgcn_layer_f32``): F % 4 == 0, N <= 256, (B + root) F <= 1024."""
    return bool(L.lib().wgamd_rgcn_layer_supported(int(F_), int(N), int(B), int(bool(has_root))))


_RGCN_LONG_ROW = 4096      # rows longer than this count relations by a sort (the ballot count is quadratic in the degree)


def _rgcn_check_types(edge_type, R: int, n_edges: int, device):
    """Refuse relation ids of the wrong type, device, count or range (ValueError) — the range once per tensor version: the
    kernels never read ids from another device nor index with one outside [0, R), and this is where the caller learns of it."""
    if not torch.is_tensor(edge_type) or edge_type.dtype not in (torch.int32, torch.int64) or edge_type.dim() != 1:
        raise ValueError("RGCNConv: edge_type must be a 1-D int32 or int64 tensor")
    if edge_type.device != torch.device(device):
        raise ValueError("RGCNConv: edge_type is on %s, the graph on %s" % (edge_type.device, torch.device(device)))
    if edge_type.shape[0] != n_edges:
        raise ValueError("RGCNConv: edge_type has %d entries for %d edges" % (edge_type.shape[0], n_edges))
    key = (edge_type.data_ptr(), edge_type._version, edge_type.shape[0], int(R))
    if getattr(edge_type, "_wgamd_rgcn_checked", None) == key:
        return
    if edge_type.numel() > 0 and bool(((edge_type < 0) | (edge_type >= R)).any()):
        raise ValueError("RGCNConv: a relation id lies outside [0, %d)" % R)
    edge_type._wgamd_rgcn_checked = key


def rgcn_edge_coef(row_ptr, edge_type, R: int, mean: bool = True, long_rows: bool = False):
    """Per-edge ``(rel int32, coef float32)`` of one hop (``wgamd_rgcn_edge_coef``, one launch): ``coef[e]`` = 1 / the number of
    edges of e's destination row with e's relation (``mean``), else 1.  ``edge_type`` (int32 / int64, ids in [0, R), on the
    graph's device) is in CSR order.  ``long_rows``: the hop has rows of more than ``_RGCN_LONG_ROW`` edges (a COO or CSR
    graph over a whole power-law graph): the counts come from one sort of (row, relation) keys instead."""
    assert row_ptr.dtype == torch.int32 and row_ptr.is_cuda and row_ptr.is_contiguous()
    assert edge_type.device == row_ptr.device, "edge_type must be on the graph's device"
    E, dev = edge_type.shape[0], row_ptr.device
    et = edge_type.contiguous()
    if long_rows and E > 0:
        rel = et.to(torch.int32)
        if not mean:
            return rel, torch.ones(E, dtype=torch.float32, device=dev)
        _, inv, cnt = torch.unique(_edge_dst(row_ptr, E) * R + et.long(), return_inverse=True, return_counts=True)
        return rel, 1.0 / cnt.to(torch.float32)[inv]
    rel = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    coef = torch.empty(max(E, 1), dtype=torch.float32, device=dev)
    if E > 0:
        L.check(L.lib().wgamd_rgcn_edge_coef(row_ptr.data_ptr(), row_ptr.shape[0] - 1, et.data_ptr(), torch_dtype_to_wm(et.dtype),
                                             int(R), int(bool(mean)), rel.data_ptr(), coef.data_ptr(), get_stream()),
                "wgamd_rgcn_edge_coef")
    return rel[:E], coef[:E]


def rgcn_layer_forward(row_ptr, col, x, self_rows, rel, coef, wt, comp, B: int, has_root: bool, bias=None, relu=False, src_ids=None,
                       out=None):
    """A whole RGCN layer over one hop in ONE kernel (``wgamd_rgcn_layer_f32``, include/wgamd_ext.h): ``wt`` is the stacked weight
    transposed, [N, (B + root) F] (``_rgcn_stacked``); ``comp`` [R, B], or None for the identity (B = R)."""
    hop = _hop_args(row_ptr, col, x, src_ids)
    N = wt.shape[0]
    assert wt.dtype == torch.float32 and wt.stride(1) == 1
    assert self_rows is None or (self_rows.dtype == torch.int64 and self_rows.is_contiguous())
    assert rel.dtype == torch.int32 and coef.dtype == torch.float32 and rel.shape[0] == col.shape[0] == coef.shape[0]
    out = _out_rows(out, row_ptr.shape[0] - 1, N, row_ptr.device)
    L.check(L.lib().wgamd_rgcn_layer_f32(
        *hop, _ptr(self_rows), _nonempty(rel, torch.int32).data_ptr(), _nonempty(coef, torch.float32).data_ptr(), _ptr(comp), int(B),
        int(bool(has_root)), wt.data_ptr(), wt.stride(0), N, _ptr(bias), int(bool(relu)), out.data_ptr(), out.stride(0),
        get_stream()), "wgamd_rgcn_layer_f32")
    return out


def rgcn_wgrad(x, pair_src, pair_dst, pair_coef, seg, n_seg: int, grad, src_ids=None):
    """``M[s] = sum_{pairs p of segment s} pair_coef[p] X[pair_src[p]]^T grad[pair_dst[p]]`` -> float32 [n_seg, F, N]
    (``wgamd_rgcn_wgrad_f32``): one stable sort of the pairs by segment, work items of at most S pairs of one segment, partial
    sums added in item order — the same bits from run to run."""
    F_, N, P, dev = x.shape[1], grad.shape[1], pair_src.shape[0], grad.device
    assert grad.dtype == torch.float32 and grad.stride(1) == 1 and x.stride(1) == 1
    M = torch.empty((n_seg, F_, N), dtype=torch.float32, device=dev)
    order = torch.sort(seg, stable=True).indices
    ps, pd, pc = pair_src[order].contiguous(), pair_dst[order].contiguous(), pair_coef[order].contiguous()
    S = max(_RGCN_PAIRS_PER_ITEM_MIN, (-(-P // _RGCN_MAX_ITEMS) + 3) // 4 * 4)
    cnt = torch.bincount(seg, minlength=n_seg)
    seg_ptr = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
    item_start = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
    seg_ptr[1:] = torch.cumsum(cnt, 0)
    item_start[1:] = torch.cumsum((cnt + S - 1) // S, 0)
    max_items = -(-P // S) + n_seg if P > 0 else 0
    ws = torch.empty(max(int(L.lib().wgamd_rgcn_wgrad_workspace_bytes(max_items, F_, N)), 4), dtype=torch.uint8, device=dev)
    ids_ptr, ids_dt = _ids_args(x, src_ids)
    L.check(L.lib().wgamd_rgcn_wgrad_f32(
        x.data_ptr(), x.stride(0), F_, ids_ptr, ids_dt, _nonempty(ps, torch.int64).data_ptr(), _nonempty(pd, torch.int64).data_ptr(),
        _nonempty(pc, torch.float32).data_ptr(), grad.data_ptr(), grad.stride(0), N, item_start.data_ptr(), seg_ptr.data_ptr(),
        n_seg, S, max_items, M.data_ptr(), ws.data_ptr(), ws.numel(), get_stream()), "wgamd_rgcn_wgrad_f32")
    return M


def _rgcn_stacked(weight, root, Nq=None):
    """The kernel's transposed stacked weight.  Forward (``Nq`` None): [N, (B + root) F] with column b F + f = basis_b[f, :].
    Input gradient: [F, (B + root) Nq] with column b Nq + n = basis_b[:, n] (the rows of basis_b^T), N zero-padded to Nq."""
    w = weight.detach()
    B, F_, N = w.shape
    r = None if root is None else root.detach()
    if Nq is None:
        parts = [w.reshape(B * F_, N)] + ([] if r is None else [r])
        return torch.cat(parts).t().contiguous()
    if Nq != N:
        w = torch.nn.functional.pad(w, (0, Nq - N))
        r = None if r is None else torch.nn.functional.pad(r, (0, Nq - N))
    parts = [w.permute(1, 0, 2).reshape(F_, B * Nq)] + ([] if r is None else [r])
    return torch.cat(parts, 1).contiguous()


class _RgcnLayer(torch.autograd.Function):
    """The one-kernel RGCN layer over a ``LayerGraph`` (one ``wgamd_rgcn_layer_f32`` launch per hop); nothing is kept but the
    per-edge coefficients and the output.  Backward: ``wgamd_rgcn_wgrad_f32`` once over every hop's (source, destination)
    pairs segmented by relation, the root's self pairs as segment R (dW = M[:R], or dbasis = comp^T M[:R] and dcomp = M[:R]
    basis^T; droot = M[R]) and, when the input rows need a gradient, the layer kernel over every hop's transpose with
    [basis_b^T; root^T] as the weight."""

    @staticmethod
    def forward(ctx, src, weight, comp, root, bias, conv, graph, coefs, ids, relu, n_src):
        B, F_, N = weight.shape
        out = torch.empty((graph.n_rows, N), dtype=torch.float32, device=weight.device)
        wt = _rgcn_stacked(weight, root)
        c = None if comp is None else comp.detach().contiguous()
        b = None if bias is None else bias.detach()
        for (h, rows, _), (rel, coef) in zip(_hops(graph), coefs):
            if h.n_rows > 0:
                rgcn_layer_forward(h.row_ptr, h.col, src, h.self_rows, rel, coef, wt, c, B, root is not None, b, relu=relu, src_ids=ids,
                                   out=out[rows])
        if any(ctx.needs_input_grad[:5]):
            ctx.save_for_backward(weight, comp, root, out)
            ctx.src, ctx.ids, ctx.graph, ctx.coefs, ctx.relu, ctx.n_src, ctx.R = src, ids, graph, coefs, relu, n_src, conv.num_relations
        return out

    @staticmethod
    def backward(ctx, g):
        _released(ctx.coefs, "RGCNConv", "per-edge coefficients")
        weight, comp, root, out = ctx.saved_tensors
        B, F_, N = weight.shape
        R, dev = ctx.R, g.device
        need_x, need_w, need_c, need_r, need_b = ctx.needs_input_grad[:5]
        gz = g.contiguous().float()
        if ctx.relu:
            gz = torch.ops.aten.threshold_backward(gz, out, 0)
        gx = gw = gc = gr = gb = None
        if need_w or need_c or need_r:
            ps, pd, pc, sg = [], [], [], []
            for (h, rows, _), (rel, coef) in zip(_hops(ctx.graph), ctx.coefs):
                n = h.n_rows
                ps.append(h.col.long())
                pd.append(_edge_dst(h.row_ptr, h.col.shape[0], rows.start))
                pc.append(coef)
                sg.append(rel.long())
                if root is not None:
                    ps.append(h.self_rows)
                    pd.append(torch.arange(rows.start, rows.stop, dtype=torch.int64, device=dev))
                    pc.append(torch.ones(n, dtype=torch.float32, device=dev))
                    sg.append(torch.full((n,), R, dtype=torch.int64, device=dev))
            M = rgcn_wgrad(ctx.src, torch.cat(ps), torch.cat(pd), torch.cat(pc), torch.cat(sg), R + (root is not None), gz,
                           src_ids=ctx.ids)
            if comp is None:
                gw = M[:R] if need_w else None
            else:
                Mr = M[:R].reshape(R, F_ * N)
                gw = (comp.detach().t() @ Mr).view(B, F_, N) if need_w else None
                gc = Mr @ weight.detach().reshape(B, F_ * N).t() if need_c else None
            gr = M[R] if need_r else None
        if need_b:
            gb = gz.sum(0)
        if need_x:
            Nq = (N + 3) // 4 * 4
            w_bwd, gq, coefs, n_src = _rgcn_stacked(weight, root, Nq), _pad_cols(gz, Nq), ctx.coefs, ctx.n_src
            c = None if comp is None else comp.detach().contiguous()

            def input_grad(h, rows, _, k):      # the layer kernel over hop k's transpose, per-edge arrays in the transposed order
                row_ptr_t, col_t, _, perm = h.transposed(n_src, need_self=False, need_perm=True)
                p, (rel, coef) = perm[:h.col.shape[0]], coefs[k]
                return rgcn_layer_forward(row_ptr_t, col_t, gq[rows], h.input_dst(n_src), rel[p], coef[p], w_bwd, c, B, root is not None)
            gx = _sum_over_hops(ctx.graph, (n_src, F_), dev, input_grad)
        ctx.src = ctx.coefs = None
        return gx, gw, gc, gr, gb, None, None, None, None, None, None


def _rgcn_library_ops(conv, x, lg: LayerGraph, coefs, relu: bool):
    """The layer composed of library ops under autograd, from the same per-edge coefficients: the route of shapes outside the
    one-kernel layer's domain (correctness, not speed).  Per hop: the per-relation sums H [n, R, F] (or per-basis, [n, B, F],
    when there are fewer bases than relations), then one GEMM against the stacked weight."""
    R, F_, N = conv.num_relations, conv.in_channels, conv.out_channels
    by_basis = conv.comp is not None and conv.num_bases < R
    if by_basis:
        Wk, K = conv.weight, conv.num_bases
    else:
        Wk, K = conv._relation_weights(), R
    outs = []
    for h, (rel, coef) in zip(lg.hops, coefs):
        n = h.n_rows
        dst = _edge_dst(h.row_ptr, h.col.shape[0])
        xs = x[h.col.long()]
        if by_basis:
            w_e = coef.unsqueeze(1) * conv.comp[rel.long()]                   # [E, B]
            H = x.new_zeros((n, K, F_)).index_add(0, dst, w_e.unsqueeze(2) * xs.unsqueeze(1))
        else:
            H = x.new_zeros((n * K, F_)).index_add(0, dst * K + rel.long(), coef.unsqueeze(1) * xs)
        o = H.reshape(n, K * F_) @ Wk.reshape(K * F_, N)
        if conv.root is not None:
            o = o + x[h.self_rows] @ conv.root
        outs.append(o)
    out = torch.cat(outs) if outs else x.new_zeros((0, N))
    if conv.bias is not None:
        out = out + conv.bias
    return torch.relu(out) if relu else out


class RGCNConv(torch.nn.Module):
    """PyG ``RGCNConv`` (``FastRGCNConv`` is the same class): ``x'_i = sum_r agg_{j in N_r(i)} x_j W_r + x_i root + bias``, with
    ``agg`` the per-relation mean (``aggr="mean"``) or sum (``"add"`` / ``"sum"``) and, with ``num_bases``, ``W_r = sum_b
    comp[r, b] weight[b]``.  Parameters as PyG names them (``weight`` [B or R, in, out], ``comp`` [R, B], ``root`` [in, out],
    ``bias``; glorot, bias zeros), so a PyG ``state_dict`` loads.

    ``forward(x, graph, edge_type, act=None)``: ``graph`` = a COO ``edge_index`` with ``edge_type`` [E] (the ``for batch in
    loader`` loop of rgcn_link_class_mnmg.py with ``rel[batch.e_id]``; output rows = x's rows), a ``[csr_row_ptr, csr_col_ind]``
    pair with ``edge_type`` in CSR order (destinations = the first rows of x), or a call group's ``LayerGraph`` with ``x`` a
    tensor or ``LazyRows`` and ``edge_type`` hop-major in ``CallGroup.e_id`` order (``CallGroup.edge_attr``; every layer takes
    the same tensor and reads the prefix of its hops).  The layer — feature fetch, per-relation mean, the product with the
    stacked weight, bias, optional ``act="relu"`` — is ONE kernel per hop (``wgamd_rgcn_layer_f32``) for F % 4 == 0, N <= 256,
    (B + root) F <= 1024 (B = R without bases), and the input gradient is the same kernel over the hop's transpose.  When x
    needs a gradient the transposed shape (F' = N rounded up to 4, N' = F) must fit as well; if either does not, the WHOLE
    layer, forward included, runs library ops over the same per-edge coefficients (correct, not fast, not bitwise
    reproducible).  ``edge_type`` must be on the graph's device; ids outside [0, R) or a wrong count raise ValueError."""

    def __init__(self, in_channels: int, out_channels: int, num_relations: int, num_bases: Optional[int] = None,
                 num_blocks: Optional[int] = None, aggr: str = "mean", root_weight: bool = True, is_sorted: bool = False,
                 bias: bool = True):
        super().__init__()
        if num_blocks is not None:
            raise NotImplementedError("RGCNConv: num_blocks (block-diagonal decomposition) is not supported")
        if aggr not in ("mean", "add", "sum"):
            raise ValueError("RGCNConv: aggr must be 'mean', 'add' or 'sum' (got %r)" % (aggr,))
        if num_relations < 1 or (num_bases is not None and num_bases < 1):
            raise ValueError("RGCNConv: num_relations and num_bases must be positive")
        self.in_channels, self.out_channels, self.num_relations = in_channels, out_channels, num_relations
        self.num_bases, self.num_blocks, self.aggr, self.is_sorted = num_bases, num_blocks, aggr, is_sorted
        if num_bases is not None:
            self.weight = torch.nn.Parameter(torch.empty(num_bases, in_channels, out_channels))
            self.comp = torch.nn.Parameter(torch.empty(num_relations, num_bases))
        else:
            self.weight = torch.nn.Parameter(torch.empty(num_relations, in_channels, out_channels))
            self.register_parameter("comp", None)
        if root_weight:
            self.root = torch.nn.Parameter(torch.empty(in_channels, out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for p in (self.weight, self.comp, self.root):     # PyG's glorot: U(-a, a), a = sqrt(6 / (size(-2) + size(-1)))
            if p is not None:
                a = math.sqrt(6.0 / (p.size(-2) + p.size(-1)))
                torch.nn.init.uniform_(p, -a, a)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    @property
    def _b_eff(self) -> int:
        return self.num_bases if self.num_bases is not None else self.num_relations

    def _relation_weights(self):
        """W_r [R, in, out] (autograd through comp and weight)."""
        if self.comp is None:
            return self.weight
        return (self.comp @ self.weight.reshape(self.num_bases, -1)).view(self.num_relations, self.in_channels, self.out_channels)

    def _coefs(self, lg: LayerGraph, edge_type):
        """Per hop ``(rel, coef)`` from the hop-major ``edge_type``: hop k reads the slice after the edges of hops < k."""
        mean = self.aggr == "mean"
        key = (edge_type._version, self.num_relations, mean)
        cache = getattr(lg, "_rgcn_coefs", None)
        if cache is not None and cache[0] is edge_type and cache[1] == key:     # (the tensor itself: a new one at a reused
            return cache[2]                                                     #  address is not the old one)
        coefs = [rgcn_edge_coef(h.row_ptr, edge_type[edges], self.num_relations, mean, long_rows=getattr(h, "_rgcn_long_rows", False))
                 for h, _, edges in _hops(lg)]
        lg._rgcn_coefs = (edge_type, key, coefs)
        return coefs

    def _forward_layer(self, x, lg: LayerGraph, edge_type, act=None):
        assert act in (None, "relu"), "act: None or 'relu'"
        relu = act == "relu"
        F_, N = self.in_channels, self.out_channels
        x = _x16_as_rows(x)
        src, ids, n_src, n_edges = _layer_input(self, x, lg, F_)
        _rgcn_check_types(edge_type, self.num_relations, n_edges, lg.hops[0].row_ptr.device if lg.hops else src.device)
        coefs = self._coefs(lg, edge_type)
        has_root, B = self.root is not None, self._b_eff
        need_x = torch.is_grad_enabled() and ids is None and x.requires_grad
        Nq = (N + 3) // 4 * 4
        if (rgcn_layer_supported(F_, N, B, has_root) and (not need_x or rgcn_layer_supported(Nq, F_, B, has_root))
                and _kernel_rows_ok(src)):
            return _RgcnLayer.apply(src, self.weight, self.comp, self.root, self.bias, self, lg, coefs, ids, relu, n_src)
        xd = x.materialize() if isinstance(x, LazyRows) else x
        return _rgcn_library_ops(self, xd.float(), lg, coefs, relu)

    def forward(self, x, graph, edge_type, act=None):
        _refuse_capture(self, "per-graph caches")             # (per-edge coefficients and transposes)
        _refuse_featureless(self, x)
        if isinstance(graph, HeteroLayerGraph):
            raise NotImplementedError("RGCNConv over a heterogeneous call group's layer graph is not supported")
        if isinstance(graph, LayerGraph):
            return self._forward_layer(x, graph, edge_type, act)
        if isinstance(x, LazyRows):
            x = x.materialize()
        # (graph[1]: the CSR pair's col, or the COO list's destinations — one entry per edge either way)
        _rgcn_check_types(edge_type, self.num_relations, graph[1].shape[0], graph[0].device)
        lg, _, et = _single_hop(graph, x.shape[0], edge_type)
        et._wgamd_rgcn_checked = (et.data_ptr(), et._version, et.shape[0], int(self.num_relations))
        hop = lg.hops[0]
        if hop.n_rows > 0:                             # (these paths may synchronise: the range check above does)
            hop._rgcn_long_rows = int((hop.row_ptr[1:] - hop.row_ptr[:-1]).max()) > _RGCN_LONG_ROW
        return self._forward_layer(x, lg, et, act)


FastRGCNConv = RGCNConv


# ---------------------------------------------------------------------------------------------------------------------
# Graph transformer (torch_geometric.nn.TransformerConv; the layer of the reference's cugraph-pyg example mag_lp_mnmg.py)
# — csrc/wg_transformer.hip
# ---------------------------------------------------------------------------------------------------------------------
def transformer_layer_supported(F_src: int, F_dst: int, D: int, H: int, N: int) -> bool:
    """Shapes of the one-kernel transformer layer (``wgamd_transformer_layer_f32``): F_src and F_dst (0: no skip) multiples of 4
    and <= 256, edge_dim D <= 32, heads H <= 8, output width N <= 256, K = H ceil4(F_src + D + 1) + F_dst <= 1024."""
    return bool(L.lib().wgamd_transformer_layer_supported(int(F_src), int(F_dst), int(D), int(H), int(N)))


def transformer_block_width(F_src: int, D: int) -> int:
    """Width of one head's block of the layer's rows A: ``[x_j | a_ij | 1]`` padded to a multiple of 4."""
    return (F_src + D + 1 + 3) // 4 * 4


def transformer_folds(conv):
    """The parameters of ``conv`` (a ``TransformerConv``) in the aggregate-first form, built with torch ops (under autograd when
    it is on), in the parameters' dtype and device:
      ``(Fu [F_dst, H F_src], bu [H F_src], Fw [F_dst, H D] | None, bw [H D] | None, wt [N, K], bias [N] | None)``
    with ``u = x_dst @ Fu + bu`` (u_ih = W_k,h^T q_ih / sqrt(C)), ``w = x_dst @ Fw + bw`` (W_e,h^T q_ih / sqrt(C)) and
    ``wt = Wstack^T``: the columns of head h's block are ``[W_v,h | W_e,h | b_v,h | 0]`` (scaled by 1 / H and summed over the
    heads when ``concat=False``), then ``lin_skip.weight`` (root_weight).  lin_key's bias cancels in the softmax; it enters u
    as an exact 0 so that it still receives a (zero) gradient."""
    H, C = conv.heads, conv.out_channels
    Fs, Fd, D = conv.in_src, conv.in_dst, conv.edge_dim or 0
    sc = 1.0 / math.sqrt(C)
    Wq, bq = conv.lin_query.weight.view(H, C, Fd), conv.lin_query.bias.view(H, C)
    Wk = conv.lin_key.weight.view(H, C, Fs)
    Fu = torch.einsum("hcd,hcf->dhf", Wq, Wk).reshape(Fd, H * Fs) * sc
    bu = torch.einsum("hc,hcf->hf", bq, Wk).reshape(H * Fs) * sc + 0.0 * conv.lin_key.bias.sum()
    Fw = bw = None
    parts = [conv.lin_value.weight.view(H, C, Fs)]
    if D:
        We = conv.lin_edge.weight.view(H, C, D)
        Fw = torch.einsum("hcd,hce->dhe", Wq, We).reshape(Fd, H * D) * sc
        bw = torch.einsum("hc,hce->he", bq, We).reshape(H * D) * sc
        parts.append(We)
    parts.append(conv.lin_value.bias.view(H, C, 1))
    W4 = transformer_block_width(Fs, D)
    if W4 > Fs + D + 1:
        parts.append(Fu.new_zeros((H, C, W4 - Fs - D - 1)))
    blk = torch.cat(parts, 2)                                        # [H, C, W4]
    if conv.concat:
        wt = torch.block_diag(*blk.unbind(0))                        # [H C, H W4]
    else:
        wt = blk.permute(1, 0, 2).reshape(C, H * W4) / H             # [C, H W4]
    bias = None
    if conv.root_weight:
        wt = torch.cat([wt, conv.lin_skip.weight], 1)
        bias = conv.lin_skip.bias
    return Fu, bu, Fw, bw, wt, bias


def transformer_layer_forward(row_ptr, col, x, u, wt, H: int, self_rows=None, x_dst=None, x_dst_ids=False, edge_attr=None, w=None,
                              bias=None, relu=False, src_ids=None, out=None, alpha=None, a_save=None):
    """A whole transformer layer over one hop in ONE kernel (``wgamd_transformer_layer_f32``, include/wgamd_ext.h).  ``u``
    [n, H F_src] and ``w`` [n, H D] are the per-destination vectors (``transformer_folds``), ``wt`` = Wstack^T [N, K];
    ``x_dst`` (None: no skip block) is read at ``self_rows`` (through ``src_ids`` when ``x_dst_ids``)."""
    hop = _hop_args(row_ptr, col, x, src_ids)
    n_rows, F_, N = row_ptr.shape[0] - 1, x.shape[1], wt.shape[0]
    D = 0 if edge_attr is None else edge_attr.shape[1]
    Fd = 0 if x_dst is None else x_dst.shape[1]
    assert wt.dtype == torch.float32 and wt.stride(1) == 1
    assert u.dtype == torch.float32 and u.stride(1) == 1 and u.shape == (n_rows, H * F_)
    assert edge_attr is None or (edge_attr.dtype == torch.float32 and edge_attr.is_contiguous() and edge_attr.shape[0] == col.shape[0])
    assert w is None or (w.dtype == torch.float32 and w.stride(1) == 1 and w.shape == (n_rows, H * D))
    assert x_dst is None or (self_rows is not None and self_rows.dtype == torch.int64 and self_rows.is_contiguous())
    out = _out_rows(out, n_rows, N, row_ptr.device)
    assert alpha is None or (alpha.shape == (col.shape[0], H) and alpha.is_contiguous())
    assert a_save is None or a_save.is_contiguous()
    L.check(L.lib().wgamd_transformer_layer_f32(
        *hop, _ptr(x_dst), 0 if x_dst is None else x_dst.stride(0), Fd, _ptr(self_rows), int(bool(x_dst_ids)),
        None if D == 0 else _nonempty(edge_attr, torch.float32).data_ptr(), D, u.data_ptr(), u.stride(0), _ptr(w),
        0 if w is None else w.stride(0), int(H), wt.data_ptr(), wt.stride(0), N, _ptr(bias), int(bool(relu)), out.data_ptr(),
        out.stride(0), None if alpha is None or alpha.numel() == 0 else alpha.data_ptr(), _ptr(a_save), get_stream()),
        "wgamd_transformer_layer_f32")
    return out


def transformer_bwd_dst(row_ptr, col, x, H: int, alpha, dA, A, du, ds, edge_attr=None, dw=None, src_ids=None):
    """The destination-major backward launch of one hop (``wgamd_transformer_bwd_dst_f32``, include/wgamd_ext.h): from ``dA`` = dZ
    Wstack^T and the kept rows ``A`` (both [n_rows, K]) and ``alpha`` [E, H], writes ``du`` [n_rows, H F_src], ``dw`` [n_rows,
    H D] (with ``edge_attr`` [E, D]) and ``ds`` [E, H]."""
    D = 0 if edge_attr is None else edge_attr.shape[1]
    assert dA.stride(1) == 1 and A.stride(1) == 1 and du.is_contiguous() and (dw is None or dw.is_contiguous())
    L.check(L.lib().wgamd_transformer_bwd_dst_f32(
        *_hop_args(row_ptr, col, x, src_ids), None if D == 0 else _nonempty(edge_attr, torch.float32).data_ptr(), D, int(H),
        _nonempty(alpha, torch.float32).data_ptr(), dA.data_ptr(), dA.stride(0), A.data_ptr(), A.stride(0), du.data_ptr(),
        _ptr(dw), _nonempty(ds, torch.float32).data_ptr(), get_stream()), "wgamd_transformer_bwd_dst_f32")


def transformer_bwd_src(row_ptr_t, col_t, perm, self_t, D: int, H: int, skip_at: int, alpha, ds, dA, u, gx):
    """The source-major backward launch of one hop over its transpose (``wgamd_transformer_bwd_src_f32``, include/wgamd_ext.h):
    ``gx`` [n_src, F_src] += the hop's part of the input gradient, from the hop's rows of ``dA`` and ``u``; ``row_ptr_t, col_t,
    self_t, perm`` as ``HopGraph.transposed`` gives them (``self_t`` None or ``skip_at`` < 0: no skip term)."""
    assert dA.stride(1) == 1 and u.stride(1) == 1 and gx.stride(1) == 1 and u.shape[0] == dA.shape[0]
    L.check(L.lib().wgamd_transformer_bwd_src_f32(
        row_ptr_t.data_ptr(), _nonempty(col_t, torch.int32).data_ptr(), perm.data_ptr(), _ptr(self_t), dA.shape[0], gx.shape[0],
        gx.shape[1], D, H, skip_at, _nonempty(alpha, torch.float32).data_ptr(), _nonempty(ds, torch.float32).data_ptr(), dA.data_ptr(),
        dA.stride(0), u.data_ptr(), u.stride(0), gx.data_ptr(), gx.stride(0), 1, get_stream()), "wgamd_transformer_bwd_src_f32")


def _tconv_rows(t):
    """``t`` as the kernels read it: float32, and a contiguous copy when its rows are strided or not 16-B aligned (a fresh
    allocation is; F is a multiple of 4 in the kernel's domain).  Under autograd: the gradient reaches ``t``."""
    t = t.float()
    if not _kernel_rows_ok(t):
        t = t.contiguous() if not t.is_contiguous() else t.clone()
    return t


class _TconvLayer(torch.autograd.Function):
    """The one-kernel transformer layer over a ``LayerGraph`` (one ``wgamd_transformer_layer_f32`` launch per hop), from the
    aggregate-first folds ``u``, ``w`` and ``wt`` (built from the parameters under autograd by the caller: their gradients
    reach the parameters through autograd over small tensors).  When training the forward keeps alpha [E, H] and the rows A
    [n, K] — A is both the weight gradient's operand (dWstack = A^T dZ, a library GEMM) and what gives the softmax backward its
    row sums (dA_ih . A_ih), so keeping it costs one [n, K] write and saves rebuilding it.  Backward: dA = dZ Wstack^T (library
    GEMM), then ``wgamd_transformer_bwd_dst_f32`` per hop (du, dw, ds) and, for x, ``wgamd_transformer_bwd_src_f32`` over each
    hop's transpose (no atomics).  The edge-attribute gradient, when asked for, is library ops."""

    @staticmethod
    def forward(ctx, x, x_dst, u, w, edge_attr, wt, bias, graph, ids, relu, H, skip, n_src, want_alpha):
        lg, dev = graph, wt.device
        n, N, F_ = lg.n_rows, wt.shape[0], x.shape[1]
        D = 0 if edge_attr is None else edge_attr.shape[1]
        train = any(ctx.needs_input_grad[:7])
        E = sum(int(h.col.shape[0]) for h in lg.hops)
        out = torch.empty((n, N), dtype=torch.float32, device=dev)
        alpha = torch.empty((E, H), dtype=torch.float32, device=dev) if (train or want_alpha) else None
        A = torch.empty((n, wt.shape[1]), dtype=torch.float32, device=dev) if train else None
        wt_d, b_d = wt.detach().contiguous(), None if bias is None else bias.detach()
        u_d, w_d = u.detach().contiguous(), None if w is None else w.detach().contiguous()
        xd = x_dst if x_dst is not None else x
        for h, rows, edges in _hops(lg):
            if h.n_rows > 0:
                transformer_layer_forward(
                    h.row_ptr, h.col, x, u_d[rows], wt_d, H, self_rows=h.self_rows, x_dst=xd if skip else None,
                    x_dst_ids=ids is not None and x_dst is None, edge_attr=None if D == 0 else edge_attr[edges],
                    w=None if w_d is None else w_d[rows], bias=b_d, relu=relu, src_ids=ids, out=out[rows],
                    alpha=None if alpha is None else alpha[edges], a_save=None if A is None else A[rows])
        ctx.set_materialize_grads(False)
        if train:
            ctx.save_for_backward(u_d, w_d, wt_d, out, alpha, A)
            ctx.x, ctx.edge_attr, ctx.graph, ctx.ids, ctx.relu, ctx.H, ctx.skip, ctx.n_src = x, edge_attr, lg, ids, relu, H, skip, n_src
            ctx.bipartite = x_dst is not None
        if want_alpha:
            ctx.mark_non_differentiable(alpha)
            return out, alpha
        return out

    @staticmethod
    def backward(ctx, g, *unused):
        _released(ctx.x, "TransformerConv", "input rows")
        u, w, wt, out, alpha, A = ctx.saved_tensors
        need_x, need_xd, need_u, need_w, need_ea, need_wt, need_b = ctx.needs_input_grad[:7]
        x, ea, lg, H = ctx.x, ctx.edge_attr, ctx.graph, ctx.H
        dev, F_ = wt.device, x.shape[1]
        D = 0 if ea is None else ea.shape[1]
        W4 = transformer_block_width(F_, D)
        n = lg.n_rows
        gx = gxd = gu = gw = gea = gwt = gb = None
        if g is None:
            g = torch.zeros_like(out)
        gz = g.contiguous().float()
        if ctx.relu:
            gz = torch.ops.aten.threshold_backward(gz, out, 0)
        if need_wt:
            gwt = gz.t() @ A
        if need_b:
            gb = gz.sum(0)
        if need_x or need_xd or need_u or need_w or need_ea:
            dA = (gz @ wt).contiguous()                                          # [n, K]
            E = alpha.shape[0]
            du = torch.empty((n, H * F_), dtype=torch.float32, device=dev)
            dw = torch.empty((n, H * D), dtype=torch.float32, device=dev) if D else None
            ds = torch.empty((E, H), dtype=torch.float32, device=dev)
            for h, rows, edges in _hops(lg):
                if h.n_rows > 0:
                    transformer_bwd_dst(h.row_ptr, h.col, x, H, alpha[edges], dA[rows], A[rows], du[rows], ds[edges],
                                        edge_attr=None if D == 0 else ea[edges], dw=None if dw is None else dw[rows], src_ids=ctx.ids)
            gu, gw = du, dw
            if need_x:
                gx = torch.zeros((ctx.n_src, F_), dtype=torch.float32, device=dev)
                # the skip block reaches x only when the destinations are rows of x itself (not an (x_src, x_dst) pair,
                # whose self_rows index x_dst)
                own_skip = ctx.skip and not ctx.bipartite
                skip_at = H * W4 if own_skip else -1
                for h, rows, edges in _hops(lg):
                    if h.n_rows > 0:
                        row_ptr_t, col_t, self_t, perm = h.transposed(ctx.n_src, need_self=own_skip, need_perm=True)
                        transformer_bwd_src(row_ptr_t, col_t, perm, self_t, D, H, skip_at, alpha[edges], ds[edges], dA[rows], u[rows], gx)
            if need_xd and ctx.skip:
                gxd = dA[:, H * W4:].contiguous()
            if need_ea and D:
                gea = torch.zeros_like(ea)
                dA3 = dA[:, :H * W4].view(n, H, W4)
                w3 = w.view(n, H, D)
                for h, rows, edges in _hops(lg):
                    if edges.stop > edges.start:
                        dst = _edge_dst(h.row_ptr, edges.stop - edges.start, rows.start)
                        a_e, s_e = alpha[edges].unsqueeze(2), ds[edges].unsqueeze(2)
                        gea[edges] = (a_e * dA3[dst, :, F_:F_ + D] + s_e * w3[dst]).sum(1)
        ctx.x = ctx.edge_attr = None
        return gx, gxd, gu, gw, gea, gwt, gb, None, None, None, None, None, None, None


def _tconv_library_ops(conv, x_src, x_dst_rows, lg: LayerGraph, edge_attr, relu: bool):
    """The layer in PyG's own formulation, composed of library ops under autograd: the route of shapes outside the one-kernel
    layer's domain (correctness, not speed).  Returns ``(out, alpha)`` with alpha [E, H] hop-major in CSR order."""
    H, C = conv.heads, conv.out_channels
    outs, alphas = [], []
    for h, rows, edges in _hops(lg):
        nh, Eh = h.n_rows, int(h.col.shape[0])
        xd = x_dst_rows[rows]
        dst = _edge_dst(h.row_ptr, Eh)
        xs = x_src[h.col.long()]
        q = conv.lin_query(xd).view(nh, H, C)
        k = conv.lin_key(xs).view(Eh, H, C)
        v = conv.lin_value(xs).view(Eh, H, C)
        if conv.lin_edge is not None:
            e = conv.lin_edge(edge_attr[edges]).view(Eh, H, C)
            k, v = k + e, v + e
        s = (q[dst] * k).sum(-1) / math.sqrt(C)                                   # [E, H]
        smax = s.new_full((nh, H), -math.inf).scatter_reduce(0, dst.unsqueeze(1).expand(Eh, H), s, "amax", include_self=True)
        ex = (s - smax[dst]).exp()
        den = s.new_zeros((nh, H)).index_add(0, dst, ex) + 1e-16
        alpha = ex / den[dst]
        o = s.new_zeros((nh, H, C)).index_add(0, dst, alpha.unsqueeze(2) * v)
        o = o.reshape(nh, H * C) if conv.concat else o.mean(1)
        if conv.root_weight:
            o = o + conv.lin_skip(xd)
        outs.append(o)
        alphas.append(alpha)
    out = torch.cat(outs) if outs else x_src.new_zeros((0, H * C if conv.concat else C))
    alpha = torch.cat(alphas) if alphas else x_src.new_zeros((0, H))
    return (torch.relu(out) if relu else out), alpha


class TransformerConv(torch.nn.Module):
    """PyG ``TransformerConv`` (flow source_to_target):
        alpha_ij = softmax_j( q_i . (k_j + e_ij) / sqrt(C) ),   out_i = sum_j alpha_ij (v_j + e_ij)  [+ lin_skip(x_i)]
    with ``q = lin_query(x_dst)``, ``k = lin_key(x_src)``, ``v = lin_value(x_src)``, ``e = lin_edge(edge_attr)`` (``edge_dim``),
    per head; ``concat=True`` concatenates the heads ([N, H C]), ``concat=False`` averages them ([N, C]).  A destination with no
    edges gets no message (no value bias), only the skip term.  Parameters as PyG names them (``lin_key``, ``lin_query``,
    ``lin_value``, ``lin_skip``: ``weight`` [out, in] and ``bias``; ``lin_edge.weight``), initialised as ``torch.nn.Linear``
    does, so a PyG ``state_dict`` loads.  ``lin_skip`` exists whatever ``root_weight`` says (as in PyG); ``bias`` is its bias.

    ``forward(x, graph, edge_attr=None, act=None, return_attention_weights=False)``: ``graph`` = a COO ``edge_index`` (the ``for
    batch in loader`` loop of mag_lp_mnmg.py with ``attr[batch.e_id]``; x a tensor or an ``(x_src, x_dst)`` pair, output rows
    = the destination rows), a ``[csr_row_ptr, csr_col_ind]`` pair with ``edge_attr`` in CSR order (destinations = the first
    rows of x, or x_dst), or a call group's ``LayerGraph`` with x a tensor or ``LazyRows`` and ``edge_attr`` hop-major in
    ``CallGroup.e_id`` order (``CallGroup.edge_attr``; every layer takes the same tensor and reads the prefix of its hops).
    ``edge_attr`` is [E, edge_dim] (or [E] when edge_dim is 1), floating, on the graph's device; a wrong length, width, dtype or
    device, or none when ``edge_dim`` is set, raises ValueError (without ``edge_dim`` it is ignored, as in PyG).

    The layer is computed aggregate-first: the logit is linear in x_j, so each destination keeps ``u = W_k^T q / sqrt(C)`` and
    ``w = W_e^T q / sqrt(C)`` (one library GEMM over the destination rows) and ONE kernel per hop (``wgamd_transformer_layer_f32``)
    walks the edges with an online softmax, builds ``[sum alpha [x_j | a_ij | 1] per head | x_dst]`` and multiplies it by the
    stacked value / edge / skip weight on the fp32 matrix pipe, bias and ``act="relu"`` fused.  The backward is two more kernels
    and library GEMMs, without atomics (the same bits from run to run).  Inputs of another floating dtype, or with strided or
    misaligned rows, are first copied to float32 rows (a lazy table of that kind is gathered).  Shapes outside the kernel's
    domain (``transformer_layer_supported``: in_channels multiples of 4 and <= 256, edge_dim <= 32, heads <= 8, output width
    <= 256, K <= 1024), and inputs on the CPU, run the WHOLE layer as library ops in PyG's formulation — correct, not fast.
    Other keyword arguments of PyG's are refused (TypeError) except its defaults ``aggr="add"`` and ``node_dim=0``.
    ``return_attention_weights=True`` also returns alpha [E, H] (not differentiable): ``(out, (edge_index, alpha))`` in the
    edge_index's order for a COO graph, ``(out, alpha)`` in CSR / hop-major order otherwise.

    Not supported: ``beta=True`` (NotImplementedError at construction) and attention dropout (``dropout > 0`` raises
    NotImplementedError in training mode; in eval mode dropout is the identity, as in PyG)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1, concat: bool = True,
                 beta: bool = False, dropout: float = 0.0, edge_dim: Optional[int] = None, bias: bool = True,
                 root_weight: bool = True, **kwargs):
        super().__init__()
        for k, v in kwargs.items():
            if not ((k == "aggr" and v == "add") or (k == "node_dim" and v == 0)):
                raise TypeError("TransformerConv: unsupported argument %s=%r (of PyG's MessagePassing arguments only the defaults "
                                "aggr='add' and node_dim=0 are accepted)" % (k, v))
        if beta:
            raise NotImplementedError("TransformerConv: beta=True (the gated skip connection) is not supported")
        if heads < 1 or out_channels < 1:
            raise ValueError("TransformerConv: heads and out_channels must be positive")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.in_src, self.in_dst = int(in_channels[0]), int(in_channels[1])
        self.beta, self.dropout, self.edge_dim, self.root_weight = beta, float(dropout), edge_dim, root_weight
        HC = heads * out_channels
        self.lin_key = torch.nn.Linear(self.in_src, HC)
        self.lin_query = torch.nn.Linear(self.in_dst, HC)
        self.lin_value = torch.nn.Linear(self.in_src, HC)
        self.lin_edge = torch.nn.Linear(edge_dim, HC, bias=False) if edge_dim is not None else None
        self.lin_skip = torch.nn.Linear(self.in_dst, HC if concat else out_channels, bias=bias)
        self._wgamd_derived = {}       # (``_derived``'s store, here from the start: a forward adds no attribute to the module)

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge, self.lin_skip):
            if lin is not None:
                lin.reset_parameters()

    @property
    def _out_width(self) -> int:
        return self.heads * self.out_channels if self.concat else self.out_channels

    def _folds(self):
        """``transformer_folds`` in float32: under autograd when a parameter needs a gradient, else cached against the
        parameters (``_derived``), contiguous."""
        params = list(self.parameters())
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _derived(self, "folds", params, grad=grad, build=lambda: [
            None if t is None else (t.float() if grad else t.float().contiguous()) for t in transformer_folds(self)])

    def _check_edge_attr(self, edge_attr, n_edges: int, device):
        """The edge attribute as the kernels read it (float32 [E, D] contiguous), or None without edge_dim; ValueError on a
        missing one or a wrong length, width, dtype or device — before any launch."""
        if self.edge_dim is None:
            return None
        D = self.edge_dim
        if edge_attr is None:
            raise ValueError("TransformerConv: edge_dim=%d needs edge_attr" % D)
        if not torch.is_tensor(edge_attr) or not edge_attr.is_floating_point():
            raise ValueError("TransformerConv: edge_attr must be a floating-point tensor")
        if edge_attr.dim() == 1 and D == 1:
            edge_attr = edge_attr.unsqueeze(1)
        if edge_attr.dim() != 2 or edge_attr.shape[1] != D:
            raise ValueError("TransformerConv: edge_attr has shape %s, the layer takes [E, %d]" % (tuple(edge_attr.shape), D))
        if edge_attr.device != torch.device(device):
            raise ValueError("TransformerConv: edge_attr is on %s, the graph on %s" % (edge_attr.device, torch.device(device)))
        if edge_attr.shape[0] != n_edges:
            raise ValueError("TransformerConv: edge_attr has %d rows for %d edges" % (edge_attr.shape[0], n_edges))
        return edge_attr

    def _forward_layer(self, x, lg: LayerGraph, edge_attr, act, x_dst=None, want_alpha=False):
        """``x`` (tensor or LazyRows) over a layer graph; ``x_dst`` (bipartite, one hop with self_rows = arange): the destination
        rows.  Returns ``(out, alpha or None)`` with alpha hop-major in CSR order."""
        assert act in (None, "relu"), "act: None or 'relu'"
        relu = act == "relu"
        H, N, D = self.heads, self._out_width, self.edge_dim or 0
        src, ids, n_src, n_edges = _layer_input(self, x, lg, self.in_src)
        lazy = ids is not None
        if x_dst is not None and x_dst.shape[1] != self.in_dst:
            raise ValueError("TransformerConv: x_dst has %d features, the layer takes %d" % (x_dst.shape[1], self.in_dst))
        if x_dst is None and self.in_src != self.in_dst:
            raise ValueError("TransformerConv: in_channels = %s needs an (x_src, x_dst) pair" % (self.in_channels,))
        dev = lg.hops[0].row_ptr.device if lg.hops else src.device
        ea = self._check_edge_attr(edge_attr, n_edges, dev)
        skip = self.root_weight
        kernel = transformer_layer_supported(self.in_src, self.in_dst if skip else 0, D, H, N) and src.is_cuda and (
            x_dst is None or x_dst.is_cuda)
        if kernel:
            # rows as the kernel reads them (float32, unit column stride, 16-B aligned rows): copied (under autograd) when they
            # are not; a lazy table that is not is gathered
            if lazy and not _kernel_rows_ok(src):
                x, lazy = x.materialize(), False
            if not lazy:
                x = src = _tconv_rows(x)
            if x_dst is not None:
                x_dst = _tconv_rows(x_dst)
        self_all = torch.cat([h.self_rows for h in lg.hops]) if lg.hops else torch.zeros(0, dtype=torch.int64, device=dev)
        # the destination rows as a tensor: the query's input (and the skip's, on the library route)
        if x_dst is not None:
            xd_rows = x_dst
        elif lazy:
            xd_rows = src[x.ids[self_all].long()] if not getattr(src, "byte_offset_ids", False) else x.materialize()[self_all]
        else:
            xd_rows = x[self_all]
        if kernel:
            Fu, bu, Fw, bw, wt, bias = self._folds()
            xq = xd_rows.float()
            u = torch.addmm(bu, xq, Fu)
            w = torch.addmm(bw, xq, Fw) if D else None
            eak = None if ea is None else ea.float().contiguous()
            res = _TconvLayer.apply(src, x_dst, u, w, eak, wt, bias, lg, x.ids if lazy else None, relu, H, skip, n_src,
                                    want_alpha)
            return res if want_alpha else (res, None)
        xs = x.materialize() if lazy else x
        out, alpha = _tconv_library_ops(self, xs.float(), xd_rows.float(), lg, None if ea is None else ea.float(), relu)
        return out, (alpha.detach() if want_alpha else None)

    def forward(self, x, graph, edge_attr=None, act=None, return_attention_weights=False):
        if self.dropout > 0 and self.training:
            raise NotImplementedError("TransformerConv: attention dropout (dropout > 0 in training mode) is not supported")
        _refuse_capture(self, "per-graph caches")
        if isinstance(graph, HeteroLayerGraph):
            raise NotImplementedError("TransformerConv over a heterogeneous call group's layer graph is not supported "
                                      "(wrap the relations in HeteroConv({edge_type: TransformerConv}))")
        x_dst = None
        if isinstance(x, (tuple, list)):
            x, x_dst = x
        _refuse_featureless(self, x)
        if x_dst is not None:
            _refuse_featureless(self, x_dst)
        if isinstance(graph, LayerGraph):
            if x_dst is not None:
                raise NotImplementedError("TransformerConv: an (x_src, x_dst) pair over a LayerGraph is not supported")
            out, alpha = self._forward_layer(x, graph, edge_attr, act, want_alpha=return_attention_weights)
            return (out, alpha) if return_attention_weights else out
        if isinstance(x, LazyRows):
            x = x.materialize()
        if isinstance(x_dst, LazyRows):
            x_dst = x_dst.materialize()
        # (graph[1]: the CSR pair's col, or the COO list's destinations — one entry per edge either way)
        ea = self._check_edge_attr(edge_attr, graph[1].shape[0], graph[0].device)
        lg, order, ea = _single_hop(graph, x.shape[0] if x_dst is None else x_dst.shape[0], ea)
        n_dst = lg.n_rows
        if x_dst is not None and x_dst.shape[0] < n_dst:
            raise ValueError("TransformerConv: x_dst has %d rows for %d destinations" % (x_dst.shape[0], n_dst))
        if x_dst is None and x.shape[0] < n_dst:
            raise ValueError("TransformerConv: x has %d rows for %d destinations" % (x.shape[0], n_dst))
        if x_dst is not None:
            x_dst = x_dst[:n_dst]
        out, alpha = self._forward_layer(x, lg, ea, act, x_dst=x_dst, want_alpha=return_attention_weights)
        if not return_attention_weights:
            return out
        if isinstance(graph, (tuple, list)):
            return out, alpha
        if order is not None:                          # alpha back in edge_index order
            a = torch.empty_like(alpha)
            a[order] = alpha
            alpha = a
        return out, (graph, alpha)


# ---------------------------------------------------------------------------------------------------------------------
# GIN (torch_geometric.nn.GINConv with the GIN paper's MLP, and global_add_pool; the model of the reference's cugraph-pyg
# example dist_gin_sg.py) — csrc/wg_gin.hip
# ---------------------------------------------------------------------------------------------------------------------
GIN_RELU_HIDDEN, GIN_RELU_OUT = 1, 2     # WGAMD_GIN_* (include/wgamd_ext.h)


def gin_layer_supported(F_: int, H: int, N: int = 0) -> bool:
    """Shapes of the one-kernel GIN layer (``wgamd_gin_layer_f32``): F % 4 == 0; F, H, N <= 256; H % 4 == 0 with a second
    product (N > 0; N = 0: the layer ends after the first product)."""
    return bool(L.lib().wgamd_gin_layer_supported(int(F_), int(H), int(N)))


def _gin_hop_args(row_ptr, x, self_rows, x_dst, eps):
    """GIN's four arguments behind ``_hop_args``: ``self_rows, x_dst, ldx_dst, eps`` (the self row of destination i is ``x_dst[i]``
    when ``x_dst`` is given, else row ``self_rows[i]`` of x)."""
    F_ = x.shape[1]
    assert self_rows is None or (self_rows.dtype == torch.int64 and self_rows.is_contiguous())
    assert x_dst is None or (x_dst.dtype == torch.float32 and x_dst.stride(1) == 1 and x_dst.shape[1] == F_
                             and x_dst.shape[0] >= row_ptr.shape[0] - 1)
    assert eps is None or (eps.dtype == torch.float32 and eps.is_cuda and eps.numel() == 1)
    return (None if x_dst is not None else _ptr(self_rows), _ptr(x_dst), 0 if x_dst is None else x_dst.stride(0), _ptr(eps))


def gin_layer_forward(row_ptr, col, x, self_rows, w1, b1=None, w2=None, b2=None, eps=None, relu_hidden=True, relu_out=False,
                      src_ids=None, x_dst=None, out=None, keep=False, agg_out=None, hidden_out=None):
    """A whole GIN layer over one hop in ONE kernel (``wgamd_gin_layer_f32``, include/wgamd_ext.h):
    ``act2(act1(agg @ w1^T + b1) @ w2^T + b2)`` with ``agg = sum of the neighbour rows + (1 + eps) self row``; ``w1`` [H, F] and
    ``w2`` [N, H] in ``torch.nn.Linear`` layout, ``eps`` a one-element float32 device tensor (None: 0).  ``w2 = None``: the layer
    ends after the first product (output [n_rows, H]).  The self row of destination i is ``x_dst[i]`` when ``x_dst`` is given,
    else row ``self_rows[i]`` of x; neither: no self term.  ``keep`` (or ``agg_out`` / ``hidden_out`` buffers): the launch also
    stores the aggregate and, with a second product, the hidden activation (``_train``), and ``(out, agg, hidden)`` is returned."""
    hop = _hop_args(row_ptr, col, x, src_ids) + _gin_hop_args(row_ptr, x, self_rows, x_dst, eps)
    n_rows, F_, H = row_ptr.shape[0] - 1, x.shape[1], w1.shape[0]
    N = 0 if w2 is None else w2.shape[0]
    for w, k in ((w1, F_), (w2, H)):
        assert w is None or (w.dtype == torch.float32 and w.stride(1) == 1 and w.shape[1] == k)
    dev = row_ptr.device
    out = _out_rows(out, n_rows, N or H, dev)
    flags = (GIN_RELU_HIDDEN if relu_hidden else 0) | (GIN_RELU_OUT if relu_out else 0)
    common = hop + (w1.data_ptr(), w1.stride(0), H, _ptr(b1), _ptr(w2), 0 if w2 is None else w2.stride(0), N, _ptr(b2), flags,
                    out.data_ptr(), out.stride(0))
    if not (keep or agg_out is not None or hidden_out is not None):
        L.check(L.lib().wgamd_gin_layer_f32(*common, get_stream()), "wgamd_gin_layer_f32")
        return out
    if keep and agg_out is None:
        agg_out = torch.empty((n_rows, F_), dtype=torch.float32, device=dev)
    if keep and hidden_out is None and w2 is not None:
        hidden_out = torch.empty((n_rows, H), dtype=torch.float32, device=dev)
    assert agg_out is None or (agg_out.shape == (n_rows, F_) and agg_out.stride(1) == 1)
    assert hidden_out is None or (w2 is not None and hidden_out.shape == (n_rows, H) and hidden_out.stride(1) == 1)
    L.check(L.lib().wgamd_gin_layer_f32_train(*common, _ptr(agg_out), 0 if agg_out is None else agg_out.stride(0), _ptr(hidden_out),
                                              0 if hidden_out is None else hidden_out.stride(0), get_stream()),
            "wgamd_gin_layer_f32_train")
    return out, agg_out, hidden_out


def gin_aggregate(row_ptr, col, x, self_rows, eps=None, src_ids=None, x_dst=None, out=None):
    """The GIN aggregate alone, any F (``wgamd_gin_aggregate_f32``): the sum of the neighbour rows plus ``(1 + eps)`` times the
    self row (``gin_layer_forward``'s)."""
    hop = _hop_args(row_ptr, col, x, src_ids) + _gin_hop_args(row_ptr, x, self_rows, x_dst, eps)
    out = _out_rows(out, row_ptr.shape[0] - 1, x.shape[1], row_ptr.device)
    L.check(L.lib().wgamd_gin_aggregate_f32(*hop, out.data_ptr(), out.stride(0), get_stream()), "wgamd_gin_aggregate_f32")
    return out


def _gin_self_rows(src, ids, x_dst, graph: LayerGraph):
    """The self rows of a GIN layer's destinations as a tensor [n_rows, F] (the operand of d eps)."""
    if x_dst is not None:
        return x_dst[:graph.n_rows]
    self_all = torch.cat([h.self_rows for h in graph.hops])
    if ids is None:
        return src[self_all]
    if getattr(src, "byte_offset_ids", False):
        raise NotImplementedError("GINConv(train_eps=True) over a peer-mapped feature table: pass the gathered rows")
    return src[ids[self_all].long()]


def _gin_hop_self(h: HopGraph, rows, x_dst, no_root: bool):
    """``(self_rows, x_dst rows)`` of one hop as the kernels take them."""
    if no_root:
        return None, None
    return (None, x_dst[rows]) if x_dst is not None else (h.self_rows, None)


def _gin_input_grad(graph: LayerGraph, g, n_src: int, eps, has_self: bool, weight=None):
    """``A^T g + (1 + eps) S^T g`` over every hop of ``graph`` (rows = the layer's input rows; the second term only where an
    input row is a destination itself, and only with ``has_self``), times ``weight`` ([F, Hq]) when given: the GIN kernels run
    over the hops' transposes."""
    def per_hop(h, rows, _, k):
        row_ptr_t, col_t, _ = h.transposed(n_src, need_self=False)
        self_t = h.input_dst(n_src) if has_self else None
        if weight is None:
            return gin_aggregate(row_ptr_t, col_t, g[rows], self_t, eps=eps)
        return gin_layer_forward(row_ptr_t, col_t, g[rows], self_t, weight, eps=eps, relu_hidden=False)
    return _sum_over_hops(graph, (n_src, g.shape[1] if weight is None else weight.shape[0]), g.device, per_hop)


class _GinLayer(torch.autograd.Function):
    """The one-kernel GIN layer over a ``LayerGraph`` (one ``wgamd_gin_layer_f32`` launch per hop; under autograd the ``_train``
    form keeps the aggregate and the hidden activation).  Backward, no atomics: ``wgamd_gcn_wgrad_f32`` per hop and product
    (dW2, db2 from the hidden activation; dW1, db1 from the aggregate), one library GEMM between them (dHidden = dOut W2), and
    for the input rows the GIN kernel over every hop's transpose with ``W1^T`` as its only weight."""

    @staticmethod
    def forward(ctx, src, x_dst, eps, w1, b1, w2, b2, graph, ids, relu_hidden, relu_out, n_src, no_root):
        H, F_ = w1.shape
        two = w2 is not None
        keep = any(ctx.needs_input_grad[:7])
        dev = w1.device
        n = graph.n_rows
        out = torch.empty((n, w2.shape[0] if two else H), dtype=torch.float32, device=dev)
        agg = torch.empty((n, F_), dtype=torch.float32, device=dev) if keep else None
        hidden = torch.empty((n, H), dtype=torch.float32, device=dev) if keep and two else None
        det = lambda t: None if t is None else t.detach()      # noqa: E731
        for h, rows, _ in _hops(graph):
            if h.n_rows > 0:
                self_rows, xd = _gin_hop_self(h, rows, det(x_dst), no_root)
                gin_layer_forward(h.row_ptr, h.col, src, self_rows, det(w1), det(b1), det(w2), det(b2), eps=det(eps),
                                  relu_hidden=relu_hidden, relu_out=relu_out, src_ids=ids, x_dst=xd, out=out[rows],
                                  agg_out=None if agg is None else agg[rows], hidden_out=None if hidden is None else hidden[rows])
        if keep:
            ctx.save_for_backward(w1, w2, eps, out, x_dst)
            ctx.kept = (agg, hidden)
            ctx.src = src if ctx.needs_input_grad[2] else None      # (d eps reads the self rows; a mapped table is no tensor)
            ctx.graph, ctx.ids, ctx.flags, ctx.n_src, ctx.no_root = graph, ids, (relu_hidden, relu_out), n_src, no_root
        return out

    @staticmethod
    def backward(ctx, g):
        _released(ctx.kept, "GINConv", "activations")
        w1, w2, eps, out, x_dst = ctx.saved_tensors
        agg, hidden = ctx.kept
        src = ctx.src
        relu_hidden, relu_out = ctx.flags
        need_x, need_xd, need_eps, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:7]
        H, F_ = w1.shape
        dev = g.device
        graph = ctx.graph
        g = g.contiguous().float()
        gw1 = gb1 = gw2 = gb2 = None
        some = any(h.n_rows > 0 for h in graph.hops)
        if w2 is not None:
            if relu_out:
                g = torch.ops.aten.threshold_backward(g, out, 0)
            if need_w2 or need_b2:      # (a bias gradient alone: the product's launches all the same, dW dropped)
                gw2, gb2 = _dense_wgrad(graph, hidden, g, w2, need_b2, None)
                gw2 = gw2 if need_w2 else None
            g1, act1 = g @ w2.detach(), hidden if relu_hidden else None          # dHidden: one library GEMM
        else:
            g1, act1 = g, out if relu_hidden else None
        lower = need_x or need_xd or need_eps
        if act1 is not None and lower:
            g1, act1 = torch.ops.aten.threshold_backward(g1, act1, 0), None      # dZ1 once, read by every gradient below
        if need_w1 or need_b1:
            gw1, gb1 = _dense_wgrad(graph, agg, g1, w1, need_b1, act1)
            gw1 = gw1 if need_w1 else None
        gx = gxd = geps = None
        has_self = not ctx.no_root and x_dst is None
        if need_x:
            Hq = (H + 3) // 4 * 4
            gx = _gin_input_grad(graph, _pad_cols(g1, Hq), ctx.n_src, eps.detach(), has_self, weight=_padded_wt(w1, Hq))
        if (need_xd or need_eps) and not ctx.no_root:
            d_agg = g1 @ w1.detach() if some else torch.zeros((0, F_), dtype=torch.float32, device=dev)
            if need_xd:
                gxd = torch.zeros_like(x_dst, dtype=torch.float32)
                gxd[:d_agg.shape[0]] = (1.0 + eps.detach()) * d_agg
            if need_eps:
                geps = (d_agg * _gin_self_rows(src, ctx.ids, x_dst, graph)).sum().reshape(eps.shape)
        elif need_eps:
            geps = torch.zeros_like(eps)
        ctx.kept = None
        return gx, gxd, geps, gw1, gb1, gw2, gb2, None, None, None, None, None, None


class _GinAggregate(torch.autograd.Function):
    """The GIN aggregate over every hop of a ``LayerGraph`` (``wgamd_gin_aggregate_f32``), rows back to back; backward = the same
    kernel over the hops' transposes.  The route of shapes and ``nn`` modules the one-kernel layer does not take."""

    @staticmethod
    def forward(ctx, x, x_dst, eps, graph, no_root):
        out = torch.empty((graph.n_rows, x.shape[1]), dtype=torch.float32, device=x.device)
        for h, rows, _ in _hops(graph):
            if h.n_rows > 0:
                self_rows, xd = _gin_hop_self(h, rows, x_dst, no_root)
                gin_aggregate(h.row_ptr, h.col, x, self_rows, eps=eps, x_dst=xd, out=out[rows])
        ctx.save_for_backward(x, x_dst, eps)
        ctx.graph, ctx.no_root = graph, no_root
        return out

    @staticmethod
    def backward(ctx, g):
        x, x_dst, eps = ctx.saved_tensors
        need_x, need_xd, need_eps = ctx.needs_input_grad[:3]
        g = g.contiguous()
        gx = gxd = geps = None
        if need_x:
            gx = _gin_input_grad(ctx.graph, g, x.shape[0], eps, not ctx.no_root and x_dst is None)
        if need_xd:
            gxd = torch.zeros_like(x_dst)
            gxd[:g.shape[0]] = (1.0 + eps) * g
        if need_eps:
            geps = torch.zeros_like(eps) if ctx.no_root else (g * _gin_self_rows(x, None, x_dst, ctx.graph)).sum().reshape(eps.shape)
        return gx, gxd, geps, None, None


def _gin_aggregate_torch(x, x_dst, eps, lg: LayerGraph, no_root: bool):
    """PyG's formulation of the GIN aggregate in torch ops (CPU tensors)."""
    aggs = []
    for h, rows, _ in _hops(lg):
        n, E = h.n_rows, int(h.col.shape[0])
        agg = torch.zeros((n, x.shape[1]), dtype=x.dtype, device=x.device)
        if E > 0:
            agg = agg.index_add_(0, _edge_dst(h.row_ptr, E), x[h.col.long()])
        if not no_root:
            agg = agg + (1.0 + eps.to(x.dtype)) * (x_dst[rows] if x_dst is not None else x[h.self_rows])
        aggs.append(agg)
    if not aggs:
        return torch.zeros((0, x.shape[1]), dtype=x.dtype, device=x.device)
    return aggs[0] if len(aggs) == 1 else torch.cat(aggs)


class _MLPBatchNorm(torch.nn.Module):
    """PyG's ``BatchNorm`` wrapper as ``MLP`` holds it: the ``torch.nn.BatchNorm1d`` lives under ``module``."""

    def __init__(self, channels: int, eps: float = 1e-5, momentum=0.1):
        super().__init__()
        self.module = torch.nn.BatchNorm1d(channels, eps=eps, momentum=momentum)

    def reset_parameters(self):
        self.module.reset_parameters()

    def forward(self, x):
        return self.module(x)


class MLP(torch.nn.Module):
    """PyG ``MLP(channel_list)`` by name and state dict: ``torch.nn.Linear`` layers under ``lins`` and, with
    ``norm="batch_norm"``, ``torch.nn.BatchNorm1d`` under ``norms[i].module`` (keys ``lins.{i}.weight/bias``,
    ``norms.{i}.module.weight/bias/running_mean/running_var/num_batches_tracked``), so a PyG state dict of ``MLP([...])`` loads
    with ``strict=True``.  ``forward`` is PyG's order in torch ops — per layer ``lin -> [act if act_first] -> norm -> [act] ->
    dropout``, the last layer plain with ``plain_last`` — on any device.  ``norm``: ``"batch_norm"`` or None (``norm_kwargs``:
    ``eps``, ``momentum``); ``act``: ``"relu"`` or None.  Inside ``GINConv`` a three-channel ``MLP`` runs on the layer kernels
    (routes ``"mlp_bn"`` and ``"mlp"``)."""

    def __init__(self, channel_list, dropout: float = 0.0, act="relu", act_first: bool = False, norm="batch_norm",
                 norm_kwargs=None, plain_last: bool = True, bias: bool = True):
        super().__init__()
        if not isinstance(channel_list, (tuple, list)) or len(channel_list) < 2 or not all(
                isinstance(c, int) and c > 0 for c in channel_list):
            raise ValueError("MLP: channel_list must hold at least two positive ints, got %r" % (channel_list,))
        if norm not in ("batch_norm", None):
            raise ValueError("MLP: norm=%r is not supported ('batch_norm' or None)" % (norm,))
        if act not in ("relu", None):
            raise ValueError("MLP: act=%r is not supported ('relu' or None)" % (act,))
        norm_kwargs = dict(norm_kwargs or {})
        unknown = sorted(set(norm_kwargs) - {"eps", "momentum"})
        if unknown:
            raise ValueError("MLP: norm_kwargs %s not supported ('eps', 'momentum')" % unknown)
        if not isinstance(dropout, (int, float)) or isinstance(dropout, bool) or not 0.0 <= dropout <= 1.0:
            raise ValueError("MLP: dropout must be a number in [0, 1], got %r" % (dropout,))
        if not isinstance(bias, bool):
            raise ValueError("MLP: bias must be a bool, got %r" % (bias,))
        self.channel_list = [int(c) for c in channel_list]
        self.act, self.act_first, self.plain_last, self.norm = act, bool(act_first), bool(plain_last), norm
        n_lins = len(self.channel_list) - 1
        self.dropout = [float(dropout)] * n_lins
        if self.plain_last:
            self.dropout[-1] = 0.0
        self.lins = torch.nn.ModuleList(torch.nn.Linear(a, b, bias=bias) for a, b in zip(self.channel_list[:-1], self.channel_list[1:]))
        widths = self.channel_list[1:-1] if self.plain_last else self.channel_list[1:]
        self.norms = torch.nn.ModuleList(_MLPBatchNorm(c, **norm_kwargs) if norm == "batch_norm" else torch.nn.Identity()
                                         for c in widths)

    @property
    def in_channels(self) -> int:
        return self.channel_list[0]

    @property
    def out_channels(self) -> int:
        return self.channel_list[-1]

    @property
    def num_layers(self) -> int:
        return len(self.channel_list) - 1

    def reset_parameters(self):
        for m in list(self.lins) + list(self.norms):
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()

    def flat_modules(self):
        """The equivalent flat list of torch modules, in ``forward``'s order (the Linears and BatchNorm1ds are this module's own;
        ReLU and Dropout are fresh, Dropout in this module's training mode): what ``GINConv`` applies its rules to."""
        mods = []
        for i, (lin, norm) in enumerate(zip(self.lins, self.norms)):
            mods.append(lin)
            if self.act is not None and self.act_first:
                mods.append(torch.nn.ReLU())
            if self.norm is not None:
                mods.append(norm.module)
            if self.act is not None and not self.act_first:
                mods.append(torch.nn.ReLU())
            if self.dropout[i] > 0.0:
                mods.append(torch.nn.Dropout(self.dropout[i]).train(self.training))
        if self.plain_last:
            mods.append(self.lins[-1])
        return mods

    def forward(self, x):
        for i, (lin, norm) in enumerate(zip(self.lins, self.norms)):
            x = lin(x)
            if self.act is not None and self.act_first:
                x = torch.relu(x)
            x = norm(x)
            if self.act is not None and not self.act_first:
                x = torch.relu(x)
            x = torch.nn.functional.dropout(x, p=self.dropout[i], training=self.training)
        if self.plain_last:
            x = self.lins[-1](x)
        return x

    def extra_repr(self) -> str:
        return str(self.channel_list)[1:-1]


def batch_norm_supported(H: int) -> bool:
    """Widths of the batch-norm kernels (``wgamd_batch_norm_supported``): H % 4 == 0, 4 <= H <= 256."""
    return bool(L.lib().wgamd_batch_norm_supported(int(H)))


def _tiles(n_rows: int) -> int:
    return (int(n_rows) + 15) // 16


def gin_layer_stats(row_ptr, col, x, self_rows, w1, b1, z_out, partials, counts, tile0: int, eps=None, src_ids=None, x_dst=None,
                    agg_out=None):
    """Launch A of the batch-norm route over one hop (``wgamd_gin_layer_f32_stats``): ``z = agg @ w1^T + b1`` into ``z_out``
    (``agg`` into ``agg_out`` when given) and the hop's per-tile ``(mean, M2)`` records into ``partials[tile0:]`` /
    ``counts[tile0:]`` (``partials`` float32 [T, 2, H], ``counts`` int32 [T])."""
    hop = _hop_args(row_ptr, col, x, src_ids) + _gin_hop_args(row_ptr, x, self_rows, x_dst, eps)
    n_rows, F_, H = row_ptr.shape[0] - 1, x.shape[1], w1.shape[0]
    assert w1.dtype == torch.float32 and w1.stride(1) == 1 and w1.shape[1] == F_
    assert z_out.shape == (n_rows, H) and z_out.stride(1) == 1 and (agg_out is None or (agg_out.shape == (n_rows, F_) and agg_out.stride(1) == 1))
    assert partials.dtype == torch.float32 and partials.is_contiguous() and partials.shape[1:] == (2, H)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.shape[0] == partials.shape[0] >= tile0 + _tiles(n_rows)
    L.check(L.lib().wgamd_gin_layer_f32_stats(*hop, w1.data_ptr(), w1.stride(0), H, _ptr(b1), z_out.data_ptr(), z_out.stride(0),
                                              _ptr(agg_out), 0 if agg_out is None else agg_out.stride(0), partials.data_ptr(),
                                              counts.data_ptr(), int(tile0), get_stream()), "wgamd_gin_layer_f32_stats")
    return z_out


def bn_finalize(partials, counts, gamma=None, beta=None, eps: float = 1e-5, momentum: float = 0.1, running_mean=None,
                running_var=None):
    """Launch B (``wgamd_bn_finalize_f32``): the per-tile records combined in a fixed order -> ``(mean, var, rstd, scale, shift)``
    (biased ``var``; ``scale = gamma rstd``, ``shift = beta - mean scale``), ``running_mean`` / ``running_var`` updated in place
    with ``momentum`` and the unbiased variance."""
    T, _, H = partials.shape
    stats = torch.empty((5, H), dtype=torch.float32, device=partials.device)
    for t in (gamma, beta, running_mean, running_var):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H,))
    L.check(L.lib().wgamd_bn_finalize_f32(partials.data_ptr(), counts.data_ptr(), T, H, _ptr(gamma), _ptr(beta), float(eps),
                                          float(momentum), _ptr(running_mean), _ptr(running_var), *(stats[k].data_ptr() for k in range(5)),
                                          get_stream()), "wgamd_bn_finalize_f32")
    return tuple(stats[k] for k in range(5))


def bn_act_linear(z, scale, shift, w2, b2=None, relu_out=False, keep=False):
    """Launch C (``wgamd_bn_act_linear_f32``): ``act(relu(z scale + shift) @ w2^T + b2)`` over all rows -> ``(out, hidden)``
    (``hidden`` None unless ``keep``)."""
    n, H = z.shape
    N = w2.shape[0]
    assert w2.dtype == torch.float32 and w2.stride(1) == 1 and w2.shape[1] == H and z.stride(1) == 1
    out = torch.empty((n, N), dtype=torch.float32, device=z.device)
    hidden = torch.empty((n, H), dtype=torch.float32, device=z.device) if keep else None
    L.check(L.lib().wgamd_bn_act_linear_f32(z.data_ptr(), z.stride(0), n, H, scale.data_ptr(), shift.data_ptr(), w2.data_ptr(),
                                            w2.stride(0), N, _ptr(b2), int(bool(relu_out)), out.data_ptr(), out.stride(0),
                                            _ptr(hidden), 0 if hidden is None else hidden.stride(0), get_stream()),
            "wgamd_bn_act_linear_f32")
    return out, hidden


def bn_column_stats(z):
    """``(mean, biased variance)`` of the columns of ``z`` [n, H] (float32 on the device, ``batch_norm_supported(H)``): the
    per-tile records of ``wgamd_bn_partials_f32`` combined by ``wgamd_bn_finalize_f32`` — the statistics of the batch-norm
    route on their own."""
    assert z.dim() == 2 and z.dtype == torch.float32 and z.is_cuda and z.stride(1) == 1
    n, H = z.shape
    T = _tiles(n)
    partials = torch.empty((T, 2, H), dtype=torch.float32, device=z.device)
    counts = torch.empty(T, dtype=torch.int32, device=z.device)
    L.check(L.lib().wgamd_bn_partials_f32(z.data_ptr(), z.stride(0), n, H, partials.data_ptr(), counts.data_ptr(), 0, get_stream()),
            "wgamd_bn_partials_f32")
    mean, var = bn_finalize(partials, counts)[:2]
    return mean, var


def bn_relu_backward(dhidden, hidden, z, mean, rstd, gamma):
    """``(dz, dgamma, dbeta)`` of ``hidden = relu((z - mean) rstd gamma + beta)`` over all rows (``wgamd_bn_bwd_reduce_f32`` then
    ``wgamd_bn_bwd_apply_f32``; no atomics); ``dz`` overwrites ``dhidden``."""
    n, H = z.shape
    assert dhidden.shape == (n, H) and dhidden.is_contiguous() and dhidden.dtype == torch.float32
    dev = z.device
    lib = L.lib()
    part = torch.empty((max(int(lib.wgamd_bn_bwd_blocks(n, H)), 1), 2, H), dtype=torch.float32, device=dev)
    dgb = torch.empty((2, H), dtype=torch.float32, device=dev)
    head = (dhidden.data_ptr(), dhidden.stride(0), hidden.data_ptr(), hidden.stride(0), z.data_ptr(), z.stride(0), n, H,
            mean.data_ptr(), rstd.data_ptr())
    L.check(lib.wgamd_bn_bwd_reduce_f32(*head, part.data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(), get_stream()),
            "wgamd_bn_bwd_reduce_f32")
    L.check(lib.wgamd_bn_bwd_apply_f32(*head, _ptr(gamma), dgb[0].data_ptr(), dgb[1].data_ptr(), dhidden.data_ptr(),
                                       dhidden.stride(0), get_stream()), "wgamd_bn_bwd_apply_f32")
    return dhidden, dgb[0], dgb[1]


def gin_bn_forward(hops, x, w1, b1, gamma, beta, w2, b2=None, bn_eps: float = 1e-5, momentum: float = 0.1, running_mean=None,
                   running_var=None, eps=None, relu_out=False, src_ids=None, keep=False):
    """The training forward of ``GINConv(MLP([F, H, N]))`` over ``hops`` — a list of ``(row_ptr, col, self_rows, x_dst)``, rows back
    to back: ``wgamd_gin_layer_f32_stats`` per hop, ONE ``wgamd_bn_finalize_f32`` (it updates the running statistics in place),
    ONE ``wgamd_bn_act_linear_f32``.  -> ``out``, or with ``keep`` ``(out, agg, z, hidden, mean, rstd)``."""
    H, F_ = w1.shape
    dev = w1.device
    sizes = [int(h[0].shape[0]) - 1 for h in hops]
    n, T = sum(sizes), sum(_tiles(s) for s in sizes)
    z = torch.empty((n, H), dtype=torch.float32, device=dev)
    agg = torch.empty((n, F_), dtype=torch.float32, device=dev) if keep else None
    partials = torch.empty((T, 2, H), dtype=torch.float32, device=dev)
    counts = torch.empty(T, dtype=torch.int32, device=dev)
    at = tile0 = 0
    for (row_ptr, col, self_rows, x_dst), s in zip(hops, sizes):
        if s > 0:
            rows = slice(at, at + s)
            gin_layer_stats(row_ptr, col, x, self_rows, w1, b1, z[rows], partials, counts, tile0, eps=eps, src_ids=src_ids,
                            x_dst=x_dst, agg_out=None if agg is None else agg[rows])
        at += s
        tile0 += _tiles(s)
    mean, _, rstd, scale, shift = bn_finalize(partials, counts, gamma, beta, bn_eps, momentum, running_mean, running_var)
    out, hidden = bn_act_linear(z, scale, shift, w2, b2, relu_out=relu_out, keep=keep)
    return (out, agg, z, hidden, mean, rstd) if keep else out


class _GinBnLayer(torch.autograd.Function):
    """The training-mode ``"mlp_bn"`` route over a ``LayerGraph`` (``gin_bn_forward``).  Backward, no atomics: dW2, db2 from the
    kept hidden activation, dHidden = dOut W2 (one library GEMM), the batch norm's own backward (``bn_relu_backward``: dgamma,
    dbeta, dz), then ``_GinLayer``'s lower half fed with dz."""

    @staticmethod
    def forward(ctx, src, x_dst, eps, w1, b1, gamma, beta, w2, b2, graph, ids, relu_out, n_src, no_root, bn):
        det = lambda t: None if t is None else t.detach()      # noqa: E731
        keep = any(ctx.needs_input_grad[:9])
        hops = []
        for h, rows, _ in _hops(graph):
            self_rows, xd = _gin_hop_self(h, rows, det(x_dst), no_root)
            hops.append((h.row_ptr, h.col, self_rows, xd))
        res = gin_bn_forward(hops, src, det(w1), det(b1), det(gamma), det(beta), det(w2), det(b2), bn_eps=bn.eps,
                             momentum=bn.momentum, running_mean=bn.running_mean, running_var=bn.running_var, eps=det(eps),
                             relu_out=relu_out, src_ids=ids, keep=keep)
        bn.num_batches_tracked.add_(1)
        if not keep:
            return res
        out, agg, z, hidden, mean, rstd = res
        ctx.save_for_backward(w1, w2, eps, out, x_dst, gamma)
        ctx.kept = (agg, z, hidden, mean, rstd)
        ctx.src = src if ctx.needs_input_grad[2] else None
        ctx.graph, ctx.ids, ctx.relu_out, ctx.n_src, ctx.no_root = graph, ids, relu_out, n_src, no_root
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        _released(ctx.kept, "GINConv", "activations")
        w1, w2, eps, out, x_dst, gamma = ctx.saved_tensors
        agg, z, hidden, mean, rstd = ctx.kept
        need_x, need_xd, need_eps, need_w1, need_b1, need_gamma, need_beta, need_w2, need_b2 = ctx.needs_input_grad[:9]
        H, F_ = w1.shape
        graph = ctx.graph
        g = g.contiguous().float()
        if ctx.relu_out:
            g = torch.ops.aten.threshold_backward(g, out, 0)
        gw1 = gb1 = gw2 = gb2 = None
        if need_w2 or need_b2:
            gw2, gb2 = _dense_wgrad(graph, hidden, g, w2, need_b2, None)
            gw2 = gw2 if need_w2 else None
        dz, dgamma, dbeta = bn_relu_backward(g @ w2, hidden, z, mean, rstd, gamma)      # dHidden: one library GEMM
        if need_w1 or need_b1:
            gw1, gb1 = _dense_wgrad(graph, agg, dz, w1, need_b1, None)
            gw1 = gw1 if need_w1 else None
        gx = gxd = geps = None
        has_self = not ctx.no_root and x_dst is None
        if need_x:
            gx = _gin_input_grad(graph, dz, ctx.n_src, eps, has_self, weight=_padded_wt(w1, H))
        if (need_xd or need_eps) and not ctx.no_root:
            d_agg = dz @ w1
            if need_xd:
                gxd = torch.zeros_like(x_dst, dtype=torch.float32)
                gxd[:d_agg.shape[0]] = (1.0 + eps) * d_agg
            if need_eps:
                geps = (d_agg * _gin_self_rows(ctx.src, ctx.ids, x_dst, graph)).sum().reshape(eps.shape)
        elif need_eps:
            geps = torch.zeros_like(eps)
        ctx.kept = None
        return (gx, gxd, geps, gw1, gb1, dgamma if need_gamma else None, dbeta if need_beta else None, gw2, gb2, None, None, None,
                None, None, None)


def _bn_folded_linear(lin1, bn, grad: bool):
    """``(W1', b1')`` with the eval-mode BatchNorm folded into the Linear before it: ``W1' = diag(s) W1``, ``b1' = s b1 + t``,
    ``s = gamma / sqrt(running_var + eps)``, ``t = beta - running_mean s`` — built once per weight change (``_derived``), or
    under autograd when a gradient is wanted."""
    def build():
        s = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        t = bn.bias - bn.running_mean * s
        return (lin1.weight * s[:, None]).contiguous(), (t if lin1.bias is None else lin1.bias * s + t).contiguous()
    params = (lin1.weight, lin1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    return _derived(bn, "folded_linear", params, build, extra=float(bn.eps), grad=grad)


class GINConv(torch.nn.Module):
    """PyG ``GINConv`` (``flow="source_to_target"``): ``x'_i = nn((1 + eps) x_i + sum_{j -> i} x_j)`` — every edge is summed,
    loop edges and duplicates too.  ``eps`` is a Parameter with ``train_eps`` and a buffer otherwise, ``nn`` any module
    (``nn.*`` in the state dict), so a PyG ``state_dict`` loads.

    ``forward(x, graph, act=None)``: ``graph`` = a COO ``edge_index`` (output rows = x's rows; ``x`` may be a pair
    ``(x_src, x_dst)``, ``x_dst = None`` = no root term), a ``[csr_row_ptr, csr_col_ind]`` pair (destinations = the first rows of
    x), or a call group's ``LayerGraph`` with ``x`` a tensor or ``LazyRows``.  ``act="relu"`` is the ``.relu()`` that follows the
    layer in the reference's model.  What runs depends on ``nn`` (``route``):

    * ``"mlp"`` — ``Sequential(Linear(F, H), ReLU(), Linear(H, N))``, the GIN paper's MLP: the whole layer is ONE kernel per hop
      (``wgamd_gin_layer_f32``: aggregate, both products, biases, ReLUs; the hidden activation never leaves LDS); an
      ``MLP([F, H, N], norm=None)`` is the same layer;
    * ``"mlp_bn"`` — ``MLP([F, H, N])`` with its defaults (``Linear -> BatchNorm1d -> ReLU -> Linear``, no dropout), the layer the
      reference's example trains.  Eval mode: the running statistics fold into ``W1``, ``b1`` and the layer is the ``"mlp"``
      kernel, ONE launch per hop.  Training mode: the layer kernel per hop with per-tile statistics
      (``wgamd_gin_layer_f32_stats``), one finalize launch (``wgamd_bn_finalize_f32``, which updates the running statistics) and
      one fused normalise -> ReLU -> ``W2`` launch (``wgamd_bn_act_linear_f32``); fewer than 2 rows: ValueError, as
      ``BatchNorm1d`` does;
    * ``"linear"`` — a ``Linear``, or a ``Sequential`` that starts with one (a ``ReLU`` right behind it included): one kernel for
      the aggregate and that product, the remaining modules run as they are (a ``Sequential`` with a BatchNorm between the
      Linears lands here, and any ``MLP`` outside the two routes above goes by its ``flat_modules()``);
    * ``"aggregate"`` — anything else, and shapes outside the kernel's domain (F % 4 == 0; F, H, N <= 256; H % 4 == 0 for
      ``"mlp"``): the aggregate kernel, then ``nn``.  CPU tensors run PyG's formulation in torch ops."""

    def __init__(self, nn: torch.nn.Module, eps: float = 0.0, train_eps: bool = False, **kwargs):
        super().__init__()
        if kwargs:
            raise TypeError("GINConv: unsupported keyword argument(s) %s (sum aggregation, flow source_to_target)"
                            % sorted(kwargs))
        if not isinstance(nn, torch.nn.Module):
            raise TypeError("GINConv: nn must be a torch.nn.Module")
        self.nn, self.initial_eps, self.train_eps = nn, float(eps), bool(train_eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer("eps", torch.empty(1))
        self.eps.data.fill_(self.initial_eps)

    def reset_parameters(self):
        for m in self.nn.modules():
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()
        self.eps.data.fill_(self.initial_eps)

    def _plan(self):
        """``(route, lin1, relu1, lin2, rest)``: the leading modules the kernel runs and the ones that follow it."""
        if isinstance(self.nn, MLP):
            m = self.nn
            bn = m.norms[0].module if m.norm == "batch_norm" and len(m.norms) == 1 else None
            if (bn is not None and len(m.lins) == 2 and m.act == "relu" and not m.act_first and m.plain_last and m.dropout[0] == 0.0
                    and bn.affine and bn.track_running_stats and isinstance(bn.momentum, float)
                    and gin_layer_supported(*m.channel_list)):
                return "mlp_bn", m.lins[0], True, m.lins[1], []
            mods = m.flat_modules()
        else:
            mods = list(self.nn) if isinstance(self.nn, torch.nn.Sequential) else [self.nn]
        if not mods or type(mods[0]) is not torch.nn.Linear:
            return "aggregate", None, False, None, [self.nn]
        lin1 = mods[0]
        relu1 = len(mods) > 1 and type(mods[1]) is torch.nn.ReLU
        rest = mods[2:] if relu1 else mods[1:]
        F_, H = lin1.in_features, lin1.out_features
        if relu1 and len(rest) == 1 and type(rest[0]) is torch.nn.Linear and gin_layer_supported(F_, H, rest[0].out_features):
            return "mlp", lin1, True, rest[0], []
        if gin_layer_supported(F_, H, 0):
            return "linear", lin1, relu1, None, rest
        return "aggregate", None, False, None, [self.nn]

    @property
    def route(self) -> str:
        """``"mlp"``, ``"mlp_bn"``, ``"linear"`` or ``"aggregate"``: what ``nn``'s form and shapes select on the device."""
        return self._plan()[0]

    def _forward_layer(self, x, lg: LayerGraph, act=None, x_dst=None, no_root=False):
        assert act in (None, "relu"), "act: None or 'relu'"
        relu = act == "relu"
        lazy = isinstance(x, LazyRows)
        F_ = x.shape[1]
        if x_dst is not None and x_dst.shape[1] != F_:
            raise ValueError("GINConv: x_dst has %d features, x_src %d" % (x_dst.shape[1], F_))
        src, ids, n_src, _ = _layer_input(self, x, lg, F_)
        if not src.is_cuda:                                     # CPU tensors: PyG's formulation
            out = self.nn(_gin_aggregate_torch(x.materialize() if lazy else x, x_dst, self.eps, lg, no_root))
            return torch.relu(out) if relu else out
        eps = self.eps if self.eps.dtype == torch.float32 else self.eps.float()
        route, lin1, relu1, lin2, rest = self._plan()
        bn = self.nn.norms[0].module if route == "mlp_bn" else None
        if route != "aggregate":
            ws = [t for t in (lin1.weight, lin1.bias, lin2 and lin2.weight, lin2 and lin2.bias) if t is not None]
            if bn is not None:
                ws += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
            ok = all(t.dtype == torch.float32 and t.is_cuda for t in ws) and _kernel_rows_ok(lin1.weight) and (
                lin2 is None or _kernel_rows_ok(lin2.weight)) and all(t.is_contiguous() for t in ws if t.dim() == 1) and (
                bn is None or all(t.data_ptr() % 16 == 0 for t in ws[-4:]))      # (the batch-norm kernels read [H] vectors as float4)
            if ok and lazy and not _kernel_rows_ok(src):
                x, lazy = x.materialize(), False
                src, ids = x, None
            if ok and not lazy and not _kernel_rows_ok(src):
                src = x = x.float().contiguous()
            if ok and x_dst is not None and not _kernel_rows_ok(x_dst):
                x_dst = x_dst.float().contiguous()
            if not ok or lin1.in_features != F_:
                route = "aggregate"
                rest = [self.nn]
        if route == "aggregate":
            xd = (x.materialize() if lazy else x).float().contiguous()
            out = _GinAggregate.apply(xd, None if x_dst is None else x_dst.float().contiguous(), eps, lg, no_root)
            out = self.nn(out)
            return torch.relu(out) if relu else out
        fuse_act = relu and not rest                            # the layer's ReLU rides in the kernel when nothing follows it
        if bn is not None and bn.training and lg.n_rows > 0:
            if lg.n_rows < 2:
                raise ValueError("GINConv: the batch norm of nn needs more than 1 row in training mode, got %d" % lg.n_rows)
            return _GinBnLayer.apply(src, x_dst, eps, lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias, lg, ids,
                                     fuse_act, n_src, no_root, bn)
        if bn is not None:                                      # eval mode (or no row at all): the "mlp" kernel on the folded W1, b1
            w1, b1 = (lin1.weight, lin1.bias) if bn.training else _bn_folded_linear(
                lin1, bn, torch.is_grad_enabled() and any(t.requires_grad for t in (lin1.weight, lin1.bias, bn.weight, bn.bias) if t is not None))
            return _GinLayer.apply(src, x_dst, eps, w1, b1, lin2.weight, lin2.bias, lg, ids, True, fuse_act, n_src, no_root)
        if lin2 is None:
            out = _GinLayer.apply(src, x_dst, eps, lin1.weight, lin1.bias, None, None, lg, ids, relu1 or fuse_act, False, n_src,
                                  no_root)
        else:
            out = _GinLayer.apply(src, x_dst, eps, lin1.weight, lin1.bias, lin2.weight, lin2.bias, lg, ids, True, fuse_act, n_src,
                                  no_root)
        for m in rest:
            out = m(out)
        return torch.relu(out) if relu and not fuse_act else out

    def forward(self, x, graph, act=None):
        _refuse_capture(self, "per-graph caches")              # (the hops' transposes, cached against the graph object)
        x_dst, pair = None, False
        if isinstance(x, (tuple, list)):
            (x, x_dst), pair = x, True
        _refuse_featureless(self, x)
        if x_dst is not None:
            _refuse_featureless(self, x_dst)
        if isinstance(graph, HeteroLayerGraph):
            raise NotImplementedError("GINConv over a heterogeneous call group's layer graph is not supported")
        if isinstance(graph, LayerGraph):
            if pair:
                raise NotImplementedError("GINConv: an (x_src, x_dst) pair over a LayerGraph is not supported")
            return self._forward_layer(x, graph, act)
        if isinstance(x, LazyRows):
            x = x.materialize()
        if isinstance(x_dst, LazyRows):
            x_dst = x_dst.materialize()
        if isinstance(graph, (tuple, list)):
            n_dst = int(graph[0].shape[0]) - 1
        elif not pair:
            n_dst = x.shape[0]
        elif x_dst is not None:
            n_dst = x_dst.shape[0]
        else:                                                   # (x_src, None): as many rows as the edges reach (one read-back)
            n_dst = int(graph[1].max()) + 1 if graph.shape[1] > 0 else 0
        have = x.shape[0] if not pair else (x_dst.shape[0] if x_dst is not None else n_dst)
        if have < n_dst:
            raise ValueError("GINConv: %d destination rows for %d destinations" % (have, n_dst))
        lg = _single_hop(graph, n_dst)[0]
        return self._forward_layer(x, lg, act, x_dst=None if x_dst is None else x_dst[:n_dst], no_root=pair and x_dst is None)


class _SegmentSum(torch.autograd.Function):
    """``out[g] = sum of rows [offsets[g], offsets[g + 1])`` of x (``wgamd_segment_sum_f32``: rows added in order, no atomics)."""

    @staticmethod
    def forward(ctx, x, offsets, batch):
        n_seg, F_ = offsets.shape[0] - 1, x.shape[1]
        out = torch.empty((n_seg, F_), dtype=torch.float32, device=x.device)
        if F_ > 0:
            L.check(L.lib().wgamd_segment_sum_f32(x.data_ptr(), x.stride(0), F_, offsets.data_ptr(), n_seg, out.data_ptr(),
                                                  out.stride(0), get_stream()), "wgamd_segment_sum_f32")
        ctx.save_for_backward(batch)
        return out

    @staticmethod
    def backward(ctx, g):
        (batch,) = ctx.saved_tensors
        return g[batch], None, None


def global_add_pool(x: torch.Tensor, batch: Optional[torch.Tensor], size: Optional[int] = None, ptr: Optional[torch.Tensor] = None):
    """PyG ``global_add_pool``: ``out[g] = sum of the rows of x with batch == g``, [size, F] (``size`` None: ``batch.max() + 1``,
    one read-back; ``batch`` None: one graph).  A sorted ``batch`` on the device runs ``wgamd_segment_sum_f32`` over its segment
    offsets — rows added in order, the same bits from run to run, empty graphs give zero rows.  ``ptr`` (PyG's ``Batch.ptr``)
    vouches that ``batch`` is sorted and gives ``size``; without it one ``(batch[1:] >= batch[:-1]).all()`` check is made.  An
    unsorted or CPU ``batch`` goes through ``index_add_``.  Gradient: ``grad[batch]``."""
    if batch is None:
        return x.sum(0, keepdim=True)
    assert x.dim() == 2 and batch.dim() == 1 and batch.shape[0] == x.shape[0]
    if size is None:
        size = int(ptr.shape[0]) - 1 if ptr is not None else (int(batch.max()) + 1 if batch.numel() > 0 else 0)
    size = int(size)
    batch = batch.long()
    on_device = x.is_cuda and batch.is_cuda and x.dtype == torch.float32
    if on_device and (ptr is not None or batch.numel() < 2 or bool((batch[1:] >= batch[:-1]).all())):
        if x.stride(1) != 1:
            x = x.contiguous()
        offsets = torch.searchsorted(batch.contiguous(), torch.arange(size + 1, device=batch.device))
        return _SegmentSum.apply(x, offsets.contiguous(), batch)
    return torch.zeros((size, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, batch, x)


# ---------------------------------------------------------------------------------------------------------------------
# GATv2 (torch_geometric.nn.GATv2Conv) — csrc/wg_gatv2.hip
# ---------------------------------------------------------------------------------------------------------------------
def gatv2_supported(H: int, C: int) -> bool:
    """Shapes of the GATv2 attention kernels (``wgamd_gatv2_supported``, answered on the host): 1 <= H <= 8, C % 4 == 0,
    H C <= 256."""
    return bool(L.lib().wgamd_gatv2_supported(int(H), int(C)))


def _gatv2_operands(row_ptr, col, xl, xr, att, heads: int, xr_rows):
    """The leading arguments the three GATv2 launches share, checked: ``row_ptr, col, n_rows, xl, ldxl, xr, ldxr, xr_rows, att,
    H, C`` (``col`` may be the transposed hop's; an empty one goes in as one element)."""
    H, HC = int(heads), int(xl.shape[1])
    assert HC % H == 0 and gatv2_supported(H, HC // H), "outside gatv2_supported"
    assert _kernel_rows_ok(xl) and _kernel_rows_ok(xr) and xr.shape[1] == HC, "xl / xr: float32 rows, 16-B aligned, unit column stride"
    assert att.dtype == torch.float32 and att.is_cuda and att.is_contiguous() and att.numel() == HC
    assert xr_rows is None or (xr_rows.dtype == torch.int64 and xr_rows.is_contiguous() and xr_rows.is_cuda)
    return (row_ptr.data_ptr(), _nonempty(col, torch.int32).data_ptr(), row_ptr.shape[0] - 1, xl.data_ptr(), xl.stride(0), xr.data_ptr(),
            xr.stride(0), _ptr(xr_rows), att.data_ptr(), H, HC // H)


def gatv2_attention(row_ptr, col, xl, xr, att, heads: int, negative_slope: float = 0.2, xr_rows=None, bias=None, relu=False, out=None,
                    need_alpha=False, mean=False):
    """The whole GATv2 attention of one hop in ONE launch (``wgamd_gatv2_attention_f32``, include/wgamd_ext.h): ``xl`` [n_src,
    H C] = lin_l(x_src) with ``col`` its rows, ``xr`` = lin_r over the destination rows, dense [n_rows, H C] or read at
    ``xr_rows`` (shared weights: ``xr = xl``, ``xr_rows`` = the destinations' input rows), ``att`` [1, H, C].  ``out``
    [n_rows, H C] — with ``mean`` (concat=False) [n_rows, C], the head mean taken in the launch — gets ``bias`` and ReLU fused;
    pass a slice of the layer's output to have the hop written in place.  Self loops are entries of the CSR.  With
    ``need_alpha`` returns ``(out, alpha [E, H], agg [n_rows, H C])``, what the backward reads.  An empty hop (no rows, or no
    entries at all) is filled without a launch: zeros plus bias."""
    _check_csr(row_ptr, col)
    H, HC, n_rows, E, dev = int(heads), int(xl.shape[1]), row_ptr.shape[0] - 1, int(col.shape[0]), row_ptr.device
    args = _gatv2_operands(row_ptr, col, xl, xr, att, H, xr_rows)
    N = HC // H if mean else HC
    assert xr_rows is not None or xr.shape[0] == n_rows
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N)
    out = _out_rows(out, n_rows, N, dev)
    alpha = torch.empty((E, H), dtype=torch.float32, device=dev) if need_alpha else None
    agg = torch.empty((n_rows, HC), dtype=torch.float32, device=dev) if need_alpha else None
    if n_rows > 0 and E == 0:
        out.zero_()
        if bias is not None:
            out.add_(bias)
        if relu:
            out.relu_()
        if agg is not None:
            agg.zero_()
    elif n_rows > 0:
        L.check(L.lib().wgamd_gatv2_attention_f32(*args, float(negative_slope), _ptr(bias), int(bool(relu)), int(bool(mean)),
                                                  out.data_ptr(), out.stride(0), _ptr(alpha), _ptr(agg), get_stream()),
                "wgamd_gatv2_attention_f32")
    return (out, alpha, agg) if need_alpha else out


def gatv2_bwd_dst(row_ptr, col, xl, xr, att, heads: int, alpha, g, agg, negative_slope: float = 0.2, xr_rows=None, dxr=None):
    """The destination-major backward launch of one hop (``wgamd_gatv2_bwd_dst_f32``): from ``g`` = dL/d agg [n_rows, H C] and
    the forward's ``alpha`` and ``agg`` returns ``(dxr [n_rows, H C], de [E, H], datt_part [blocks, H C])`` — the gradient of
    att is the sum of the partial rows."""
    H, HC, n_rows, dev = int(heads), int(xl.shape[1]), row_ptr.shape[0] - 1, row_ptr.device
    args = _gatv2_operands(row_ptr, col, xl, xr, att, H, xr_rows)
    assert _kernel_rows_ok(g) and g.shape == (n_rows, HC) and agg.is_contiguous() and alpha.is_contiguous()
    dxr = _out_rows(dxr, n_rows, HC, dev)
    assert dxr.is_contiguous()
    de = torch.empty((int(col.shape[0]), H), dtype=torch.float32, device=dev)
    part = torch.empty((int(L.lib().wgamd_gatv2_bwd_blocks(n_rows)), HC), dtype=torch.float32, device=dev)
    L.check(L.lib().wgamd_gatv2_bwd_dst_f32(*args, float(negative_slope), _nonempty(alpha, torch.float32).data_ptr(), g.data_ptr(),
                                            g.stride(0), agg.data_ptr(), dxr.data_ptr(), _nonempty(de, torch.float32).data_ptr(),
                                            part.data_ptr(), get_stream()), "wgamd_gatv2_bwd_dst_f32")
    return dxr, de, part


def gatv2_bwd_src(row_ptr_t, col_t, perm, xl, xr, att, heads: int, alpha, de, g, gx, negative_slope: float = 0.2, xr_rows=None,
                  accumulate=True):
    """The source-major backward launch of one hop over its transpose (``wgamd_gatv2_bwd_src_f32``): ``gx`` [n_src, H C] (+)= the
    hop's part of dL/d xl; ``row_ptr_t, col_t, perm`` as ``HopGraph.transposed(n_src, need_self=False, need_perm=True)`` gives them
    for the CSR the forward walked (self loops included)."""
    H = int(heads)
    args = _gatv2_operands(row_ptr_t, col_t, xl, xr, att, H, xr_rows)
    assert _kernel_rows_ok(g) and _kernel_rows_ok(gx) and gx.shape == xl.shape and row_ptr_t.shape[0] - 1 == xl.shape[0]
    L.check(L.lib().wgamd_gatv2_bwd_src_f32(args[0], args[1], perm.data_ptr(), *args[2:], float(negative_slope),
                                            _nonempty(alpha, torch.float32).data_ptr(), _nonempty(de, torch.float32).data_ptr(),
                                            g.data_ptr(), g.stride(0), gx.data_ptr(), gx.stride(0), int(bool(accumulate)), get_stream()),
            "wgamd_gatv2_bwd_src_f32")
    return gx


def _gatv2_hop(h: HopGraph, loops: bool) -> HopGraph:
    """The hop whose CSR the GATv2 kernels walk: ``h``, or — with self loops — ``h.with_self_loops()`` as a ``HopGraph`` of its
    own (kept on ``h``), whose ``transposed`` is then the transpose WITH the loops."""
    if not loops:
        return h
    rp, col = h.with_self_loops()
    hit = getattr(h, "_looped", None)
    if hit is None or hit.row_ptr is not rp:
        hit = h._looped = HopGraph(rp, col, h.self_rows)
    return hit


class _Gatv2Layer(torch.autograd.Function):
    """The GATv2 attention over a ``LayerGraph`` from the transformed rows: ONE ``wgamd_gatv2_attention_f32`` launch per hop, each
    writing its slice of the output in place (bias, ReLU and the head mean fused).  ``xr`` None = shared weights: XR[i] is
    ``xl[self_rows[i]]`` and its gradient is added into ``xl``'s at ``self_rows`` (injective: a plain indexed add).  When
    training the forward keeps alpha and agg per hop; the backward is ``wgamd_gatv2_bwd_dst_f32`` and ``wgamd_gatv2_bwd_src_f32``
    per hop, without atomics.  ``lin_l`` / ``lin_r`` and their gradients are ordinary autograd around this function."""

    @staticmethod
    def forward(ctx, xl, xr, att, bias, graph, loops, H, slope, relu, mean):
        lg, dev, HC = graph, xl.device, xl.shape[1]
        n = lg.n_rows
        train = any(ctx.needs_input_grad[:4])
        out = torch.empty((n, HC // H if mean else HC), dtype=torch.float32, device=dev)
        xl_d, xr_d = xl.detach(), None if xr is None else xr.detach()
        att_d, b_d = att.detach().contiguous(), None if bias is None else bias.detach().contiguous()
        kept = []
        for h, rows, _ in _hops(lg):
            res = None
            if h.n_rows > 0:
                hop = _gatv2_hop(h, loops)
                res = gatv2_attention(hop.row_ptr, hop.col, xl_d, xl_d if xr is None else xr_d[rows], att_d, H, slope,
                                      xr_rows=h.self_rows if xr is None else None, bias=b_d, relu=relu, out=out[rows],
                                      need_alpha=train, mean=mean)
            kept.append(res[1:] if train and res is not None else None)
        ctx.set_materialize_grads(False)
        if train:
            ctx.save_for_backward(xl_d, xr_d, att_d, out)
            ctx.kept, ctx.graph, ctx.conf = kept, lg, (loops, H, slope, relu, mean)
        return out

    @staticmethod
    def backward(ctx, g):
        _released(ctx.kept, "GATv2Conv", "attention weights")
        xl, xr, att, out = ctx.saved_tensors
        need_xl, need_xr, need_att, need_b = ctx.needs_input_grad[:4]
        loops, H, slope, relu, mean = ctx.conf
        lg, dev, HC = ctx.graph, xl.device, xl.shape[1]
        n, n_src = lg.n_rows, xl.shape[0]
        gxl = gxr = gatt = gb = None
        if g is None:
            g = torch.zeros_like(out)
        gz = g.contiguous().float()
        if relu:
            gz = torch.ops.aten.threshold_backward(gz, out, 0)
        if need_b:
            gb = gz.sum(0)
        if need_xl or need_xr or need_att:
            G = (gz * (1.0 / H)).repeat(1, H) if mean else gz                # dL/d agg [n, H C]
            gxl = torch.zeros((n_src, HC), dtype=torch.float32, device=dev)
            gxr = None if xr is None else torch.zeros((n, HC), dtype=torch.float32, device=dev)
            parts = []
            for k, (h, rows, _) in enumerate(_hops(lg)):
                if h.n_rows == 0:
                    continue
                hop = _gatv2_hop(h, loops)
                if hop.col.shape[0] == 0:
                    continue
                alpha, agg = ctx.kept[k]
                xr_h, xr_rows = (xl, h.self_rows) if xr is None else (xr[rows], None)
                dxr, de, part = gatv2_bwd_dst(hop.row_ptr, hop.col, xl, xr_h, att, H, alpha, G[rows], agg, slope, xr_rows=xr_rows,
                                              dxr=None if xr is None else gxr[rows])
                parts.append(part)
                row_ptr_t, col_t, _, perm = hop.transposed(n_src, need_self=False, need_perm=True)
                gatv2_bwd_src(row_ptr_t, col_t, perm, xl, xr_h, att, H, alpha, de, G[rows], gxl, slope, xr_rows=xr_rows)
                if xr is None:
                    gxl[h.self_rows] += dxr
            gatt = (torch.cat(parts).sum(0) if parts else torch.zeros(HC, dtype=torch.float32, device=dev)).view(1, H, HC // H)
        ctx.kept = None
        return gxl, gxr, gatt, gb, None, None, None, None, None, None


def _gatv2_torch_ops(conv, xs, x_dst, lg: LayerGraph, relu: bool):
    """The layer in PyG's own formulation, composed of torch ops under ordinary autograd in the parameters' dtype: the route of
    shapes outside the kernel's domain and of CPU tensors (correctness, not speed — [E, H, C] is materialised three times)."""
    H, C, dt = conv.heads, conv.out_channels, conv.att.dtype
    xs = xs.to(dt)
    XL = conv.lin_l(xs).view(-1, H, C)
    outs = []
    for h, rows, _ in _hops(lg):
        n, E = h.n_rows, int(h.col.shape[0])
        XR = conv.lin_r(x_dst[rows].to(dt) if x_dst is not None else xs[h.self_rows]).view(n, H, C)
        src, dst = h.col.long(), _edge_dst(h.row_ptr, E)
        if conv.add_self_loops:
            src, dst = torch.cat([h.self_rows, src]), torch.cat([torch.arange(n, device=dst.device), dst])
        xj = XL[src]
        e = (torch.nn.functional.leaky_relu(xj + XR[dst], conv.negative_slope) * conv.att).sum(-1)       # [E', H]
        emax = e.new_full((n, H), -math.inf).scatter_reduce(0, dst.unsqueeze(1).expand(-1, H), e, "amax", include_self=True)
        ex = (e - emax[dst]).exp()
        alpha = ex / e.new_zeros((n, H)).index_add(0, dst, ex)[dst]
        o = e.new_zeros((n, H, C)).index_add(0, dst, alpha.unsqueeze(2) * xj)
        outs.append(o.reshape(n, H * C) if conv.concat else o.mean(1))
    out = torch.cat(outs) if outs else xs.new_zeros((0, H * C if conv.concat else C))
    if conv.bias is not None:
        out = out + conv.bias
    return torch.relu(out) if relu else out


class GATv2Conv(torch.nn.Module):
    """PyG ``GATv2Conv`` (flow source_to_target):
        e_ijh = att_h . LeakyReLU(lin_l(x_j) + lin_r(x_i))_h,   alpha = softmax_j(e_ijh),   out_i = sum_j alpha_ijh lin_l(x_j)_h
    per head; ``concat=True`` concatenates the heads ([N, H C]), ``concat=False`` averages them ([N, C]); then ``bias``.
    Parameters as PyG names them (``lin_l``, ``lin_r``: ``weight`` [H C, in] and ``bias``; ``att`` [1, H, C]; ``bias``), glorot
    weights and zero biases, so a PyG ``state_dict`` loads; ``share_weights=True``: ``lin_r is lin_l``.  Self loops follow
    ``GATConv`` here: the destination's own input row is one extra leading neighbour, sampled loops and duplicate edges stay
    ordinary edges; a destination without any entry gets zeros plus bias.

    ``forward(x, graph, act=None)``: ``graph`` = a COO ``edge_index`` (output rows = x's rows, or x_dst's for a pair), a
    ``[csr_row_ptr, csr_col_ind]`` pair (destinations = the first rows of x), or a call group's ``LayerGraph`` with x a tensor or
    ``LazyRows`` (materialised once; 16-bit tables arrive as float32 rows) and ``act=None | "relu"`` — the output rows are the
    hops' destination lists back to back, every hop written in place into its slice.  ``x`` may be a pair ``(x_src, x_dst)``:
    the sampler layout (x_dst = the first rows of x_src in the same storage) keeps self loops, any other pair needs
    ``add_self_loops=False`` (ValueError otherwise: a foreign destination row is no row of lin_l's input).

    The logit's nonlinearity sits inside the dot product with ``att``, so there is no aggregate-first form (as ``GATConv`` and
    ``TransformerConv`` have): ``XL = lin_l(x)`` is one library GEMM over all input rows of the layer, ``XR = lin_r`` one over
    the destination rows (none with shared weights: the kernel reads ``XL[self_rows]``), and ONE kernel per hop
    (``wgamd_gatv2_attention_f32``) scores, soft-maxes and sums the transformed neighbour rows, reading each once; bias, ReLU and
    the head mean of ``concat=False`` are done IN that launch.  The backward is two more kernels per hop, without atomics (the
    same bits from run to run).  ``route``: ``"kernel"`` inside ``gatv2_supported`` (heads <= 8, out_channels % 4 == 0,
    heads x out_channels <= 256) with float32 tensors on the device, else ``"torch"`` — the same layer out of torch ops with
    ordinary autograd, CPU tensors included, for correctness only (``torch_ops = True`` forces it).

    Not supported: ``edge_dim``, ``fill_value``, ``residual`` and any other keyword (TypeError), attention dropout (``dropout >
    0`` raises NotImplementedError in training mode; in eval mode it is the identity), a ``HeteroLayerGraph``
    (NotImplementedError), ``HeteroConv`` relations, HIP-graph capture."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True, bias: bool = True,
                 share_weights: bool = False, **kwargs):
        super().__init__()
        if kwargs:
            raise TypeError("GATv2Conv: unsupported keyword argument(s) %s" % ", ".join(sorted(kwargs)))
        if heads < 1 or out_channels < 1:
            raise ValueError("GATv2Conv: heads and out_channels must be positive")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.in_src, self.in_dst = int(in_channels[0]), int(in_channels[1])
        self.negative_slope, self.dropout, self.add_self_loops = float(negative_slope), float(dropout), add_self_loops
        self.share_weights = share_weights
        self.torch_ops = False
        HC = heads * out_channels
        self.lin_l = torch.nn.Linear(self.in_src, HC, bias=bias)
        self.lin_r = self.lin_l if share_weights else torch.nn.Linear(self.in_dst, HC, bias=bias)
        self.att = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(HC if concat else out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        def glorot(t):
            bound = math.sqrt(6.0 / (t.shape[-2] + t.shape[-1]))
            torch.nn.init.uniform_(t, -bound, bound)
        for lin in (self.lin_l, self.lin_r):
            glorot(lin.weight)
            if lin.bias is not None:
                torch.nn.init.zeros_(lin.bias)
        glorot(self.att)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    @property
    def route(self) -> str:
        """``"kernel"`` or ``"torch"``: what the shapes and the parameters' dtype and device select for float32 device inputs."""
        ok = (not self.torch_ops and self.att.is_cuda and self.att.dtype == torch.float32
              and gatv2_supported(self.heads, self.out_channels))
        return "kernel" if ok else "torch"

    def _forward_layer(self, x, lg: LayerGraph, act=None, x_dst=None):
        assert act in (None, "relu"), "act: None or 'relu'"
        x = _x16_as_rows(x)
        if isinstance(x, LazyRows):
            _refuse_lazy_table_grad(x.table)
            x = x.materialize()
        if x.shape[1] != self.in_src:
            raise ValueError("GATv2Conv: x has %d features, the layer takes %d" % (x.shape[1], self.in_src))
        if x_dst is not None and x_dst.shape[1] != (self.in_src if self.share_weights else self.in_dst):
            raise ValueError("GATv2Conv: x_dst has %d features, the layer takes %d"
                             % (x_dst.shape[1], self.in_src if self.share_weights else self.in_dst))
        if x_dst is None and self.in_src != self.in_dst and not self.share_weights:
            raise ValueError("GATv2Conv: in_channels = %s needs an (x_src, x_dst) pair" % (self.in_channels,))
        on_device = all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in (x, x_dst))
        if self.route != "kernel" or not on_device:
            return _gatv2_torch_ops(self, x, x_dst, lg, act == "relu")
        XL = self.lin_l(x)
        if x_dst is not None:
            XR = self.lin_r(x_dst)
        elif self.share_weights:
            XR = None
        else:
            dev = x.device
            self_all = torch.cat([h.self_rows for h in lg.hops]) if lg.hops else torch.zeros(0, dtype=torch.int64, device=dev)
            XR = self.lin_r(x[self_all])
        return _Gatv2Layer.apply(XL, XR, self.att, self.bias, lg, bool(self.add_self_loops), self.heads, self.negative_slope,
                                 act == "relu", not self.concat)

    def forward(self, x, graph, act=None):
        if self.dropout > 0 and self.training:
            raise NotImplementedError("GATv2Conv: attention dropout (dropout > 0 in training mode) is not supported")
        _refuse_capture(self, "per-graph caches")              # (the hops' self-looped CSR and transposes, kept on the graph object)
        if isinstance(graph, HeteroLayerGraph):
            raise NotImplementedError("GATv2Conv over a heterogeneous call group's layer graph is not supported")
        x_dst, pair = None, False
        if isinstance(x, (tuple, list)):
            (x, x_dst), pair = x, True
        _refuse_featureless(self, x)
        if pair:
            _refuse_featureless(self, x_dst)
        if isinstance(graph, LayerGraph):
            if pair:
                raise NotImplementedError("GATv2Conv: an (x_src, x_dst) pair over a LayerGraph is not supported")
            return self._forward_layer(x, graph, act)
        if isinstance(x, LazyRows):
            x = _x16_as_rows(x)
            x = x.materialize() if isinstance(x, LazyRows) else x
        if isinstance(x_dst, LazyRows):
            x_dst = _x16_as_rows(x_dst)
            x_dst = x_dst.materialize() if isinstance(x_dst, LazyRows) else x_dst
        if pair:
            # the sampler layout: the destinations are the first rows of x_src, in the same storage
            own = x_dst is x or (x_dst.data_ptr() == x.data_ptr() and x_dst.dtype == x.dtype and x_dst.stride() == x.stride()
                                 and x_dst.shape[0] <= x.shape[0] and x_dst.shape[1] == x.shape[1])
            if not own and self.add_self_loops:
                raise ValueError("GATv2Conv: an (x_src, x_dst) pair whose destinations are not the first rows of x_src needs "
                                 "add_self_loops=False (a self loop reads the destination's own row of x_src)")
        if isinstance(graph, (tuple, list)):
            n_dst = int(graph[0].shape[0]) - 1
        else:
            n_dst = x_dst.shape[0] if pair else x.shape[0]
        have = x_dst.shape[0] if pair else x.shape[0]
        if have < n_dst:
            raise ValueError("GATv2Conv: %d destination rows for %d destinations" % (have, n_dst))
        lg = _single_hop(graph, n_dst)[0]
        return self._forward_layer(x, lg, act, x_dst=x_dst[:n_dst] if pair and not own else None)


# ---------------------------------------------------------------------------------------------------------------------
# heterogeneous layers over a call group (BASELINE configs[4]: ogbn-mag-like 2-hop walk + HeteroConv{GATConv})
# ---------------------------------------------------------------------------------------------------------------------
_stage_hook = None


def set_stage_hook(hook):
    """``hook(name, fn) -> fn()`` wraps every device stage of the call-group layers (bench_mag.py times them with HIP events);
    ``None`` = plain calls."""
    global _stage_hook
    _stage_hook = hook


def _stage(name, fn):
    return fn() if _stage_hook is None else _stage_hook(name, fn)


class RelationHop:
    """One (hop, edge type) of a heterogeneous call group as a layer consumes it: CSR over the hop's frontier entries of the
    destination type (``row_ptr`` int32 [n + 1]); ``col`` int32 = row of every edge's source in the layer's INPUT of the source
    type; ``dst_rows`` int64 [n] = row of every frontier entry in the layer's input of the destination type (its attention
    term); ``out_rows`` int64 [n] = its row in the layer's OUTPUT of the destination type (None: entry j is output row j);
    ``edge_base`` = row of the hop's first edge in the edge type's hop-major per-edge tensors (``edge_attr_dict[edge_type]``:
    the number of edges of the same edge type in the earlier hops)."""

    def __init__(self, edge_type, hop, row_ptr, col, dst_rows, out_rows, n_edges, fanout, edge_base=0):
        self.edge_type, self.hop, self.row_ptr, self.col = edge_type, hop, row_ptr, col
        self.dst_rows, self.out_rows, self.n_edges, self.fanout = dst_rows, out_rows, int(n_edges), int(fanout)
        self.edge_base = int(edge_base)

    @property
    def n_rows(self):
        return int(self.row_ptr.shape[0]) - 1


class HeteroLayerGraph:
    """What ONE layer of a trimmed heterogeneous GNN runs over (``cugraph_pyg_amd.loader.HeteroCallGroup.layer_graph``): the
    relation hops, and per node type the number of output rows (every output row of a type is a frontier entry of exactly one
    hop of that type).  ``num_group_edges`` ({edge type: edges of the whole call group}, None for a user-built graph): the
    length of the edge type's hop-major per-edge tensors, of which every layer reads the prefix of its hops."""

    def __init__(self, relations, n_out, node_types, num_group_edges=None):
        self.relations, self.n_out, self.node_types = list(relations), dict(n_out), list(node_types)
        self.num_group_edges = None if num_group_edges is None else dict(num_group_edges)

    @property
    def num_edges(self):
        return sum(r.n_edges for r in self.relations)


def _relation_groups(graph: HeteroLayerGraph):
    """``[((hop, dst_type), [RelationHop, ...]), ...]`` sorted by hop, then type: the relation hops of a layer graph that add up
    to the same output rows (in the graph's order; they share ``n_rows``, ``dst_rows`` and ``out_rows``)."""
    groups = {}
    for r in graph.relations:
        groups.setdefault((r.hop, r.edge_type[2]), []).append(r)
    return sorted(groups.items(), key=lambda kv: kv[0])


def _group_outputs(graph: HeteroLayerGraph, groups, width, device, make=torch.empty):
    """``{type: make([n_out, width(type)])}`` float32 for the node types some group of ``groups`` ends in."""
    ends = {dt for (_, dt), _ in groups}
    return {t: make((n, width(t)), dtype=torch.float32, device=device) for t, n in graph.n_out.items() if n > 0 and t in ends}


def _place_rows(out, dt, y, out_rows):
    """The rows ``y`` of one group in the output of type ``dt``: the output itself (``out_rows`` None: row j is output row j), or
    copied to ``out_rows`` in place — the hops of a type write disjoint rows of one buffer."""
    if out_rows is None:
        out[dt] = y
    else:
        out[dt].index_copy_(0, out_rows, y)


from .pool import GrowOnlyPool  # noqa: E402

_agg_pool = GrowOnlyPool()


class _NarrowTerms(torch.autograd.Function):
    """``terms = x @ v`` for a LONG ``x`` ([n, F], a feature table or a hidden state) and a narrow ``v`` ([F, T], T <= 32: the
    folded attention vectors of a node type).  Forward: ``rows_terms`` (one streaming pass, exact-fp32 MFMA) where the shape
    allows, a library product otherwise; backward: ``dv = x^T @ dterms`` by ``wgamd_rows_terms_bwd_f32`` (x streamed once; a
    library GEMM sees a 128 x 12 output and a reduction over a million rows), ``dx = dterms @ v^T`` only where x asks for it."""

    @staticmethod
    def forward(ctx, x, v):
        v = v.contiguous()
        F_, T = int(v.shape[0]), int(v.shape[1])
        fast = _kernel_rows_ok(x) and gather_terms_supported(F_, T)
        terms = rows_terms(x, v) if fast and x.shape[0] > 0 else x @ v
        ctx.save_for_backward(x, v)
        return terms

    @staticmethod
    def backward(ctx, g):
        x, v = ctx.saved_tensors
        g = g.contiguous()
        F_, T = int(v.shape[0]), int(v.shape[1])
        dv = None
        if ctx.needs_input_grad[1]:
            if x.stride(1) == 1 and F_ <= 256 and T <= 32 and x.shape[0] > 0:
                dv = torch.zeros((F_, T), dtype=torch.float32, device=g.device)
                L.check(L.lib().wgamd_rows_terms_bwd_f32(x.data_ptr(), x.stride(0), int(x.shape[0]), F_, g.data_ptr(), T, dv.data_ptr(),
                                                         get_stream()), "wgamd_rows_terms_bwd_f32")
            else:
                dv = x.t() @ g
        dx = g @ v.t() if ctx.needs_input_grad[0] else None
        return dx, dv


class _GatAggregateHeads(torch.autograd.Function):
    """``gat_aggregate_heads`` under autograd: the aggregate-first GAT aggregation of a sampled hop with gradients for the
    attention terms (at the rows the forward read them from: per listed row, or per TABLE row) and, when ``x`` requires it, for
    the source rows (``wgamd_gat_aggregate_heads_bwd_f32``; float atomics: reproducible to fp32 rounding).  The dense tail —
    per-head weights, the sum over relations, bias — stays in torch on the few destination rows."""

    @staticmethod
    def forward(ctx, x, a_src, a_dst, row_ptr, col, heads, dst_rows, src_ids, dst_ids, src_by_id, dst_by_id, slope):
        a_src, a_dst = a_src.contiguous(), a_dst.contiguous()
        # (the [rows, heads x F] aggregate is gigabytes per hop of a call group and changes size by a per cent from group to
        #  group: a grow-only buffer instead of a hipMalloc / hipFree pair per hop — recycled once nothing holds it any more)
        out = _agg_pool.take((int(row_ptr.shape[0]) - 1, heads * int(x.shape[1])), torch.float32, x.device)
        agg = gat_aggregate_heads(row_ptr, col, x, a_src, a_dst, heads, dst_rows=dst_rows, negative_slope=slope, out=out, src_ids=src_ids,
                                  dst_ids=dst_ids, src_terms_by_id=src_by_id, dst_terms_by_id=dst_by_id)
        ctx.save_for_backward(x, a_src, a_dst, row_ptr, col)
        ctx.extra = (heads, dst_rows, src_ids, dst_ids, src_by_id, dst_by_id, slope)
        return agg

    @staticmethod
    def backward(ctx, g):
        x, a_src, a_dst, row_ptr, col = ctx.saved_tensors
        heads, dst_rows, src_ids, dst_ids, src_by_id, dst_by_id, slope = ctx.extra
        g = g.contiguous()
        n_rows, F_ = row_ptr.shape[0] - 1, x.shape[1]
        ga_src, ga_dst = torch.zeros_like(a_src), torch.zeros_like(a_dst)
        de = torch.empty((max(int(col.shape[0]), 1), heads), dtype=torch.float32, device=g.device)
        ids_p, dids_p, by_id = _gat_ids(src_ids, dst_ids, a_src, src_by_id, dst_by_id)
        want_gx = ctx.needs_input_grad[0]
        # the source rows' gradient: source-major over the transposed hop (every row written once) where the addressing is plain —
        # a hidden-state input —, float atomics (F per edge) otherwise
        transposed = want_gx and src_ids is None and int(col.shape[0]) > 0
        gx = torch.zeros_like(x) if (want_gx and not transposed) else None
        stats = torch.empty((2, n_rows, heads), dtype=torch.float32, device=g.device) if transposed else None
        L.check(L.lib().wgamd_gat_aggregate_heads_bwd_f32(
            row_ptr.data_ptr(), col.data_ptr(), n_rows, x.data_ptr(), x.stride(0), ids_p, dids_p, by_id, F_, a_src.data_ptr(),
            a_dst.data_ptr(), heads, float(slope), None if dst_rows is None else dst_rows.data_ptr(), g.data_ptr(), g.stride(0),
            de.data_ptr(), ga_src.data_ptr(), ga_dst.data_ptr(), None if gx is None else gx.data_ptr(),
            0 if gx is None else gx.stride(0), None if stats is None else stats.data_ptr(), get_stream()),
            "wgamd_gat_aggregate_heads_bwd_f32")
        if transposed:
            n_src = int(x.shape[0])
            hit = getattr(row_ptr, "_wgamd_gat_t", None)          # (one transpose per hop CSR, kept on the tensor the layer graph holds)
            if hit is None or hit[0] != n_src or hit[1] != col.data_ptr():
                row_ptr_t, _, _, col_t = _csr_transpose(row_ptr, col, n_src, want_col_t=True)
                hit = (n_src, col.data_ptr(), row_ptr_t, col_t)
                try:
                    row_ptr._wgamd_gat_t = hit
                except AttributeError:
                    pass
            gx = torch.empty_like(x)
            L.check(L.lib().wgamd_gat_aggregate_heads_bwd_gx_f32(
                hit[2].data_ptr(), hit[3].data_ptr(), n_src, n_rows, F_, a_src.data_ptr(), a_dst.data_ptr(), heads, float(slope),
                None if dst_rows is None else dst_rows.data_ptr(), stats.data_ptr(), g.data_ptr(), g.stride(0), gx.data_ptr(),
                gx.stride(0), get_stream()), "wgamd_gat_aggregate_heads_bwd_gx_f32")
        return gx, ga_src, ga_dst, None, None, None, None, None, None, None, None, None


# ---- heterogeneous SAGE layer: one launch per (hop, destination type) ---------------------------------------------------------
HETERO_SAGE_MAX_K = 1024          # floats of one launch's C row (the 16 x (K + 4) fp32 LDS tile of wg_sage_hetero.hip)
hetero_sage_launches = 0          # wgamd_hetero_sage_layer_f32(_train) launches so far (tests: the kernel route ran)


def hetero_sage_plan(widths, F_dst: int = 0, max_k: int = HETERO_SAGE_MAX_K, max_rel: int = L.HETERO_SAGE_MAX_RELATIONS):
    """The launches of one (hop, destination type) group whose relation blocks are ``widths`` floats wide (in order) and whose
    root block is ``F_dst`` wide (0: none): ``[(lo, hi, root), ...]`` — launch k reduces relations ``[lo, hi)``; whole
    relations, in order, at most ``max_rel`` of them and ``K <= max_k`` floats per launch (greedy: a launch takes relations
    while they fit).  Only the LAST launch has ``root`` — with it go the bias, the activation and the row placement; every
    launch but the first adds the running sum of the ones before it.  A root block that does not fit next to the last
    relations gets a launch of its own.  ValueError when a single block is wider than ``max_k``."""
    widths = [int(w) for w in widths]
    if any(w <= 0 or w > max_k for w in widths) or not 0 <= F_dst <= max_k:
        raise ValueError("hetero_sage_plan: a block of %s + [%d] floats does not fit a launch (K <= %d)" % (widths, F_dst, max_k))
    plan, lo, k = [], 0, 0
    for i, w in enumerate(widths):
        if k + w > max_k or i - lo == max_rel:
            plan.append((lo, i, False))
            lo, k = i, 0
        k += w
    if k + F_dst > max_k:
        plan.append((lo, len(widths), False))
        lo, k = len(widths), 0
    if lo < len(widths) or F_dst > 0 or not plan:
        plan.append((lo, len(widths), F_dst > 0))
    return plan


def _sage_ids_kind(ids) -> int:
    return 0 if ids is None else (1 if ids.dtype == torch.int32 else 2)


def _hetero_launch_tail(name: str, relu_flag: int, arr, n_rel: int, at: int, n_rows: int, wt, N: int, root, bias, relu, acc_in,
                        out_rows, out, kept):
    """The second half of ``hetero_sage_launch`` / ``hetero_transformer_launch``: the relation descriptors ``arr`` (``n_rel`` of
    them, ``at`` floats wide together) are filled; unpacks the root, checks ``wt``, ``out``, ``acc_in``, ``out_rows`` and the
    ``kept`` rows, and calls the library's ``name`` (``name + "_train"`` with ``kept``).  Returns ``out``."""
    x_dst, dst_rows, dst_ids = root if root is not None else (None, None, None)
    if x_dst is not None:
        assert x_dst.dtype == torch.float32 and x_dst.stride(1) == 1 and (dst_rows is None or dst_rows.dtype == torch.int64)
        at += int(x_dst.shape[1])
    assert wt.dtype == torch.float32 and wt.stride(1) == 1 and wt.shape[0] == N and wt.shape[1] >= at
    if out is None:
        out = torch.empty((n_rows, N), dtype=torch.float32, device=wt.device)
    assert out.stride(1) == 1 and out.shape[1] == N and (acc_in is None or (acc_in.stride(1) == 1 and acc_in.shape == (n_rows, N)))
    assert out_rows is None or (out_rows.dtype == torch.int64 and out_rows.is_contiguous())
    args = (arr, n_rel, n_rows, _ptr(x_dst), 0 if x_dst is None else x_dst.stride(0), 0 if x_dst is None else int(x_dst.shape[1]),
            _ptr(dst_rows), _ptr(dst_ids), _sage_ids_kind(dst_ids), wt.data_ptr(), wt.stride(0), N, _ptr(bias),
            relu_flag if relu else 0, _ptr(acc_in), 0 if acc_in is None else acc_in.stride(0), _ptr(out_rows),
            out.data_ptr(), out.stride(0))
    if kept is not None:
        assert kept.stride(1) == 1 and kept.shape[0] == n_rows and kept.shape[1] >= at
        name, args = name + "_train", args + (kept.data_ptr(), kept.stride(0))
    L.check(getattr(L.lib(), name)(*args, get_stream()), name)
    return out


def hetero_sage_launch(rels, n_rows: int, wt, N: int, root=None, bias=None, relu=False, acc_in=None, out_rows=None, out=None,
                       c_out=None):
    """One ``wgamd_hetero_sage_layer_f32`` launch (include/wgamd_ext.h).  ``rels``: ``[(row_ptr, col, x, ids, scale, mean), ...]``
    (x [*, F] float32 rows, ``ids`` the node list x is read through or None, ``scale`` a per-source-row factor or None);
    ``root``: ``(x_dst, dst_rows, dst_ids)`` or None; ``wt`` [N, >= K] (a column slice of the stacked weight); ``c_out``
    [n_rows, >= K]: the launch also keeps its C rows (``_train``)."""
    global hetero_sage_launches
    arr = (L.HeteroSageRelation * max(len(rels), 1))()
    keep, at = [], 0
    for k, (row_ptr, col, x, ids, scale, mean) in enumerate(rels):
        _check_csr(row_ptr, col)
        assert row_ptr.shape[0] == n_rows + 1 and x.dtype == torch.float32 and x.stride(1) == 1
        assert ids is None or ids.is_contiguous()
        col = _nonempty(col, torch.int32)
        keep.append(col)
        d = arr[k]
        d.row_ptr, d.col, d.x, d.ldx = row_ptr.data_ptr(), col.data_ptr(), x.data_ptr(), x.stride(0)
        d.src_ids, d.src_scale = _ptr(ids), _ptr(scale)
        d.F, d.ids_kind, d.mean, d.col0 = int(x.shape[1]), _sage_ids_kind(ids), int(bool(mean)), at
        at += int(x.shape[1])
    out = _hetero_launch_tail("wgamd_hetero_sage_layer_f32", L.HETERO_SAGE_RELU, arr, len(rels), at, n_rows, wt, N, root, bias, relu,
                              acc_in, out_rows, out, c_out)
    hetero_sage_launches += 1
    return out


class _HeteroGroup:
    """What one (hop, destination type) group of a hetero layer launches over: the relation ``blocks``, the root ``(x_dst,
    dst_rows, dst_ids)`` or None, the plan (``hetero_sage_plan``), and the ``RelationHop`` of every block (None: the hop lists
    no such relation) for the transposes of the backward pass.  A subclass names its stages (``stage``) and supplies
    ``launch`` (its ``hetero_*_launch``), ``rels(lo, hi, *operands)`` — the relation tuples of blocks ``[lo, hi)`` — and
    ``first_col(lo)``, the first column of block ``lo`` in the stacked weight."""

    def __init__(self, blocks, hops, root, plan, n_rows, N, relu, tag):
        self.blocks, self.hops, self.root, self.plan = blocks, hops, root, plan
        self.n_rows, self.N, self.relu, self.tag = n_rows, N, relu, tag

    def run(self, wt, bias, *operands, out=None, out_rows=None, kept=None):
        """The group's launches -> act(tile @ wt^T + bias), placed through ``out_rows`` into ``out`` when given; bias, ReLU,
        placement and root go with the last launch, every launch but the first adds the running sum of the ones before."""
        acc = None
        for k, (lo, hi, with_root) in enumerate(self.plan):
            last = k == len(self.plan) - 1
            rels, at = self.rels(lo, hi, *operands), self.first_col(lo)
            names = ",".join(str(h.edge_type[1]) for h in self.hops[lo:hi] if h is not None)
            name = "%s%s:%s (%d rows, launch %d/%d)" % (self.stage, self.tag, names, self.n_rows, k + 1, len(self.plan))
            acc = _stage(name, lambda: self.launch(
                rels, self.n_rows, wt[:, at:], self.N, root=self.root if with_root else None, bias=bias if last else None,
                relu=self.relu and last, acc_in=acc, out_rows=out_rows if last else None, out=out if last else None,
                kept=None if kept is None else kept[:, at:]))
        return acc


class _SageGroup(_HeteroGroup):
    """The hetero SAGE layer's group: per relation block ``(row_ptr, col, x, ids, mean, src)`` (``src``: index of x among the
    group's differentiable source tensors, None for a table read through a node list)."""
    stage = "sage"

    def __init__(self, blocks, hops, root, plan, n_rows, N, relu, tag):
        super().__init__(blocks, hops, root, plan, n_rows, N, relu, tag)
        self.col0 = [0]
        for b in blocks:
            self.col0.append(self.col0[-1] + int(b[2].shape[1]))
        self.K = self.col0[-1] + (int(root[0].shape[1]) if root is not None else 0)

    def launch(self, *args, kept=None, **kw):
        return hetero_sage_launch(*args, c_out=kept, **kw)

    def rels(self, lo, hi):
        return [(b[0], b[1], b[2], b[3], None, b[4]) for b in self.blocks[lo:hi]]

    def first_col(self, lo):
        return self.col0[lo]


def _relation_transpose(r: RelationHop, n_src: int, want_perm: bool = False):
    """``(row_ptr_t, col_t, scale | perm)`` of a relation hop with edges, seen from its ``n_src`` input rows (entries = the hop's
    frontier entries, hop order inside a source row: deterministic sums).  The third item is ``scale`` = 1 / degree of every
    frontier entry (a mean relation's factor), or with ``want_perm`` the hop's CSR edge of every transposed entry instead —
    computed once per form and kept on the ``RelationHop``."""
    cache = r.__dict__.setdefault("_transposed", {})
    hit = cache.get(want_perm)
    if hit is None or hit[0] != n_src:
        row_ptr_t, extra, _, col_t = _csr_transpose(r.row_ptr, r.col, n_src, want_perm=want_perm, want_col_t=True)
        if not want_perm:
            deg = (r.row_ptr[1:] - r.row_ptr[:-1]).clamp(min=1)
            extra = (1.0 / deg.float()).contiguous()
        hit = cache[want_perm] = (n_src, row_ptr_t, col_t, extra)
    return hit[1:]


class _HeteroSageGroup(torch.autograd.Function):
    """One (hop, destination type) group of the hetero SAGE layer under autograd.  Differentiable inputs: the stacked weight,
    the bias sum, the resident destination rows and the resident source tensors.  Forward: the group's launches in their
    ``_train`` form (C kept).  Backward: ``wgamd_gcn_wgrad_f32`` over column blocks of C (dW, db: deterministic split-K);
    the root's ``dX_dst[dst_rows] = dZ W_root`` (a library GEMM, rows distinct); per resident source type the layer kernel
    itself over the relations' transposes with dZ as the input rows and the relations' ``W_l`` transposed as the weight — no
    atomics anywhere: the same bits from run to run."""

    @staticmethod
    def forward(ctx, grp, wstack, bias, x_dst, *srcs):
        w, b = wstack.detach(), None if bias is None else bias.detach()
        c = _agg_pool.take((grp.n_rows, grp.K), torch.float32, w.device)
        z = grp.run(w, b, kept=c)
        ctx.grp, ctx.c, ctx.n_srcs = grp, c, len(srcs)
        ctx.src_shapes = [tuple(t.shape) for t in srcs]
        ctx.dst_shape = None if x_dst is None else tuple(x_dst.shape)
        ctx.save_for_backward(w, z)
        return z

    @staticmethod
    def backward(ctx, g):
        _released(ctx.c, "HeteroConv (SAGEConv relations)", "rows")
        grp, c = ctx.grp, ctx.c
        w, z = ctx.saved_tensors
        N, K = grp.N, grp.K
        g = g.contiguous().float()
        if grp.relu:
            g = torch.ops.aten.threshold_backward(g, z, 0)          # dZ once, read by every gradient
        need_w, need_b, need_dst = ctx.needs_input_grad[1:4]
        gw = gb = gdst = None
        if need_w or need_b:
            gw = torch.empty((N, K), dtype=torch.float32, device=g.device)
            gb = torch.empty(N, dtype=torch.float32, device=g.device) if need_b else None
            for at in range(0, K, 256):
                blk = torch.empty((N, min(256, K - at)), dtype=torch.float32, device=g.device)
                gcn_wgrad(c[:, at:at + blk.shape[1]], g, blk, gb if at == 0 else None)
                gw[:, at:at + blk.shape[1]] = blk
            if not need_w:
                gw = None
        if need_dst and grp.root is not None:
            rows = grp.root[1]
            gdst = torch.zeros(ctx.dst_shape, dtype=torch.float32, device=g.device)
            gdst.index_copy_(0, rows, g @ w[:, grp.col0[-1]:])      # (rows of one group are distinct vertices)
        gsrcs = [None] * ctx.n_srcs
        for si in range(ctx.n_srcs):
            if not ctx.needs_input_grad[4 + si]:
                continue
            mine = [k for k, blk in enumerate(grp.blocks) if blk[5] == si and grp.hops[k] is not None and grp.hops[k].n_edges > 0]
            n_src, F_ = ctx.src_shapes[si]
            gx = None
            fits = N % 4 == 0 and F_ <= 256 and g.data_ptr() % 16 == 0
            per = max(1, min(L.HETERO_SAGE_MAX_RELATIONS, HETERO_SAGE_MAX_K // N))      # relations per launch: K = per N <= 1024
            while mine:
                now, mine = mine[:per], mine[per:]
                if fits:
                    rels = []
                    for k in now:
                        row_ptr_t, col_t, scale = _relation_transpose(grp.hops[k], n_src)
                        rels.append((row_ptr_t, col_t, g, None, scale if grp.blocks[k][4] else None, False))
                    wt = torch.cat([w[:, grp.col0[k]:grp.col0[k + 1]].t() for k in now], 1).contiguous()
                    gx = _stage("sage%s dX" % grp.tag, lambda: hetero_sage_launch(rels, n_src, wt, F_, acc_in=gx))
                else:
                    for k in now:
                        part = spmm_csr_backward(grp.blocks[k][0], grp.blocks[k][1], g @ w[:, grp.col0[k]:grp.col0[k + 1]], n_src,
                                                 mean=grp.blocks[k][4])
                        gx = part if gx is None else gx.add_(part)
            gsrcs[si] = gx if gx is not None else torch.zeros((n_src, F_), dtype=torch.float32, device=g.device)
        ctx.c = None
        return (None, gw, gb, gdst) + tuple(gsrcs)


# ---- heterogeneous transformer layer: one launch per (hop, destination type) — csrc/wg_transformer_hetero.hip ------------------
HETERO_TRANSFORMER_MAX_K = 1024   # floats of one launch's A row (the 16 x (K + 4) fp32 LDS tile of wg_transformer_hetero.hip)
hetero_transformer_launches = 0   # wgamd_hetero_transformer_layer_f32(_train) launches so far (tests: the kernel route ran)


def hetero_transformer_stack(convs):
    """The parameters of the ``TransformerConv`` relations ``convs`` ending in ONE node type, stacked the way
    ``wgamd_hetero_transformer_layer_f32`` reads them (torch ops in the parameters' dtype, under autograd when it is on):
      ``(wt [N, K], bias [N] | None, fold [F_dst, T], fold_bias [T], layout)``
    ``wt = [wt_r1[:, :H W4] | wt_r2[:, :H W4] | ... | sum_r lin_skip_r.weight]`` (``transformer_folds`` per relation; the skip
    block and ``bias`` = the sum of the skip biases cover the relations with ``root_weight``, and are absent when none has
    it), ``fold = [Fu_r1 | Fu_r2 | ... | Fw_r1 | ... | 0 pad]`` so that ``x_dst @ fold + fold_bias`` holds every relation's
    ``u`` and ``w`` as column slices (T a multiple of 4: rows stay 16-B aligned), and ``layout[r] = dict(col0, width, W4, u0,
    w0, H, F, D)``: the relation's columns of ``wt`` and of the fold product (``w0`` None without ``edge_dim``)."""
    N = {c._out_width for c in convs}
    Fd = {c.in_dst for c in convs}
    if len(N) != 1 or len(Fd) != 1:
        raise ValueError("HeteroConv: the TransformerConv relations ending in one node type must agree on the output width "
                         "(heads x out_channels, or out_channels with concat=False) and on in_channels[1]; got widths %s, "
                         "destination widths %s" % (sorted(N), sorted(Fd)))
    folds = [transformer_folds(c) for c in convs]
    layout, wts, at, ut = [], [], 0, 0
    for c, (Fu, bu, Fw, bw, wt, _) in zip(convs, folds):
        D = c.edge_dim or 0
        W4 = transformer_block_width(c.in_src, D)
        layout.append(dict(col0=at, width=c.heads * W4, W4=W4, u0=ut, w0=None, H=c.heads, F=c.in_src, D=D))
        wts.append(wt[:, :c.heads * W4])
        at += c.heads * W4
        ut += c.heads * c.in_src
    us, ub = [f[0] for f in folds], [f[1] for f in folds]
    for c, lay, f in zip(convs, layout, folds):
        if lay["D"]:
            lay["w0"] = ut
            us.append(f[2])
            ub.append(f[3])
            ut += c.heads * lay["D"]
    if ut % 4:
        us.append(us[0].new_zeros((us[0].shape[0], 4 - ut % 4)))
        ub.append(ub[0].new_zeros(4 - ut % 4))
    skips = [c.lin_skip for c in convs if c.root_weight]
    bias = None
    if skips:
        wts.append(_sum_of([l.weight for l in skips]))
        bias = _sum_of([l.bias for l in skips if l.bias is not None])
    return torch.cat(wts, 1), bias, torch.cat(us, 1), torch.cat(ub), layout


def hetero_transformer_launch(rels, n_rows: int, wt, N: int, root=None, bias=None, relu=False, acc_in=None, out_rows=None,
                              out=None, a_save=None):
    """One ``wgamd_hetero_transformer_layer_f32`` launch (include/wgamd_ext.h).  ``rels``: ``[(row_ptr, col, x, ids, edge_attr,
    u, w, H, alpha), ...]`` (x [*, F] float32 rows, ``ids`` the node list x is read through or None, ``edge_attr`` [E, D] in
    CSR order or None, ``u`` [n_rows, H F] / ``w`` [n_rows, H D] column slices of the fold product, ``alpha`` [E, H] or None);
    ``root``: ``(x_dst, dst_rows, dst_ids)`` or None; ``wt`` [N, >= K] (a column slice of the stacked weight); ``a_save``
    [n_rows, >= K]: the launch also keeps its A rows, and every relation its alpha (``_train``)."""
    global hetero_transformer_launches
    arr = (L.HeteroTransformerRelation * max(len(rels), 1))()
    keep, at = [], 0
    for k, (row_ptr, col, x, ids, ea, u, w, H, alpha) in enumerate(rels):
        _check_csr(row_ptr, col)
        F_, D = int(x.shape[1]), 0 if ea is None else int(ea.shape[1])
        assert row_ptr.shape[0] == n_rows + 1 and x.dtype == torch.float32 and x.stride(1) == 1
        assert ids is None or ids.is_contiguous()
        assert u.dtype == torch.float32 and u.stride(1) == 1 and u.shape == (n_rows, H * F_)
        assert ea is None or (ea.dtype == torch.float32 and ea.is_contiguous() and ea.shape[0] == col.shape[0])
        assert (w is None) == (ea is None) and (w is None or (w.dtype == torch.float32 and w.stride(1) == 1 and w.shape == (n_rows, H * D)))
        assert alpha is None or (alpha.dtype == torch.float32 and alpha.is_contiguous() and alpha.shape == (col.shape[0], H))
        assert a_save is None or alpha is not None
        col = _nonempty(col, torch.int32)
        bufs = [col] + [None if t is None else _nonempty(t, torch.float32) for t in (ea, alpha)]
        keep.append(bufs)
        d = arr[k]
        d.row_ptr, d.col, d.x, d.ldx, d.src_ids = row_ptr.data_ptr(), col.data_ptr(), x.data_ptr(), x.stride(0), _ptr(ids)
        d.edge_attr, d.u, d.ldu, d.w, d.ldw = _ptr(bufs[1]), u.data_ptr(), u.stride(0), _ptr(w), 0 if w is None else w.stride(0)
        d.alpha, d.F, d.ids_kind, d.D, d.H, d.col0 = _ptr(bufs[2]), F_, _sage_ids_kind(ids), D, int(H), at
        at += int(H) * transformer_block_width(F_, D)
    assert a_save is None or a_save.dtype == torch.float32
    out = _hetero_launch_tail("wgamd_hetero_transformer_layer_f32", L.HETERO_TRANSFORMER_RELU, arr, len(rels), at, n_rows, wt, N, root,
                              bias, relu, acc_in, out_rows, out, a_save)
    hetero_transformer_launches += 1
    return out


class _TconvGroup(_HeteroGroup):
    """The hetero transformer layer's group: per relation block a dict ``(row_ptr, col, x, ids, ea, src, n_edges)`` (``ea``: the
    hop's rows of the relation's edge attributes or None; ``src``: index of x among the group's differentiable source tensors,
    None for a table read through a node list) next to the relation's ``layout`` entry of ``hetero_transformer_stack``."""
    stage = "tconv"

    def __init__(self, blocks, layout, hops, root, plan, n_rows, N, relu, tag):
        super().__init__(blocks, hops, root, plan, n_rows, N, relu, tag)
        self.layout = layout
        self.K_rel = layout[-1]["col0"] + layout[-1]["width"] if layout else 0
        self.K = self.K_rel + (int(root[0].shape[1]) if root is not None else 0)

    def u_w(self, uw, k):
        lay = self.layout[k]
        u = uw[:, lay["u0"]:lay["u0"] + lay["H"] * lay["F"]]
        return u, (uw[:, lay["w0"]:lay["w0"] + lay["H"] * lay["D"]] if lay["D"] else None)

    def launch(self, *args, kept=None, **kw):
        return hetero_transformer_launch(*args, a_save=kept, **kw)

    def rels(self, lo, hi, uw, alphas=None):
        """``uw``: the fold product; ``alphas``: every block's alpha buffer (training) or None."""
        return [(blk["row_ptr"], blk["col"], blk["x"], blk["ids"], blk["ea"], *self.u_w(uw, b), self.layout[b]["H"],
                 None if alphas is None else alphas[b]) for b, blk in enumerate(self.blocks[lo:hi], lo)]

    def first_col(self, lo):
        return self.layout[lo]["col0"] if lo < len(self.layout) else self.K_rel


class _HeteroTconvGroup(torch.autograd.Function):
    """One (hop, destination type) group of the hetero transformer layer under autograd.  Differentiable inputs: the stacked
    weight, the bias sum, the fold product ``uw`` (every relation's u and w: their gradients reach the query folds and the
    destination rows through autograd over the GEMM that made it), the resident destination rows (the skip block) and the
    resident source tensors.  Forward: the group's launches in their ``_train`` form (A [n, K] and every relation's alpha
    kept).  Backward: ``gwt = gz^T A`` and ``dA = gz wt`` (library GEMMs); per relation ``wgamd_transformer_bwd_dst_f32`` on
    the column slices of dA and A at the relation's col0 (du, dw, ds) and, per resident source tensor,
    ``wgamd_transformer_bwd_src_f32`` over the relation hop's transpose; the skip block's ``dA[:, K_rel:]`` goes to the
    destination rows through ``dst_rows`` (rows of one group are distinct vertices) — no atomics: the same bits every run."""

    @staticmethod
    def forward(ctx, grp, wt, bias, uw, x_dst, *srcs):
        w, b, uw_d = wt.detach().contiguous(), None if bias is None else bias.detach(), uw.detach()
        dev = w.device
        A = torch.empty((grp.n_rows, grp.K), dtype=torch.float32, device=dev)
        alphas = [torch.empty((blk["n_edges"], lay["H"]), dtype=torch.float32, device=dev) for blk, lay in zip(grp.blocks, grp.layout)]
        z = grp.run(w, b, uw_d, alphas, kept=A)
        ctx.grp, ctx.A, ctx.alphas, ctx.n_srcs = grp, A, alphas, len(srcs)
        ctx.src_shapes = [tuple(t.shape) for t in srcs]
        ctx.dst_shape = None if x_dst is None else tuple(x_dst.shape)
        ctx.save_for_backward(w, uw_d, z)
        return z

    @staticmethod
    def backward(ctx, g):
        _released(ctx.A, "HeteroConv (TransformerConv relations)", "rows")
        grp, A, alphas = ctx.grp, ctx.A, ctx.alphas
        w, uw, z = ctx.saved_tensors
        n, dev = grp.n_rows, w.device
        g = g.contiguous().float()
        if grp.relu:
            g = torch.ops.aten.threshold_backward(g, z, 0)          # dZ once, read by every gradient
        need_w, need_b, need_uw, need_dst = ctx.needs_input_grad[1:5]
        need_src = [ctx.needs_input_grad[5 + si] for si in range(ctx.n_srcs)]
        gw = g.t() @ A if need_w else None
        gb = g.sum(0) if need_b else None
        guw = gdst = None
        gsrcs = [None] * ctx.n_srcs
        if need_uw or need_dst or any(need_src):
            dA = (g @ w).contiguous()                                # [n, K]
            guw = torch.zeros_like(uw)
            for si in range(ctx.n_srcs):
                if need_src[si]:
                    gsrcs[si] = torch.zeros(ctx.src_shapes[si], dtype=torch.float32, device=dev)
            for k, (blk, lay) in enumerate(zip(grp.blocks, grp.layout)):
                if blk["n_edges"] == 0:
                    continue
                H, F_, D, c0 = lay["H"], lay["F"], lay["D"], lay["col0"]
                du = torch.empty((n, H * F_), dtype=torch.float32, device=dev)
                dw = torch.empty((n, H * D), dtype=torch.float32, device=dev) if D else None
                ds = torch.empty((blk["n_edges"], H), dtype=torch.float32, device=dev)
                transformer_bwd_dst(blk["row_ptr"], blk["col"], blk["x"], H, alphas[k], dA[:, c0:], A[:, c0:], du, ds,
                                    edge_attr=blk["ea"], dw=dw, src_ids=blk["ids"])
                guw[:, lay["u0"]:lay["u0"] + H * F_] = du
                if D:
                    guw[:, lay["w0"]:lay["w0"] + H * D] = dw
                si = blk["src"]
                if si is not None and need_src[si]:
                    row_ptr_t, col_t, perm = _relation_transpose(grp.hops[k], ctx.src_shapes[si][0], want_perm=True)
                    transformer_bwd_src(row_ptr_t, col_t, perm, None, D, H, -1, alphas[k], ds, dA[:, c0:], grp.u_w(uw, k)[0], gsrcs[si])
            if need_dst and grp.root is not None:
                gdst = torch.zeros(ctx.dst_shape, dtype=torch.float32, device=dev)
                gdst.index_copy_(0, grp.root[1], dA[:, grp.K_rel:])  # (rows of one group are distinct vertices)
            if not need_uw:
                guw = None
        ctx.A = ctx.alphas = None
        return (None, gw, gb, guw, gdst) + tuple(gsrcs)


class HeteroConv(torch.nn.Module):
    """``torch_geometric.nn.HeteroConv({edge_type: conv}, aggr="sum")`` for ``GATConv`` relations, or for ``SAGEConv``
    relations: the output of a node type is the sum over the relations ending in it (examples/mag_lp_mnmg.py:141 builds this
    stack; GATConv as pylibwholegraph/torch/gnn_model.py:45-59; bipartite SAGEConv per direction as movielens_mnmg.py).

    ``forward(x_dict, graph, act=None, edge_attr_dict=None)``
      * ``graph`` a ``HeteroLayerGraph`` of a loader call group (no autograd): every (hop, edge type) is ONE launch —
        AGGREGATE-FIRST (the attention-weighted sum is linear, so it runs over the UNTRANSFORMED source rows and the per-head
        weights are applied to the few destination rows afterwards: the ``lin`` GEMM over every source row, 10-20x more rows,
        never runs), attention logits ``x @ fold(W, att)`` made by the feature gather itself when ``x_dict[t]`` is a
        ``LazyRows`` (``wgamd_gather_terms_f32``), HeteroConv's running sum, bias, ReLU and the row placement folded into the
        last relation's launch (``wgamd_gat_layer_fused_bf16x3`` / ``wgamd_gat_transform_heads_bf16x3``).  With ``SAGEConv``
        relations (autograd too) every (hop, destination type) is ONE launch: ``_forward_layer_sage``; with ``TransformerConv``
        relations likewise (``_forward_layer_tconv``, the to_hetero'd encoder of mag_lp_mnmg.py:53-66), ``edge_attr_dict[et]``
        = the edge type's attributes [edges of et in the call group, edge_dim], hop-major (``HeteroCallGroup.edge_attr``):
        every layer takes the same dict and reads the prefix of the hops it runs (``RelationHop.edge_base``).
      * ``graph`` a dict ``{edge_type: edge_index | [csr_row_ptr, csr_col_ind]}`` (a mini-batch ``HeteroData``; autograd):
        ``convs[edge_type]((x_src, x_dst), graph[edge_type])`` summed per destination type — PyG's own formulation; a
        ``TransformerConv`` relation with ``edge_dim`` takes ``edge_attr_dict[edge_type]`` as its ``edge_attr``.
    A relation with ``edge_dim`` and no entry in ``edge_attr_dict`` raises ValueError before any launch."""

    def __init__(self, convs, aggr: str = "sum"):
        super().__init__()
        assert aggr in ("sum", "add"), "aggr: sum"
        self.edge_types = sorted(convs)
        self.convs = torch.nn.ModuleDict({"__".join(et): convs[et] for et in self.edge_types})
        self._wgamd_derived = {}       # (``_derived``'s store, here from the start: a forward adds no attribute to the module)
        self.stage_tag = ""        # suffix of this layer's stage names under set_stage_hook ("1": gat1:..., transform1, ...)
        # the one-kernel relation keeps 10 neighbours of a row in registers and continues longer rows one neighbour at a time:
        # hops with a larger fan-out take the two-kernel path (the fan-out-25 hop of the mag workload through the one-kernel
        # relation: 0.77 ms instead of 0.39 + 0.16 per call group)
        self.fused_max_fanout = 10
        # a LazyRows input (table + node list) stays lazy: its attention terms come from one read-only pass over the listed rows
        # and every relation kernel reads the table through the list — the [n, F] copy of the rows is never written
        self.fetch_in_layer = True
        # under autograd a call-group layer is aggregate-first too (``_forward_layer_train``); False: PyG's own relation-by-relation,
        # transform-first formulation on ``GATConv`` (``_forward_relations``: the lin GEMM over every source row)
        self.train_aggregate_first = True
        # TransformerConv relations over a call group: True runs the library-ops route (``_forward_tconv_library``) whatever the
        # shapes — the comparison route of examples/hetero_transformer_call_groups.py --torch-ops
        self.transformer_library_ops = False

    def conv(self, edge_type):
        return self.convs["__".join(edge_type)]

    # ---- parameters in the form the kernels read (``_derived``, kept on the module) --------------------------------------
    def _rel(self, et):
        """(w [in, H C] contiguous, fold(w, att_src) [in, H], fold(w, att_dst) [in, H]) of a relation, rebuilt when a parameter
        changed: ``alpha_src = ((x W).view(H, C) * att).sum(-1) = x (W . att)``."""
        c = self.conv(et)

        def build():
            w = c.lin.weight.t().contiguous()
            w3 = w.view(w.shape[0], c.heads, c.out_channels)
            return (w, (w3 * c.att_src.view(1, c.heads, c.out_channels)).sum(-1).contiguous(),
                    (w3 * c.att_dst.view(1, c.heads, c.out_channels)).sum(-1).contiguous())
        return _derived(self, ("rel", et), (c.lin.weight, c.att_src, c.att_dst), build)

    def _term_keys(self, t):
        keys = []
        for et in self.edge_types:
            if et[0] == t:
                keys.append(("src", et))
            if et[2] == t:
                keys.append(("dst", et))
        return keys

    def _terms_matrix(self, t):
        """[in, H x relation ends of node type t]: the folded attention vectors of every relation end reading type t."""
        ends = self._term_keys(t)
        convs = [self.conv(et) for et in self.edge_types if t in (et[0], et[2])]

        def build():
            mats = [self._rel(et)[1 if end == "src" else 2] for end, et in ends]
            return torch.cat(mats, 1).contiguous() if mats else None
        return _derived(self, ("terms", t), [p for c in convs for p in (c.lin.weight, c.att_src, c.att_dst)], build)

    def _bias(self, dt):
        """Sum of the biases of the relations ending in ``dt`` (HeteroConv adds the relations' outputs, bias included)."""
        rels = [et for et in self.edge_types if et[2] == dt]
        if rels and all(isinstance(self.conv(et), SAGEConv) for et in rels):
            return self._sage_weights(dt)[1]
        bs = [self.conv(et).bias for et in rels if self.conv(et).bias is not None]
        return _derived(self, ("bias", dt), bs, lambda: _sum_of(bs))

    # ---- call-group layer ----------------------------------------------------------------------------------------------
    def _attention_terms(self, xs, graph):
        """-> (x tensors, a_src{et}, a_dst{et}, by_id): ``x_t @ [fold(W_r, att_src) | fold(W_r, att_dst) ...]`` in ONE pass over
        the rows of every node type — inside the row gather for a ``LazyRows`` input, a streaming pass over a resident one.
        ``by_id``: the node types whose terms are those of the TABLE's rows (``_terms_by_id``)."""
        from .tensor import local_gather
        x, a_src, a_dst, by_id = {}, {}, {}, set()
        for t in graph.node_types:
            v = xs.get(t)
            if v is None:
                continue
            keys = [(a_src if end == "src" else a_dst, et) for end, et in self._term_keys(t)]
            vt = self._terms_matrix(t)
            H = self.conv(keys[0][1]).heads if keys else 0
            slabs = None
            if isinstance(v, LazyRows):
                n, F_ = len(v), v.table.shape[1]
                terms_ok = vt is not None and n > 0 and H == 4 and v.table.dtype == torch.float32 and gather_terms_supported(F_, vt.shape[1])
                if self.fetch_in_layer and terms_ok and _table_through_ids(v) is not None:
                    x[t] = v
                    if _terms_by_id(v.table.shape[0], n):
                        slabs = _stage("attn_terms(table)" + self.stage_tag, lambda: rows_terms(v.table, vt, heads=4))
                        by_id.add(t)
                    else:
                        slabs = _stage("attn_terms(lazy)" + self.stage_tag, lambda: lazy_rows_terms(v.table, v.ids, vt, heads=4))
                    for k, (dst, et) in enumerate(keys):
                        dst[et] = slabs[k]
                    continue
                buf = torch.empty((n, F_), dtype=torch.float32, device=v.table.device)
                if terms_ok:
                    x[t], slabs = _stage("gather+attn_terms" + self.stage_tag, lambda: gather_with_terms(v.table, v.ids, vt, out=buf, heads=4))
                else:
                    x[t] = _stage("gather", lambda: local_gather(v.table, v.ids, buf))
            else:
                x[t] = v
            if not keys or x[t].shape[0] == 0:
                continue
            if slabs is None:
                xt = x[t]
                if H == 4 and _kernel_rows_ok(xt) and gather_terms_supported(int(xt.shape[1]), int(vt.shape[1])):
                    slabs = _stage("attn_terms" + self.stage_tag, lambda: rows_terms(xt, vt, heads=4))
                else:
                    both = _stage("attn_terms" + self.stage_tag, lambda: xt @ vt)
                    slabs = both.view(both.shape[0], len(keys), H).permute(1, 0, 2).contiguous()
            for k, (dst, et) in enumerate(keys):
                dst[et] = slabs[k]
        return x, a_src, a_dst, by_id

    def _forward_layer(self, xs, graph: HeteroLayerGraph, act=None):
        assert act in (None, "relu")
        relu = act == "relu"
        x, a_src, a_dst, by_id = self._attention_terms(xs, graph)
        dev = next(iter(x.values())).device
        groups, listed = _relation_groups(graph), set()
        out = _group_outputs(graph, groups, self._width, dev)
        for (hop, dt), mine in groups:
            n_f, HC = mine[0].n_rows, self._width(dt)
            if n_f == 0:
                continue
            bias, place = self._bias(dt), mine[0].out_rows
            live = [r for r in mine if r.n_edges > 0]      # (a relation that sampled nothing adds nothing to the sum)
            acc = torch.empty((n_f, HC), dtype=torch.float32, device=dev)
            c0 = self.conv(mine[0].edge_type)
            H, C = c0.heads, c0.out_channels
            one_pass = bool(live) and all(
                gat_transform_supported(x[r.edge_type[0]].shape[1], H, C) for r in live)
            target = out[dt] if place is not None else None
            if one_pass and place is None:
                out[dt] = target = torch.empty((n_f, HC), dtype=torch.float32, device=dev)
            for j, r in enumerate(live):
                et = r.edge_type
                w = self._rel(et)[0]
                xsrc, last = x[et[0]], j == len(live) - 1
                ids, through = None, {}
                if isinstance(xsrc, LazyRows):      # fetch in the layer: the kernels read the table through the node list
                    xsrc, ids = xsrc.table, xsrc.ids
                    through = dict(src_ids=ids, src_terms_by_id=et[0] in by_id)
                    if et[2] in by_id:
                        through.update(dst_ids=x[et[2]].ids, dst_terms_by_id=True)
                elif et[2] in by_id and et not in listed:
                    # (terms of the destination TABLE's rows next to a resident source: per-list terms, made once per edge type —
                    #  the relation runs in several hops)
                    a_dst[et] = gather_term_slabs(a_dst[et].unsqueeze(0), x[et[2]].ids)[0]
                    listed.add(et)
                tail = dict(acc_in=acc if j > 0 else None, bias=bias if (last and one_pass) else None, relu=last and one_pass and relu,
                            out_rows=place if (last and one_pass) else None, out=target if (last and one_pass) else acc)
                name = "%s hop %d (%d rows, %d edges)" % (et[1], hop + 1, n_f, r.n_edges)
                if one_pass and r.fanout <= self.fused_max_fanout and gat_layer_fused_supported(xsrc.shape[1], H, C):
                    # deep hop (fan-out <= 10): aggregation + dense tail as ONE kernel, the aggregate stays in LDS
                    _stage("gat%s+transform:" % self.stage_tag + name, lambda: gat_layer_fused(r.row_ptr, r.col, xsrc, a_src[et], a_dst[et], w, H,
                                                                            dst_rows=r.dst_rows, **through, **tail))
                    continue
                agg = _stage("gat%s:" % self.stage_tag + name, lambda: gat_aggregate_heads(r.row_ptr, r.col, xsrc, a_src[et], a_dst[et], H,
                                                                       dst_rows=r.dst_rows, **through))
                if one_pass:
                    _stage("transform" + self.stage_tag, lambda: gat_transform_heads_fused(agg, w, H, **tail))
                else:
                    _stage("transform" + self.stage_tag, lambda: gat_transform_heads(agg, w, H, out=acc, overwrite=j == 0))
            if one_pass:
                continue
            if not live:
                acc.zero_()        # no relation of this type sampled an edge in this hop: act(bias) rows
            if place is not None:
                _stage("bias_act", lambda: bias_act_rows(acc, bias, relu, place, out[dt]))
            else:
                out[dt] = _stage("bias_act", lambda: bias_act_rows(acc, bias, relu))
        return out

    def _width(self, dt):
        c = next(self.conv(et) for et in self.edge_types if et[2] == dt)
        return c.heads * c.out_channels if getattr(c, "concat", False) else c.out_channels

    def forward(self, x_dict, graph, act=None, edge_attr_dict=None):
        # (folded attention vectors, weight tiles, pooled buffers: cached against the parameters' versions)
        _refuse_capture(self, "derived-weight caches")
        if isinstance(graph, HeteroLayerGraph):
            sage = [isinstance(self.conv(et), SAGEConv) for et in self.edge_types]
            if all(sage):
                return self._forward_layer_sage(x_dict, graph, act)
            tconv = [isinstance(self.conv(et), TransformerConv) for et in self.edge_types]
            if all(tconv):
                return self._forward_layer_tconv(x_dict, graph, act, edge_attr_dict)
            if any(sage) or any(tconv) or not all(isinstance(self.conv(et), GATConv) for et in self.edge_types):
                raise NotImplementedError("HeteroConv over a HeteroLayerGraph: every relation a GATConv, every relation a "
                                          "SAGEConv, or every relation a TransformerConv (mixed layer classes run over a dict "
                                          "of edge_index only)")
            needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            plain = all(self.conv(et).concat and not self.conv(et).add_self_loops for et in self.edge_types)
            if not needs_grad and plain:
                return self._forward_layer(x_dict, graph, act)
            if plain and self.train_aggregate_first and all(
                    self.conv(et).heads in (1, 2, 4, 8) and self.conv(et).lin.weight.shape[1] % 4 == 0
                    and self.conv(et).lin.weight.shape[1] <= 256 for et in self.edge_types):
                return self._forward_layer_train(x_dict, graph, act)
            return self._forward_relations(x_dict, graph, act)
        out = {}
        live = [et for et in self.edge_types if et in graph and x_dict.get(et[0]) is not None and x_dict.get(et[2]) is not None]
        attrs = {}
        for et in live:       # (a TransformerConv relation takes its edge attributes: checked before any launch)
            c = self.conv(et)
            if isinstance(c, TransformerConv) and c.edge_dim is not None:
                if edge_attr_dict is None or edge_attr_dict.get(et) is None:
                    raise ValueError("HeteroConv: TransformerConv of %r has edge_dim=%d and edge_attr_dict has no entry for it"
                                     % (et, c.edge_dim))
                attrs[et] = dict(edge_attr=c._check_edge_attr(edge_attr_dict[et], graph[et][1].shape[0], graph[et][0].device))
        for et in live:
            y = self.conv(et)((x_dict[et[0]], x_dict[et[2]]), graph[et], **attrs.get(et, {}))
            out[et[2]] = y if et[2] not in out else out[et[2]] + y
        return {t: torch.relu(v) for t, v in out.items()} if act == "relu" else out

    # ---- what the one-launch routes (_forward_layer_sage, _forward_layer_tconv) share -------------------------------------
    @staticmethod
    def _relu_of(act) -> bool:
        if act not in (None, "relu"):
            raise ValueError("HeteroConv: act is None or 'relu', not %r" % (act,))
        return act == "relu"

    @staticmethod
    def _source_slot(srcs, x, ids):
        """Index of ``x`` among the group's differentiable source tensors ``srcs`` (appended when new); None for a table read
        through a node list ``ids``."""
        if ids is not None:
            return None
        si = next((k for k, t in enumerate(srcs) if t is x), None)
        if si is None:
            srcs.append(x)
            si = len(srcs) - 1
        return si

    @staticmethod
    def _run_group(out, dt, grp, *, fn, place, needs_grad, args, srcs):
        """The group's rows into ``out[dt]``: under autograd ``fn.apply(grp, *args, root_src, *srcs)`` (``root_src``: the
        root's rows when they are resident) placed by ``_place_rows``, otherwise the group's launches ``grp.run(*args)``, the
        last one writing ``out[dt]`` through ``place`` itself."""
        if needs_grad:
            root_src = grp.root[0] if grp.root is not None and grp.root[2] is None else None
            _place_rows(out, dt, fn.apply(grp, *args, root_src, *srcs), place)
        elif place is None:
            out[dt] = grp.run(*args)
        else:
            grp.run(*args, out=out[dt], out_rows=place)

    # ---- SAGEConv relations: one launch per (hop, destination type) -----------------------------------------------------
    def _sage_weights(self, dt, grad: bool = False):
        """``(Wstack [N, K], bias sum [N] | None)`` of destination type ``dt``: ``[W_l^r1 | W_l^r2 | ... | sum_r W_r^r]`` over the
        relations ending in it (sorted edge types; the root block is absent when no relation has a root weight).  ``grad``:
        built by torch ops on the parameters (autograd hands each relation its slice and every ``lin_r`` the shared root
        gradient); otherwise detached and kept (``_derived``)."""
        convs = [self.conv(et) for et in self.edge_types if et[2] == dt]

        def build():
            root = _sum_of([c.lin_r.weight for c in convs if c.lin_r is not None])
            wstack = torch.cat([c.lin_l.weight for c in convs] + ([] if root is None else [root]), 1)
            return wstack, _sum_of([c.lin_l.bias for c in convs if c.lin_l.bias is not None])
        return _derived(self, ("sage", dt), [p for c in convs for p in c.parameters()], build, grad=grad)

    def _forward_layer_sage(self, xs, graph: HeteroLayerGraph, act=None):
        """``HeteroConv({edge_type: SAGEConv})`` over a call group's layer graph: per (hop, destination type) the sum over the
        relations ending in the type is ONE product ``[mean_r1 | mean_r2 | ... | x_dst] @ [W_l^r1 | W_l^r2 | ... | sum W_r]^T``
        — one ``wgamd_hetero_sage_layer_f32`` launch (a group wider than 1024 floats: consecutive launches of whole relations,
        ``hetero_sage_plan``), bias, ReLU and row placement folded in.  A ``LazyRows`` input (int64 ids, fp32 table, 16-B rows)
        is read through its node list, per node type.  Under autograd one ``_HeteroSageGroup`` per group.  Shapes outside the
        kernel's domain: ``_forward_sage_library``."""
        relu = self._relu_of(act)
        X, ids = {}, {}
        for t, v in xs.items():
            if v is None:
                continue
            lazy = _table_through_ids(v)
            if isinstance(v, LazyRows):
                _refuse_lazy_table_grad(v.table)
            if lazy is not None:
                X[t], ids[t] = lazy
            else:
                X[t], ids[t] = (v.materialize() if isinstance(v, LazyRows) else v), None
        convs = [self.conv(et) for et in self.edge_types]
        in_domain = all(c.aggr in ("mean", "sum", "add") and c.out_channels <= 256 for c in convs) and all(
            _kernel_rows_ok(v) and v.shape[1] % 4 == 0 and v.shape[1] <= HETERO_SAGE_MAX_K for v in X.values())
        if not in_domain:
            return self._forward_sage_library({t: (v.materialize() if isinstance(v, LazyRows) else v) for t, v in xs.items()
                                               if v is not None}, graph, relu)
        needs_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                                  or any(ids[t] is None and v.requires_grad for t, v in X.items()))
        dev = next(iter(X.values())).device
        groups = _relation_groups(graph)
        out = _group_outputs(graph, groups, self._width, dev, make=torch.zeros if needs_grad else torch.empty)
        weights = {}
        for (hop, dt), mine in groups:
            n_f = mine[0].n_rows
            if n_f == 0:
                continue
            listed = {r.edge_type: r for r in mine}
            blocks, hops, srcs = [], [], []
            for et in self.edge_types:
                if et[2] != dt:
                    continue
                c, x, r = self.conv(et), X[et[0]], listed.get(et)
                if x.shape[1] != c.lin_l.weight.shape[1]:
                    raise ValueError("HeteroConv: x_dict[%r] has %d features, SAGEConv of %r takes %d"
                                     % (et[0], x.shape[1], et, c.lin_l.weight.shape[1]))
                si = self._source_slot(srcs, x, ids[et[0]])
                if r is None:       # the hop lists no such relation: its root term and bias still count
                    row_ptr, col = torch.zeros(n_f + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
                else:
                    row_ptr, col = r.row_ptr, r.col
                blocks.append((row_ptr, col, x, ids[et[0]], c.aggr == "mean", si))
                hops.append(r)
            root = None
            roots = [self.conv(et).lin_r for et in self.edge_types if et[2] == dt and self.conv(et).lin_r is not None]
            if roots:
                F_dst = roots[0].weight.shape[1]
                if X[dt].shape[1] != F_dst:
                    raise ValueError("HeteroConv: x_dict[%r] has %d features, the root weights take %d" % (dt, X[dt].shape[1], F_dst))
                root = (X[dt], mine[0].dst_rows, ids[dt])
            plan = hetero_sage_plan([b[2].shape[1] for b in blocks], 0 if root is None else root[0].shape[1])
            grp = _SageGroup(blocks, hops, root, plan, n_f, self._width(dt), relu, self.stage_tag + " hop %d %s" % (hop + 1, dt))
            if dt not in weights:
                weights[dt] = self._sage_weights(dt, grad=needs_grad)
            self._run_group(out, dt, grp, fn=_HeteroSageGroup, place=mine[0].out_rows, needs_grad=needs_grad, args=weights[dt],
                            srcs=srcs)
        return out

    # ---- TransformerConv relations: one launch per (hop, destination type) ----------------------------------------------
    def _tconv_weights(self, ets, grad: bool = False):
        """``hetero_transformer_stack`` of the relations ``ets`` (those ending in one node type whose source type has input
        rows) in float32.  ``grad``: built by torch ops on the parameters (autograd hands each relation its slice and every
        ``lin_skip`` the shared skip gradient); otherwise detached and kept (``_derived``)."""
        convs = [self.conv(et) for et in ets]

        def build():
            wt, bias, fold, fold_b, layout = hetero_transformer_stack(convs)
            return (wt.float().contiguous(), None if bias is None else bias.float(), fold.float().contiguous(), fold_b.float(), layout)
        return _derived(self, ("tconv", tuple(ets)), [p for c in convs for p in c.parameters()], build, grad=grad)

    def _tconv_edge_attrs(self, ets, graph: HeteroLayerGraph, edge_attr_dict, device):
        """{edge type: the edge type's hop-major edge attributes as the kernels read them (float32 [E, D] contiguous)} for the
        relations of ``ets`` with ``edge_dim``; ValueError on a missing entry, a wrong width, dtype, device or length (the
        call group's edge count of the type, ``graph.num_group_edges``; for a user-built graph the rows its hops cover) — before
        any launch.  NotImplementedError for an attribute that requires a gradient: edge attributes are data here."""
        out = {}
        for et in ets:
            c = self.conv(et)
            if c.edge_dim is None:
                continue
            if edge_attr_dict is None or edge_attr_dict.get(et) is None:
                raise ValueError("HeteroConv: TransformerConv of %r has edge_dim=%d and edge_attr_dict has no entry for it"
                                 % (et, c.edge_dim))
            total = None if graph.num_group_edges is None else graph.num_group_edges.get(et)
            if total is None:
                total = max([r.edge_base + r.n_edges for r in graph.relations if r.edge_type == et] + [0])
            ea = c._check_edge_attr(edge_attr_dict[et], int(total), device)
            if torch.is_grad_enabled() and ea.requires_grad:
                raise NotImplementedError("HeteroConv over a HeteroLayerGraph: a gradient w.r.t. edge_attr_dict[%r] is not "
                                          "supported (edge attributes are data here)" % (et,))
            out[et] = ea.detach().float().contiguous()
        return out

    def _forward_layer_tconv(self, xs, graph: HeteroLayerGraph, act=None, edge_attr_dict=None):
        """``HeteroConv({edge_type: TransformerConv})`` over a call group's layer graph: the softmax is per relation and the sum
        over the relations ending in a type is linear, so per (hop, destination type) the relations' rows ``[sum alpha [x_j |
        a_ij | 1] per head]`` sit side by side, followed by ``x_dst``, and meet ONE stacked weight ``[Wstack_r1 | Wstack_r2 |
        ... | sum_r lin_skip_r]`` — one ``wgamd_hetero_transformer_layer_f32`` launch (a group wider than 1024 floats:
        consecutive launches of whole relations, ``hetero_sage_plan``), bias, ReLU and row placement folded in; every
        relation's ``u`` and ``w`` are column slices of ONE library GEMM over the destination rows.  Every relation ending in
        the type whose source type has input rows adds its skip term to every row, whether or not the hop sampled an edge of
        it.  A ``LazyRows`` input (int64 or int32 ids, fp32 table, 16-B rows) is read through its node list, per node type.
        Under autograd one ``_HeteroTconvGroup`` per group.  Shapes outside the kernel's domain, and CPU tensors:
        ``_forward_tconv_library``."""
        relu = self._relu_of(act)
        for et in self.edge_types:
            c = self.conv(et)
            if c.dropout > 0 and c.training:
                raise NotImplementedError("TransformerConv: attention dropout (dropout > 0 in training mode) is not supported")
        X, ids = {}, {}
        for t, v in xs.items():
            if v is None:
                continue
            _refuse_featureless(self, v)
            if isinstance(v, LazyRows):
                _refuse_lazy_table_grad(v.table)
                if isinstance(v.table, torch.Tensor) and _kernel_rows_ok(v.table) and v._rows is None:
                    X[t], ids[t] = v.table, v.ids
                    continue
                v = v.materialize()
            X[t], ids[t] = v, None
        groups = _relation_groups(graph)
        ends = {}
        for (_, dt), mine in groups:
            if dt in ends:
                continue
            for r in mine:      # (a source type without input rows has no edges: its relation adds nothing)
                if (r.edge_type[0] not in X and r.n_edges > 0) or (dt not in X and r.n_rows > 0):
                    raise ValueError("HeteroConv: x_dict has no rows for %r, which relation %r needs" % (
                        dt if dt not in X else r.edge_type[0], r.edge_type))
            ends[dt] = [et for et in self.edge_types if et[2] == dt and et[0] in X]
            if not ends[dt]:
                raise ValueError("HeteroConv: x_dict has rows for no source type of the relations ending in %r" % (dt,))
            for et in ends[dt]:
                c = self.conv(et)
                if X[et[0]].shape[1] != c.in_src or X[dt].shape[1] != c.in_dst:
                    raise ValueError("HeteroConv: x_dict[%r] / x_dict[%r] have %d / %d features, TransformerConv of %r takes %s"
                                     % (et[0], dt, X[et[0]].shape[1], X[dt].shape[1], et, (c.in_src, c.in_dst)))
            if len({self.conv(et)._out_width for et in ends[dt]}) > 1:
                raise ValueError("HeteroConv: the TransformerConv relations ending in %r have output widths %s; they are summed, so "
                                 "they must agree" % (dt, sorted({self.conv(et)._out_width for et in ends[dt]})))
        dev = next(iter(X.values())).device
        used = [et for dt in ends for et in ends[dt]]
        eas = self._tconv_edge_attrs(used, graph, edge_attr_dict, graph.relations[0].row_ptr.device if graph.relations else dev)

        def fits(et):
            c = self.conv(et)
            one = (ctypes.c_int * 1)
            return bool(L.lib().wgamd_hetero_transformer_layer_supported(one(c.in_src), one(c.edge_dim or 0), one(c.heads), 1,
                                                                         c.in_dst if c.root_weight else 0, c._out_width))
        in_domain = not self.transformer_library_ops and all(torch.is_tensor(v) and v.is_cuda for v in X.values()) and all(
            fits(et) for et in used) and all(
            self.conv(et).in_dst % 4 == 0 and self.conv(et).in_dst <= 256 for et in used)
        if not in_domain:
            return self._forward_tconv_library({t: (v.materialize() if isinstance(v, LazyRows) else v) for t, v in xs.items()
                                                if v is not None}, graph, relu, eas)
        for t in X:       # rows as the kernel reads them (float32, unit column stride, 16-B aligned rows): copied when they are not
            if ids[t] is None:
                X[t] = _tconv_rows(X[t])
        needs_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                                  or any(ids[t] is None and v.requires_grad for t, v in X.items()))
        out = _group_outputs(graph, groups, self._width, dev, make=torch.zeros if needs_grad else torch.empty)
        weights = {}
        for (hop, dt), mine in groups:
            n_f = mine[0].n_rows
            if n_f == 0:
                continue
            listed = {r.edge_type: r for r in mine}
            if dt not in weights:
                weights[dt] = self._tconv_weights(ends[dt], grad=needs_grad)
            wt, bias, fold, fold_b, layout = weights[dt]
            dst_rows = mine[0].dst_rows
            # the queries: x_dst[dst_rows] (through the node list for a lazy type) times every relation's folds at once
            xq = X[dt][dst_rows] if ids[dt] is None else X[dt][ids[dt][dst_rows].long()]
            uw = torch.addmm(fold_b, xq, fold)
            blocks, hops, srcs = [], [], []
            for et in ends[dt]:
                x, r = X[et[0]], listed.get(et)
                si = self._source_slot(srcs, x, ids[et[0]])
                D = self.conv(et).edge_dim or 0
                if r is None or r.n_edges == 0:      # no edge of the relation in this hop: zero blocks, its skip term still counts
                    row_ptr = torch.zeros(n_f + 1, dtype=torch.int32, device=dev)
                    col, n_e = torch.zeros(0, dtype=torch.int32, device=dev), 0
                    ea = torch.zeros((0, D), dtype=torch.float32, device=dev) if D else None
                else:
                    row_ptr, col, n_e = r.row_ptr, r.col[:r.n_edges], r.n_edges
                    ea = eas[et][r.edge_base:r.edge_base + n_e] if D else None
                blocks.append(dict(row_ptr=row_ptr, col=col, x=x, ids=ids[et[0]], ea=ea, src=si, n_edges=n_e))
                hops.append(r)
            root = (X[dt], dst_rows, ids[dt]) if any(self.conv(et).root_weight for et in ends[dt]) else None
            plan = hetero_sage_plan([lay["width"] for lay in layout], 0 if root is None else root[0].shape[1],
                                    max_k=HETERO_TRANSFORMER_MAX_K, max_rel=L.HETERO_TRANSFORMER_MAX_RELATIONS)
            grp = _TconvGroup(blocks, layout, hops, root, plan, n_f, self._width(dt), relu, self.stage_tag + " hop %d %s" % (hop + 1, dt))
            self._run_group(out, dt, grp, fn=_HeteroTconvGroup, place=mine[0].out_rows, needs_grad=needs_grad, args=(wt, bias, uw),
                            srcs=srcs)
        return out

    def _forward_tconv_library(self, x, graph: HeteroLayerGraph, relu: bool, eas):
        """The same layer out of library ops in PyG's formulation (``_tconv_library_ops`` per relation hop, summed, activation
        applied, placed through ``out_rows``), with ordinary autograd — what shapes outside the kernel's domain and CPU tensors
        take; correctness only."""
        group = [None, None]       # the destination rows of the group being summed (``head``), made once per group

        def relation(et, r, head):
            if et[0] not in x:
                return None
            if group[0] is not head:
                group[:] = head, x[et[2]][head.dst_rows].float()
            c, xd = self.conv(et), group[1]
            if r is not None and r.n_edges > 0:
                ea = eas[et][r.edge_base:r.edge_base + r.n_edges] if c.edge_dim is not None else None
                one = LayerGraph([HopGraph(r.row_ptr, r.col[:r.n_edges], None)])
                return _tconv_library_ops(c, x[et[0]].float(), xd, one, ea, False)[0]
            return c.lin_skip(xd) if c.root_weight else None
        return self._library_groups(x, graph, relu, relation)

    def _library_groups(self, x, graph: HeteroLayerGraph, relu: bool, relation):
        """The frame of the two library routes: per (hop, destination type) the sum of ``relation(et, r, head)`` over the edge
        types ending in the type — the relation's rows or None; ``r`` = the hop's ``RelationHop`` of ``et`` or None, ``head`` = the
        group's first one (its ``n_rows``, ``dst_rows`` and ``out_rows`` are the group's) — zeros when none contributed, the
        activation applied, placed through ``out_rows`` in an output of the rows' dtype (not ``_group_outputs``)."""
        dev = next(iter(x.values())).device
        out = {}
        for (_, dt), mine in _relation_groups(graph):
            head = mine[0]
            if head.n_rows == 0:
                continue
            listed = {r.edge_type: r for r in mine}
            y = None
            for et in self.edge_types:
                o = relation(et, listed.get(et), head) if et[2] == dt else None
                if o is not None:
                    y = o if y is None else y + o
            if y is None:
                y = torch.zeros((head.n_rows, self._width(dt)), dtype=torch.float32, device=dev)
            if relu:
                y = torch.relu(y)
            if head.out_rows is not None and dt not in out:
                out[dt] = torch.zeros((graph.n_out[dt], y.shape[1]), dtype=y.dtype, device=dev)
            _place_rows(out, dt, y, head.out_rows)
        return out

    def _forward_sage_library(self, x, graph: HeteroLayerGraph, relu: bool):
        """The same layer out of library ops in PyG's formulation, relation by relation, with ordinary autograd — what shapes
        outside the kernel's domain (F % 4 != 0, N > 256, other dtypes, CPU tensors, other aggregators) take; correctness only."""
        dev = next(iter(x.values())).device

        def relation(et, r, head):
            c, xs, n_f = self.conv(et), x[et[0]], head.n_rows
            agg = torch.zeros((n_f, xs.shape[1]), dtype=xs.dtype, device=dev)
            if r is not None and r.n_edges > 0:
                if xs.is_cuda and xs.dtype == torch.float32 and c.aggr in ("mean", "sum", "add"):
                    agg = spmm_csr(xs, r.row_ptr, r.col, "mean" if c.aggr == "mean" else "sum")
                else:
                    deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
                    row = torch.repeat_interleave(torch.arange(n_f, device=dev), deg)
                    rows = xs[r.col.long()[:r.n_edges]]
                    if c.aggr in ("mean", "sum", "add"):
                        agg = agg.index_add(0, row, rows)
                        if c.aggr == "mean":
                            agg = agg / deg.clamp(min=1).unsqueeze(1).to(agg.dtype)
                    elif c.aggr in ("max", "min"):
                        agg = agg.scatter_reduce(0, row.unsqueeze(1).expand_as(rows), rows, "a" + c.aggr, include_self=False)
                    else:
                        raise NotImplementedError("HeteroConv: SAGEConv aggr %r (mean, sum, max, min)" % (c.aggr,))
            o = c.lin_l(agg)
            if c.lin_r is not None:
                o = o + c.lin_r(x[et[2]][head.dst_rows])
            return o
        return self._library_groups(x, graph, relu, relation)

    def _forward_layer_train(self, xs, graph: HeteroLayerGraph, act=None):
        """The call-group layer under autograd, AGGREGATE-FIRST like the inference route: per relation the attention-weighted
        sum of the UNTRANSFORMED source rows (``_GatAggregateHeads``: one kernel forward, one backward; a ``LazyRows`` input is
        read through its node list, its attention terms are those of the table's rows when the table is the shorter side), then
        the per-head weights on the few destination rows, HeteroConv's sum, bias, activation and row placement in torch — every
        parameter (lin weight, att_src, att_dst, bias) gets its gradient through ordinary autograd on top of the two kernels."""
        assert act in (None, "relu")
        X, ids, by_id, terms = {}, {}, {}, {}
        for t in graph.node_types:
            v = xs.get(t)
            if v is None:
                continue
            ends = self._term_keys(t)
            lazy = _table_through_ids(v)
            if lazy is not None:
                X[t], ids[t] = lazy
                by_id[t] = _terms_by_id(X[t].shape[0], len(v))
                rows = X[t] if by_id[t] else None
            else:
                X[t] = v.materialize() if isinstance(v, LazyRows) else v
                ids[t], by_id[t], rows = None, False, X[t]
            if not ends or len(v) == 0:
                continue
            folds = []
            for end, et in ends:          # differentiable folds: alpha = x (W . att)
                c = self.conv(et)
                w3 = c.lin.weight.t().reshape(c.lin.weight.shape[1], c.heads, c.out_channels)
                folds.append((w3 * (c.att_src if end == "src" else c.att_dst).view(1, c.heads, c.out_channels)).sum(-1))
            if rows is None:              # lazy, table longer than the list: terms of the listed rows
                rows = v.materialize()
            both = _NarrowTerms.apply(rows, torch.cat(folds, 1))
            H = self.conv(ends[0][1]).heads
            for k, (end, et) in enumerate(ends):
                terms[(end, et)] = both[:, k * H:(k + 1) * H]
        dev = next(iter(X.values())).device
        groups = _relation_groups(graph)
        out = _group_outputs(graph, groups, self._width, dev, make=torch.zeros)
        for (hop, dt), mine in groups:
            n_f = mine[0].n_rows
            if n_f == 0:
                continue
            acc = None
            for r in mine:
                if r.n_edges == 0:
                    continue
                et = r.edge_type
                c = self.conv(et)
                H, C = c.heads, c.out_channels
                st, dt_ = et[0], et[2]
                lazy_src = ids[st] is not None
                # (the kernel's id-list mode needs a lazy source; a resident source next to by-id destination terms reads them per row)
                a_dst = terms[("dst", et)]
                dst_by_id = bool(by_id[dt_]) and lazy_src
                if by_id[dt_] and not lazy_src:
                    a_dst = a_dst[ids[dt_]]
                agg = _GatAggregateHeads.apply(X[st], terms[("src", et)], a_dst, r.row_ptr, r.col, H, r.dst_rows,
                                               ids[st], ids[dt_] if dst_by_id else None, bool(by_id[st]) and lazy_src, dst_by_id,
                                               c.negative_slope)
                F_ = X[st].shape[1]
                w3 = c.lin.weight.t().reshape(F_, H, C)
                if acc is not None and acc.shape[1:] != (H, C):      # (relations of one destination type with different head shapes)
                    acc = (acc.reshape(n_f, H * C) + _heads_transform(agg.view(n_f, H, F_), w3).reshape(n_f, H * C)).view(n_f, H, C)
                else:
                    acc = _heads_transform(agg.view(n_f, H, F_), w3, acc)
            if acc is not None:
                acc = acc.reshape(n_f, -1)
            if acc is None:
                acc = torch.zeros((n_f, self._width(dt)), dtype=torch.float32, device=dev)
            # the relations' biases summed first: ONE pass over the rows (HeteroConv adds outputs, bias included)
            bias = _sum_of([self.conv(r.edge_type).bias for r in mine if self.conv(r.edge_type).bias is not None])
            if bias is not None:
                acc = acc + bias
            if act == "relu":
                acc = torch.relu(acc)
            _place_rows(out, dt, acc, mine[0].out_rows)
        return out

    def _forward_relations(self, xs, graph: HeteroLayerGraph, act=None):
        """The same layer relation by relation through ``GATConv`` (autograd: the training route of a call group)."""
        x = {t: (v.materialize() if isinstance(v, LazyRows) else v) for t, v in xs.items()}
        dev = next(iter(x.values())).device
        out = {t: torch.zeros((n, self._width(t)), dtype=torch.float32, device=dev) for t, n in graph.n_out.items() if n > 0}
        for r in graph.relations:
            if r.n_rows == 0:
                continue
            et = r.edge_type
            y = self.conv(et)((x[et[0]], x[et[2]][r.dst_rows]), [r.row_ptr, r.col])
            rows = r.out_rows if r.out_rows is not None else torch.arange(r.n_rows, device=dev)
            out[et[2]] = out[et[2]].index_add(0, rows, y)
        return {t: torch.relu(v) for t, v in out.items()} if act == "relu" else out


# ---------------------------------------------------------------------------------------------------------------------
# NormDropoutAct: the row-wise block between two layers (LayerNorm, dropout, ReLU, residual) — csrc/wg_norm_act.hip
# ---------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
norm_act_launches = 0        # forward launches of wgamd_norm_act_f32 so far (tests: a dict call is ONE launch per 8 types)


def norm_dropout_act_supported(C: int) -> bool:
    """Widths of the NormDropoutAct kernels (``wgamd_norm_act_supported``, answered on the host): C % 4 == 0, 4 <= C <= 1024."""
    return bool(L.lib().wgamd_norm_act_supported(int(C)))


def segment_seed(seed: int, k: int) -> int:
    """The dropout seed of segment ``k`` (the k-th node type of a dict call) under ``seed``: the host twin of the kernel
    launch's ``wgamd_norm_act_segment_seed`` — the splitmix64 output function of ``seed + (k + 1) * 0x9E3779B97F4A7C15``."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _norm_act_auto_seed() -> int:
    """The seed of a training call that passes none: ``torch.initial_seed()`` mixed with one draw of torch's default CPU
    generator, which counts the calls since ``torch.manual_seed`` — host only (no device sync), and the same sequence after
    every ``torch.manual_seed(s)``, also when ``s`` was the seed before.  The draw advances the global CPU random stream."""
    count = int(torch.empty((), dtype=torch.int64).random_())
    return segment_seed((torch.initial_seed() ^ count) & _M64, 0)


def _norm_act_chunks(n: int):
    """``range`` objects of at most ``NORM_ACT_MAX_SEGMENTS`` consecutive segments: the launches of an ``n``-type dict call."""
    return [range(a, min(a + L.NORM_ACT_MAX_SEGMENTS, n)) for a in range(0, n, L.NORM_ACT_MAX_SEGMENTS)]


def _norm_act_flags(norm: bool, relu: bool, save: bool = False) -> int:
    return (L.NORM_ACT_NORM if norm else 0) | (L.NORM_ACT_RELU if relu else 0) | (L.NORM_ACT_SAVE_STATS if save and norm else 0)


def _norm_act_vec_ok(v, C: int) -> bool:
    return v is None or (v.dtype == torch.float32 and v.is_cuda and v.dim() == 1 and v.numel() == C and v.is_contiguous()
                         and v.data_ptr() % 16 == 0)


def _norm_act_rows_ok(t) -> bool:
    """``_kernel_rows_ok`` and rows that do not overlap: at least C floats apart (an expanded tensor's are 0 apart)."""
    return _kernel_rows_ok(t) and t.stride(0) >= t.shape[1]


def _norm_act_kernel_ok(x, weight, bias, residual) -> bool:
    """The kernel's domain: float32 device rows with unit column stride and 16-B alignment, a supported width, ``weight`` /
    ``bias`` of that width."""
    if not (torch.is_tensor(x) and x.dim() == 2 and _norm_act_rows_ok(x) and norm_dropout_act_supported(x.shape[1])):
        return False
    if residual is not None and not (residual.dim() == 2 and residual.shape == x.shape and _norm_act_rows_ok(residual)):
        return False
    return _norm_act_vec_ok(weight, x.shape[1]) and _norm_act_vec_ok(bias, x.shape[1])


def norm_act_forward(segs, norm=True, relu=True, eps=1e-5, p=0.0, seed=0, seed_indices=None, save_stats=False):
    """``wgamd_norm_act_f32`` over ``segs = [(x, residual, weight, bias), ...]`` (include/wgamd_ext.h): ONE launch per 8
    segments.  ``seed_indices[k]``: the segment's index under ``seed`` (``segment_seed``), negative = ``seed`` itself is the
    segment's seed.  Returns ``(outs, stats)``; ``stats[k]`` [n, 2] = (mean, rstd) per row with ``save_stats`` and ``norm``."""
    global norm_act_launches
    outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for x, _, _, _ in segs]
    stats = [torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device) if save_stats and norm else None for x, _, _, _ in segs]
    flags = _norm_act_flags(norm, relu, save_stats)
    for chunk in _norm_act_chunks(len(segs)):
        arr = (L.NormActSegment * len(chunk))()
        for d, k in zip(arr, chunk):
            x, res, w, b = segs[k]
            d.x, d.ldx, d.residual, d.ld_res = x.data_ptr(), x.stride(0), _ptr(res), 0 if res is None else res.stride(0)
            d.out, d.ldo, d.weight, d.bias, d.stats = outs[k].data_ptr(), outs[k].stride(0), _ptr(w), _ptr(b), _ptr(stats[k])
            d.n_rows, d.C, d.seed_index = x.shape[0], x.shape[1], -1 if seed_indices is None else seed_indices[k]
        L.check(L.lib().wgamd_norm_act_f32(arr, len(chunk), float(eps), float(p), int(seed) & _M64, flags, get_stream()),
                "wgamd_norm_act_f32")
        norm_act_launches += 1
    return outs, stats


def norm_act_backward(segs, grads, stats, norm=True, relu=True, eps=1e-5, p=0.0, seed=0, seed_indices=None, need_w=None,
                      need_b=None):
    """``wgamd_norm_act_bwd_f32`` and ``wgamd_norm_act_wgrad_f32`` over the forward's ``segs`` and ``stats``: two launches per 8
    segments.  Returns ``(dz, dweight, dbias)`` lists; ``dz[k]`` is the gradient of segment k's ``x`` and of its residual,
    ``dweight[k]`` / ``dbias[k]`` are None where ``need_w[k]`` / ``need_b[k]`` is false (or without ``norm``)."""
    n = len(segs)
    need_w = [False] * n if need_w is None or not norm else need_w
    need_b = [False] * n if need_b is None or not norm else need_b
    dz = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for x, _, _, _ in segs]
    dw = [torch.empty(x.shape[1], dtype=torch.float32, device=x.device) if need_w[k] else None for k, (x, _, _, _) in enumerate(segs)]
    db = [torch.empty(x.shape[1], dtype=torch.float32, device=x.device) if need_b[k] else None for k, (x, _, _, _) in enumerate(segs)]
    lib, flags, keep = L.lib(), _norm_act_flags(norm, relu), []
    for chunk in _norm_act_chunks(n):
        arr = (L.NormActSegment * len(chunk))()
        for d, k in zip(arr, chunk):
            x, res, w, b = segs[k]
            g = grads[k]
            assert _norm_act_rows_ok(g) and g.shape == x.shape
            d.x, d.ldx, d.residual, d.ld_res = x.data_ptr(), x.stride(0), _ptr(res), 0 if res is None else res.stride(0)
            d.weight, d.bias, d.stats = _ptr(w), _ptr(b), _ptr(stats[k])
            d.n_rows, d.C, d.seed_index = x.shape[0], x.shape[1], -1 if seed_indices is None else seed_indices[k]
            d.grad_out, d.ldg, d.grad_in, d.ld_gi = g.data_ptr(), g.stride(0), dz[k].data_ptr(), dz[k].stride(0)
            if need_w[k] or need_b[k]:
                part = torch.empty((int(lib.wgamd_norm_act_bwd_blocks(x.shape[0], x.shape[1])), 2 * x.shape[1]), dtype=torch.float32,
                                   device=x.device)
                keep.append(part)
                d.partials, d.dweight, d.dbias = (part.data_ptr() if part.numel() else None), _ptr(dw[k]), _ptr(db[k])
        L.check(lib.wgamd_norm_act_bwd_f32(arr, len(chunk), float(eps), float(p), int(seed) & _M64, flags, get_stream()),
                "wgamd_norm_act_bwd_f32")
        if any(need_w[k] or need_b[k] for k in chunk):
            L.check(lib.wgamd_norm_act_wgrad_f32(arr, len(chunk), get_stream()), "wgamd_norm_act_wgrad_f32")
    return dz, dw, db


def _norm_act_torch(x, weight, bias, residual, norm, eps, p, training, relu, mask=None):
    """The same formula out of torch ops under ordinary autograd.  ``mask`` None: ``torch.nn.functional.dropout`` (torch's
    own random stream); else the keep factors (0 or 1 / (1 - p)) to multiply with."""
    z = x if residual is None else x + residual
    if norm:
        z = torch.nn.functional.layer_norm(z, (z.shape[-1],), weight, bias, eps)
    if mask is not None:
        z = z * mask
    elif training and p > 0:
        z = torch.nn.functional.dropout(z, p, True)
    return torch.relu(z) if relu else z


class _NormAct(torch.autograd.Function):
    """``norm_dropout_act`` on the kernel route over n segments: ``tensors`` = the n ``x``, then the n residuals, weights and
    biases (None where absent).  Keeps x, residual, weight, the row statistics and the seed — no mask and not the output; the
    backward is ``norm_act_backward``.  A backward under ``create_graph=True`` (double backward) runs the formula out of torch
    ops with the kernel's own mask instead."""

    @staticmethod
    def forward(ctx, conf, n, *tensors):
        norm, relu, eps, p, seed, seed_indices = conf
        segs = [tuple(None if t is None else t.detach() for t in tensors[k::n]) for k in range(n)]
        outs, stats = norm_act_forward(segs, norm, relu, eps, p, seed, seed_indices, save_stats=True)
        ctx.conf, ctx.n, ctx.stats = conf, n, stats
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        norm, relu, eps, p, seed, seed_indices = ctx.conf
        n, tensors = ctx.n, ctx.saved_tensors
        if torch.is_grad_enabled():
            return (None, None) + _norm_act_double_backward(ctx, tensors, grads)
        segs = [tuple(None if t is None else t.detach() for t in tensors[k::n]) for k in range(n)]
        gs = []
        for (x, _, _, _), g in zip(segs, grads):
            if g is None:
                g = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
            elif not _norm_act_rows_ok(g):        # (an expanded or 16-bit gradient: one copy into rows the kernel reads)
                g = torch.empty(x.shape, dtype=torch.float32, device=x.device).copy_(g)
            gs.append(g)
        need = ctx.needs_input_grad[2:]
        dz, dw, db = norm_act_backward(segs, gs, ctx.stats, norm, relu, eps, p, seed, seed_indices,
                                       need_w=[bool(need[2 * n + k]) for k in range(n)],
                                       need_b=[bool(need[3 * n + k]) for k in range(n)])
        out = [dz[k] if need[k] else None for k in range(n)]
        out += [dz[k] if need[n + k] else None for k in range(n)]
        return (None, None) + tuple(out + dw + db)


def _norm_act_double_backward(ctx, tensors, grads):
    """The gradients as differentiable torch expressions of the saved inputs and ``grads``, with the kernel's keep mask."""
    norm, relu, eps, p, seed, seed_indices = ctx.conf
    n = ctx.n
    res = [None] * (4 * n)
    with torch.enable_grad():
        for k in range(n):
            x, r, w, b = tensors[k::n]
            mask = None
            if p > 0:
                ones = torch.ones(x.shape, dtype=torch.float32, device=x.device)
                s = seed if seed_indices is None or seed_indices[k] < 0 else segment_seed(seed, seed_indices[k])
                mask = norm_act_forward([(ones, None, None, None)], False, False, eps, p, s)[0][0]
            ins = [(i, t) for i, t in ((k, x), (n + k, r), (2 * n + k, w), (3 * n + k, b)) if t is not None and t.requires_grad]
            if not ins or grads[k] is None:
                continue
            y = _norm_act_torch(x, w, b, r, norm, eps, p, True, relu, mask=mask)
            for (i, _), gr in zip(ins, torch.autograd.grad(y, [t for _, t in ins], grads[k], create_graph=True, allow_unused=True)):
                res[i] = gr
    return tuple(res)


def norm_dropout_act(x, weight=None, bias=None, *, residual=None, norm=True, eps=1e-5, p=0.0, training=False, relu=True, seed=None):
    """The block between two message-passing layers in one pass over the rows:
        z = x (+ residual);  y = LayerNorm(z; weight, bias, eps) if norm;  y = y * keep / (1 - p) if training and p > 0;
        out = relu(y) if relu
    — ``torch.nn.LayerNorm`` (biased variance), then dropout, then ReLU: the reference's ``norm -> dropout -> relu``
    (mag_lp_mnmg.py), and with ``norm=False`` its ``relu -> dropout`` (gnn_model.py; the two commute).  ``residual`` is the
    encoder's ``+ lin1(x)`` term; its gradient is ``x``'s.

    ``x``: a [n, C] tensor, or a dict of them keyed by node type — then ``weight``, ``bias`` and ``residual`` are dicts too (a
    missing key = None), the result is a dict, and all types run in ONE launch forward and two backward per 8 types; type k (in
    the dict's order) gets bit for bit what the tensor form gives with ``seed=segment_seed(seed, k)``.

    ``route``: the kernels (``wgamd_norm_act_f32``, include/wgamd_ext.h) run for float32 device tensors with unit column stride,
    16-B aligned rows, ``norm_dropout_act_supported(C)`` and ``weight`` / ``bias`` of width C; a dict takes them when every type
    does.  The dropout mask is then a stateless function of ``(seed, row, column)`` — nothing is stored for the backward, and the
    same inputs give the same bits on every run.  ``seed=None`` draws one on the host from ``torch.initial_seed()`` and torch's
    default CPU generator (no device sync; the same sequence after every ``torch.manual_seed``) — every such call therefore
    advances the global CPU random stream by one draw, as a CPU dropout would: a later ``torch.randperm`` or shuffle sees other
    values than without the call; pass ``seed`` to leave the stream alone.  A dropped element is exactly 0 also where ``y`` is NaN
    or infinite (torch's dropout gives ``NaN * 0 = NaN`` there); a kept NaN stays NaN through the ReLU, as ``torch.relu``'s.
    Everything else (CPU tensors, other dtypes and widths, rows less than C floats apart such as an expanded tensor's, a
    broadcast ``weight``) runs the same formula out of torch ops, and so does a double backward; there dropout is
    ``torch.nn.functional.dropout``, which draws from torch's own random stream: ``seed`` is not used.
    ``norm=False`` without a residual and without active dropout is ``torch.relu`` (no launch).  Under HIP-graph capture,
    training with ``p > 0`` is refused (a captured host seed would replay one mask); every other mode may be captured."""
    return _norm_dropout_act(x, weight, bias, residual, norm, eps, p, training, relu, seed)[0]


def _norm_dropout_act(x, weight, bias, residual, norm, eps, p, training, relu, seed):
    """``(result, route)`` of ``norm_dropout_act``."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("norm_dropout_act: dropout probability has to be between 0 and 1, but got %r" % (p,))
    is_dict = isinstance(x, dict)
    if is_dict:
        keys = list(x)
        pick = lambda d, t: None if d is None else d.get(t)      # noqa: E731
        segs = [(x[t], pick(residual, t), pick(weight, t), pick(bias, t)) for t in keys]
    else:
        keys, segs = [None], [(x, residual, weight, bias)]
    segs = [(xs, r, w if norm else None, b if norm else None) for xs, r, w, b in segs]
    drop = bool(training) and p > 0
    p_eff = float(p) if drop else 0.0

    def wrap(outs):
        return dict(zip(keys, outs)) if is_dict else outs[0]

    if not norm and not drop and all(r is None for _, r, _, _ in segs):
        return wrap([torch.relu(xs) if relu else xs.clone() for xs, _, _, _ in segs]), "torch"      # (always a fresh tensor)
    if not segs or not all(_norm_act_kernel_ok(xs, w, b, r) for xs, r, w, b in segs):
        return wrap([_norm_act_torch(xs, w, b, r, norm, eps, p_eff, drop, relu) for xs, r, w, b in segs]), "torch"
    if drop:
        _refuse_capture("norm_dropout_act", "host-side dropout seeds (training with p > 0: a replay would repeat one mask)")
    if seed is None:
        seed = _norm_act_auto_seed() if drop else 0
    n = len(segs)
    seed_indices = list(range(n)) if is_dict else None
    flat = [s[i] for i in (0, 1, 2, 3) for s in segs]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat):
        outs = _NormAct.apply((bool(norm), bool(relu), float(eps), p_eff, int(seed) & _M64, seed_indices), n, *flat)
    else:
        outs = norm_act_forward([tuple(None if t is None else t.detach() for t in s) for s in segs], norm, relu, eps, p_eff, seed,
                                seed_indices)[0]
    return wrap(list(outs)), "kernel"


class NormDropoutAct(torch.nn.Module):
    """``norm_dropout_act`` as a module: ``forward(x, residual=None, seed=None)`` = relu(dropout(LayerNorm(x + residual))) with
    each stage optional (``norm``, ``p``, ``relu``).  The parameters are ``torch.nn.LayerNorm``'s — ``weight`` and ``bias``
    [channels], ones and zeros — under the same state-dict keys, so a reference checkpoint's ``norm1.*`` loads;
    ``elementwise_affine=False`` has neither, ``bias=False`` no bias.  ``self.training`` drives dropout.  ``route``:
    ``"kernel"`` or ``"torch"``, what the last forward took (see ``norm_dropout_act``)."""

    def __init__(self, channels: int, norm: bool = True, p: float = 0.0, relu: bool = True, eps: float = 1e-5,
                 elementwise_affine: bool = True, bias: bool = True):
        super().__init__()
        if not 0.0 <= p <= 1.0:
            raise ValueError("NormDropoutAct: dropout probability has to be between 0 and 1, but got %r" % (p,))
        self.channels, self.norm, self.p, self.relu, self.eps = int(channels), bool(norm), float(p), bool(relu), float(eps)
        self.elementwise_affine = bool(elementwise_affine)
        affine = self.norm and self.elementwise_affine
        self.weight = torch.nn.Parameter(torch.empty(self.channels)) if affine else None
        self.bias = torch.nn.Parameter(torch.empty(self.channels)) if affine and bias else None
        self.route = None
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight is not None:
            torch.nn.init.ones_(self.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, residual=None, seed=None):
        out, self.route = _norm_dropout_act(x, self.weight, self.bias, residual, self.norm, self.eps, self.p, self.training,
                                            self.relu, seed)
        return out

    def extra_repr(self):
        return "%d, norm=%s, p=%g, relu=%s, eps=%g" % (self.channels, self.norm, self.p, self.relu, self.eps)


class HeteroNormDropoutAct(torch.nn.Module):
    """One ``NormDropoutAct`` per node type (``norms``: a ModuleDict, state-dict keys ``norms.<type>.weight`` / ``.bias``) run
    as ONE launch over all types of ``x_dict`` — what ``to_hetero`` makes of the reference encoder's ``norm -> dropout -> relu``.
    ``channels``: ``{node_type: width}``; the other arguments are ``NormDropoutAct``'s.  ``forward(x_dict, residual_dict=None,
    seed=None)`` returns a dict over the types of ``x_dict`` (types without rows in this call are simply absent from it; a type
    of ``x_dict`` the module does not know is a KeyError)."""

    def __init__(self, channels, norm: bool = True, p: float = 0.0, relu: bool = True, eps: float = 1e-5,
                 elementwise_affine: bool = True, bias: bool = True):
        super().__init__()
        self.norms = torch.nn.ModuleDict({t: NormDropoutAct(c, norm, p, relu, eps, elementwise_affine, bias) for t, c in channels.items()})
        self.norm, self.p, self.relu, self.eps = bool(norm), float(p), bool(relu), float(eps)
        self.route = None

    def reset_parameters(self):
        for m in self.norms.values():
            m.reset_parameters()

    def forward(self, x_dict, residual_dict=None, seed=None):
        mods = {t: self.norms[t] for t in x_dict}
        out, self.route = _norm_dropout_act(x_dict, {t: m.weight for t, m in mods.items()}, {t: m.bias for t, m in mods.items()},
                                            residual_dict, self.norm, self.eps, self.p, self.training, self.relu, seed)
        return out


# ---------------------------------------------------------------------------------------------------------------------
# RowLinear: a Linear over gathered rows with a row-wise epilogue (ReLU, LayerNorm or L2 norm, add) — csrc/wg_row_linear.hip
# ---------------------------------------------------------------------------------------------------------------------
row_linear_launches = 0      # forward launches of wgamd_row_linear_f32 so far (tests: the kernel route ran, once per call)
_ROW_LINEAR_NORMS = {None: L.ROW_LINEAR_NORM_NONE, "layer": L.ROW_LINEAR_NORM_LAYER, "l2": L.ROW_LINEAR_NORM_L2}
_WGRAD_MAX_F = 256           # columns of the kept rows one wgamd_gcn_wgrad_f32 call takes


def linear_rows_supported(K: int, N: int) -> bool:
    """Widths of the RowLinear kernels (``wgamd_row_linear_supported``, answered on the host): K % 4 == 0, 4 <= K <= 1024,
    N % 4 == 0, 4 <= N <= 256."""
    return bool(L.lib().wgamd_row_linear_supported(int(K), int(N)))


def _row_linear_eps(norm, eps) -> float:
    return float(eps) if eps is not None else (1e-12 if norm == "l2" else 1e-5)


def row_linear_forward(src, ids, weight, bias=None, relu=False, norm=None, gamma=None, beta=None, eps=None, add=None, out=None,
                       keep_x=False, keep_y=False):
    """``wgamd_row_linear_f32`` (include/wgamd_ext.h), ONE launch: ``src`` a float32 / float16 / bfloat16 ``[m, K]`` table read by
    row or through ``ids`` (int32 / int64), ``weight`` [N, K].  Returns ``(out, kept_x, kept_y)``: the float32 input rows and the
    rows after the ReLU and before the norm, where asked for (else None)."""
    global row_linear_launches
    n = int(src.shape[0] if ids is None else ids.shape[0])
    K, N = int(src.shape[1]), int(weight.shape[0])
    out = _out_rows(out, n, N, src.device)
    kept_x = torch.empty((n, K), dtype=torch.float32, device=src.device) if keep_x else None
    kept_y = torch.empty((n, N), dtype=torch.float32, device=src.device) if keep_y else None
    L.check(L.lib().wgamd_row_linear_f32(src.data_ptr(), torch_dtype_to_wm(src.dtype), src.stride(0), _ptr(ids),
                                         0 if ids is None else torch_dtype_to_wm(ids.dtype), n, K, weight.data_ptr(),
                                         weight.stride(0), N, _ptr(bias), int(bool(relu)), _ROW_LINEAR_NORMS[norm], _ptr(gamma),
                                         _ptr(beta), _row_linear_eps(norm, eps), _ptr(add), 0 if add is None else add.stride(0),
                                         out.data_ptr(), out.stride(0), _ptr(kept_x), K, _ptr(kept_y), N, get_stream()),
            "wgamd_row_linear_f32")
    if n > 0:
        row_linear_launches += 1
    return out, kept_x, kept_y


def row_linear_backward(kept_y, grad_out, relu=False, norm=None, gamma=None, eps=None, need_gamma=False, need_beta=False):
    """``wgamd_row_linear_bwd_f32`` and, for LayerNorm's affine gradients, ``wgamd_row_linear_affine_grad_f32``: ``(dy, dgamma,
    dbeta)`` — ``grad_out`` through the norm (statistics recomputed from ``kept_y``) and the ReLU mask ``kept_y > 0``; the affine
    gradients through per-workgroup partial rows added in a fixed order (None where not asked for, or without ``norm="layer"``)."""
    n, N = grad_out.shape
    lib, dev = L.lib(), grad_out.device
    dy = torch.empty((n, N), dtype=torch.float32, device=dev)
    affine = norm == "layer" and (need_gamma or need_beta)
    part = torch.empty((int(lib.wgamd_row_linear_bwd_blocks(n, N)), 2 * N), dtype=torch.float32, device=dev) if affine else None
    L.check(lib.wgamd_row_linear_bwd_f32(_ptr(kept_y), 0 if kept_y is None else kept_y.stride(0), grad_out.data_ptr(),
                                         grad_out.stride(0), n, N, int(bool(relu)), _ROW_LINEAR_NORMS[norm], _ptr(gamma),
                                         _row_linear_eps(norm, eps), dy.data_ptr(), dy.stride(0),
                                         part.data_ptr() if affine and part.numel() else None, get_stream()),
            "wgamd_row_linear_bwd_f32")
    dg = torch.empty(N, dtype=torch.float32, device=dev) if affine and need_gamma else None
    db = torch.empty(N, dtype=torch.float32, device=dev) if affine and need_beta else None
    if affine:
        L.check(lib.wgamd_row_linear_affine_grad_f32(part.data_ptr() if part.numel() else None, n, N, _ptr(dg), _ptr(db), get_stream()),
                "wgamd_row_linear_affine_grad_f32")
    return dy, dg, db


def _row_linear_wgrad(kept_x, dy, want_bias: bool):
    """``(dW, db)`` = ``(dy^T kept_x, colsum(dy))`` through ``gcn_wgrad`` (deterministic split-K), 256 columns of ``kept_x`` per
    call."""
    N, K = dy.shape[1], kept_x.shape[1]
    gb = torch.empty(N, dtype=torch.float32, device=dy.device) if want_bias else None
    if K <= _WGRAD_MAX_F:
        gw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
        gcn_wgrad(kept_x, dy, gw, gb)
        return gw, gb
    parts = []
    for k0 in range(0, K, _WGRAD_MAX_F):
        k1 = min(k0 + _WGRAD_MAX_F, K)
        parts.append(torch.empty((N, k1 - k0), dtype=torch.float32, device=dy.device))
        gcn_wgrad(kept_x[:, k0:k1], dy, parts[-1], gb if k0 == 0 else None)
    return torch.cat(parts, dim=1), gb


def _linear_rows_torch(xr, weight, bias, relu, norm, gamma, beta, eps, add):
    """The same formula out of torch ops under ordinary autograd, over the gathered float32 rows ``xr``."""
    y = torch.nn.functional.linear(xr, weight, bias)
    if relu:
        y = y.relu()
    if norm == "layer":
        y = torch.nn.functional.layer_norm(y, (y.shape[-1],), gamma, beta, eps)
    elif norm == "l2":
        y = torch.nn.functional.normalize(y, p=2.0, dim=-1, eps=eps)
    return y if add is None else y + add


class _RowLinear(torch.autograd.Function):
    """``linear_rows`` on the kernel route.  ``src`` is the input tensor (``x_grad``: it may want a gradient) or the detached
    table of a ``LazyRows``; ``ids`` what the kernel reads it through.  Kept for the backward: the float32 input rows (only when
    they are not ``src`` itself) and the rows before the norm (with a norm, or with ReLU and ``add``; with ReLU alone the output
    is the mask).  The backward is ``row_linear_backward``, ``gcn_wgrad`` and one library GEMM for dX; a backward under
    ``create_graph=True`` runs the formula out of torch ops instead."""

    @staticmethod
    def forward(ctx, conf, src, ids, weight, bias, gamma, beta, add):
        relu, norm, eps, x_grad = conf
        d = lambda t: None if t is None else t.detach()      # noqa: E731
        need = ctx.needs_input_grad
        direct = ids is None and src.dtype == torch.float32
        keep_y = norm is not None or (relu and add is not None)
        res, kept_x, kept_y = row_linear_forward(d(src), ids, d(weight), d(bias), relu, norm, d(gamma), d(beta), eps, d(add),
                                                 keep_x=(need[3] or need[4]) and not direct, keep_y=keep_y)
        if relu and not keep_y:
            kept_y = res
        ctx.conf, ctx.direct = conf, direct
        ctx.save_for_backward(src, ids, weight, bias, gamma, beta, add, kept_x, kept_y)
        ctx.set_materialize_grads(False)
        return res

    @staticmethod
    def backward(ctx, g):
        relu, norm, eps, x_grad = ctx.conf
        src, ids, weight, bias, gamma, beta, add, kept_x, kept_y = ctx.saved_tensors
        need = ctx.needs_input_grad
        if g is None:
            return (None,) * 8
        if torch.is_grad_enabled():
            return _row_linear_double_backward(ctx, g)
        if not _norm_act_rows_ok(g):              # (an expanded or 16-bit gradient: one copy into rows the kernel reads)
            g = torch.empty(g.shape, dtype=torch.float32, device=g.device).copy_(g)
        dy, dg, db = g, None, None
        if relu or norm is not None:
            dy, dg, db = row_linear_backward(kept_y, g, relu, norm, None if gamma is None else gamma.detach(), eps,
                                             need_gamma=need[5], need_beta=need[6])
        gw = gb = gx = None
        if need[3] or need[4]:
            gw, gb = _row_linear_wgrad(src.detach() if ctx.direct else kept_x, dy, need[4])
        if need[1] and x_grad:
            gx = dy @ weight.detach()
            if ids is not None:
                gx = torch.zeros(src.shape, dtype=torch.float32, device=g.device).index_add_(0, ids.long(), gx)
        return (None, gx, None, gw if need[3] else None, gb, dg, db, g if need[7] else None)


def _row_linear_double_backward(ctx, g):
    """The gradients as differentiable torch expressions of the saved inputs and ``g``."""
    relu, norm, eps, x_grad = ctx.conf
    src, ids, weight, bias, gamma, beta, add, _, _ = ctx.saved_tensors
    res = [None] * 8
    with torch.enable_grad():
        xr = src if ids is None else src[ids.long()]
        y = _linear_rows_torch(xr.float(), weight, bias, relu, norm, gamma, beta, _row_linear_eps(norm, eps), add)
        ins = [(i, t) for i, t in ((1, src), (3, weight), (4, bias), (5, gamma), (6, beta), (7, add))
               if t is not None and t.requires_grad and ctx.needs_input_grad[i]]
        if ins:
            for (i, _), gr in zip(ins, torch.autograd.grad(y, [t for _, t in ins], g, create_graph=True, allow_unused=True)):
                res[i] = gr
    return tuple(res)


def _row_vec_ok(v, N: int) -> bool:
    return v is None or (torch.is_tensor(v) and v.dtype == torch.float32 and v.is_cuda and v.dim() == 1 and v.numel() == N
                         and v.is_contiguous() and v.data_ptr() % 16 == 0)


def linear_rows(x, weight, bias=None, *, rows=None, relu=False, norm=None, norm_weight=None, norm_bias=None, eps=None, add=None,
                out=None):
    """A Linear over gathered rows with a row-wise epilogue, in one pass:
        y = x[rows] @ weight^T + bias;  y = relu(y) if relu
        z = layer_norm(y; norm_weight, norm_bias, eps) if norm == "layer";  y / max(||y||_2, eps) if norm == "l2";  y otherwise
        out = z + add
    — the dense products around the reference's layers: ``paper_norm(paper_lin(x))`` over the stored features, ``lin1(x)`` on a
    layer's output rows (``rows``), ``normalize(lin2(x).relu()) + x_paper``, and the plain ``lin(x)`` heads.  ``eps=None`` is 1e-5
    for ``"layer"`` (``torch.nn.LayerNorm``'s) and 1e-12 for ``"l2"`` (``torch.nn.functional.normalize``'s).

    ``x``: a float32 ``[m, K]`` tensor, or ``LazyRows`` over a float32 / float16 / bfloat16 table — row ``i`` is
    ``table[ids[i]]`` converted to float32 exactly, so a 16-bit table gives bit for bit the result over ``table.float()``.
    ``rows`` (int64 or int32, optional): the ``n`` rows of ``x`` to take, repeats allowed; for ``LazyRows`` it is composed with the
    id list by one index op on the ids (``ids[rows]``) — the rows themselves are never gathered.  ``add``: ``[n, N]``.  ``out``
    (optional): a float32 ``[n, N]`` tensor or column-sliced view with 16-B aligned rows to write into (the kernel writes it
    directly; a result that carries a gradient is copied into it once).

    ``route``: the kernel (``wgamd_row_linear_f32``, include/wgamd_ext.h: ONE launch; the ``[n, K]`` float32 copy of a lazy
    input's rows and the ``[n, N]`` intermediates between the product, the norm and the add never exist) runs when the tensors
    are on the device, ``linear_rows_supported(K, N)``, ``weight`` / ``add`` / ``out`` and a float32 ``x`` are float32 with unit
    column stride and 16-B aligned rows (a 16-bit table: 8-B aligned rows), and a ``LazyRows`` table is a ``torch.Tensor``.  In
    training it keeps the float32 input rows only when they are not ``x`` itself (``rows`` or a ``LazyRows``), and the rows
    before the norm; the backward is one launch for ``dy`` (two with LayerNorm's affine gradients: per-workgroup partial rows
    added in a fixed order), ``gcn_wgrad`` for ``dW`` / ``db`` and one library GEMM for ``dX`` — no float atomics in the
    kernels, so the same call gives the same gradient bits.  ``dX`` with ``rows`` is scattered with ``index_add_`` into zeros:
    exact and reproducible when ``rows`` are distinct, as a layer's output rows are (repeats add up in an order the library does
    not fix).  A ``LazyRows`` input never gets a gradient.  ``rows`` are not range-checked on this route.
    Everything else — CPU tensors, a ``MappedTable``-backed ``LazyRows``, float64, widths outside the domain — runs the same
    formula out of torch ops under ordinary autograd (a ``LazyRows`` materialises there; ``rows`` out of range is a
    ValueError), and so does a double backward."""
    return _linear_rows(x, weight, bias, rows, relu, norm, norm_weight, norm_bias, eps, add, out)[0]


def _linear_rows(x, weight, bias, rows, relu, norm, gamma, beta, eps, add, out):
    """``(result, route)`` of ``linear_rows``."""
    if norm not in _ROW_LINEAR_NORMS:
        raise ValueError("linear_rows: norm must be None, 'layer' or 'l2', got %r" % (norm,))
    lazy = isinstance(x, LazyRows)
    if not lazy and not torch.is_tensor(x):
        raise ValueError("linear_rows: x must be a tensor or LazyRows, got %s" % type(x).__name__)
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError("linear_rows: x %s does not match weight %s" % (tuple(x.shape), tuple(weight.shape)))
    if rows is not None and (rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64)):
        raise ValueError("linear_rows: rows must be a 1-d int64 (or int32) tensor")
    if norm != "layer":
        gamma = beta = None
    m, K = int(x.shape[0]), int(x.shape[1])
    n, N = (m if rows is None else int(rows.shape[0])), int(weight.shape[0])
    if add is not None and tuple(add.shape) != (n, N):
        raise ValueError("linear_rows: add has shape %s, the result has (%d, %d)" % (tuple(add.shape), n, N))
    if out is not None and tuple(out.shape) != (n, N):
        raise ValueError("linear_rows: out has shape %s, the result has (%d, %d)" % (tuple(out.shape), n, N))
    eps_v = _row_linear_eps(norm, eps)
    if lazy:
        _refuse_lazy_table_grad(x.table)
    src = x.table if lazy else x
    kernel = (torch.is_tensor(src) and src.is_cuda and src.dim() == 2 and src.stride(1) == 1 and src.stride(0) % 4 == 0
              and linear_rows_supported(K, N)
              and (src.dtype == torch.float32 and src.data_ptr() % 16 == 0 or lazy and src.dtype in _X16 and src.data_ptr() % 8 == 0)
              and _kernel_rows_ok(weight) and _row_vec_ok(bias, N) and _row_vec_ok(gamma, N) and _row_vec_ok(beta, N)
              and (rows is None or rows.is_cuda) and (not lazy or x.ids.is_cuda) and (add is None or _norm_act_rows_ok(add))
              and (out is None or _norm_act_rows_ok(out)))
    if not kernel:
        if rows is not None and rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= m):
            raise ValueError("linear_rows: rows out of range for an input of %d rows" % m)
        if lazy and torch.is_tensor(x.table) and not x.table.is_cuda:
            ids = x.ids if rows is None else x.ids[rows.long()]      # (a host table: only the n rows are gathered, by torch,
            xr = x.table[ids.long()].float()                         # and converted exactly)
        else:
            xr = x.materialize() if lazy else x
            if rows is not None:
                xr = xr[rows.long()]
        res = _linear_rows_torch(xr, weight, bias, relu, norm, gamma, beta, eps_v, add)
        return (res if out is None else out.copy_(res)), "torch"
    if lazy:
        assert x.ids.dtype in (torch.int32, torch.int64) and x.ids.is_contiguous()      # (what LazyRows guarantees and the kernel reads)
        ids = x.ids if rows is None else x.ids[rows.long()]
    else:
        ids = None if rows is None else rows.contiguous()
    tensors = (src, weight, bias, gamma, beta, add)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        res = _RowLinear.apply((bool(relu), norm, eps_v, not lazy), src.detach() if lazy else src, ids, weight, bias, gamma, beta,
                               add)
        if out is not None:       # (a result that carries a gradient is written once more, into the caller's rows)
            res = out.copy_(res)
    else:
        d = lambda t: None if t is None else t.detach()      # noqa: E731
        res = row_linear_forward(d(src), ids, d(weight), d(bias), relu, norm, d(gamma), d(beta), eps_v, d(add), out)[0]
    return res, "kernel"


class RowLinear(torch.nn.Module):
    """``linear_rows`` as a module: ``forward(x, rows=None, add=None)`` = ``norm(act(lin(x[rows]))) + add``.  The submodules are
    ``lin`` (``torch.nn.Linear``) and, for ``norm="layer"``, ``norm`` (``torch.nn.LayerNorm``) — their parameters, their
    initialisation and their state-dict keys (``lin.weight``, ``lin.bias``, ``norm.weight``, ``norm.bias``).  ``norm="l2"`` is
    ``torch.nn.functional.normalize`` and has no parameters; ``elementwise_affine`` (None: LayerNorm's default, True) given with it
    is a ValueError.  ``RowLinear.wrap(lin, norm=None, relu=False, l2=False)`` adopts
    existing modules (parameters shared, not copied): a model's ``paper_lin`` / ``paper_norm`` pair or its ``lin2`` run through
    the kernel without touching a checkpoint.  ``route``: ``"kernel"`` or ``"torch"``, what the last forward took (see
    ``linear_rows``)."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True, relu: bool = False, norm: Optional[str] = None,
                 eps: Optional[float] = None, elementwise_affine: Optional[bool] = None):
        super().__init__()
        self._configure(relu, norm, eps, elementwise_affine)
        self.lin = torch.nn.Linear(int(in_channels), int(out_channels), bias=bool(bias))
        if norm == "layer":
            self.norm = torch.nn.LayerNorm(int(out_channels), eps=self.eps,
                                           elementwise_affine=True if elementwise_affine is None else bool(elementwise_affine))

    def _configure(self, relu, norm, eps, elementwise_affine=None):
        if norm not in _ROW_LINEAR_NORMS:
            raise ValueError("RowLinear: norm must be None, 'layer' or 'l2', got %r" % (norm,))
        if norm != "layer" and elementwise_affine is not None:
            raise ValueError("RowLinear: elementwise_affine belongs to norm='layer' (norm=%r has no parameters)" % (norm,))
        self.relu, self.norm_kind, self.eps, self.route = bool(relu), norm, _row_linear_eps(norm, eps), None

    @classmethod
    def wrap(cls, lin: torch.nn.Linear, norm: Optional[torch.nn.LayerNorm] = None, relu: bool = False, l2: bool = False):
        """A ``RowLinear`` over the existing ``lin`` (and ``norm``) modules themselves."""
        if not isinstance(lin, torch.nn.Linear) or not (norm is None or isinstance(norm, torch.nn.LayerNorm)):
            raise ValueError("RowLinear.wrap: lin must be a torch.nn.Linear and norm a torch.nn.LayerNorm (or None)")
        if norm is not None and (l2 or tuple(norm.normalized_shape) != (lin.out_features,)):
            raise ValueError("RowLinear.wrap: a LayerNorm over lin's %d output channels, or l2=True, not both" % lin.out_features)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m._configure(relu, "layer" if norm is not None else "l2" if l2 else None, norm.eps if norm is not None else None)
        m.lin = lin
        if norm is not None:
            m.norm = norm
        return m

    @property
    def in_channels(self):
        return self.lin.in_features

    @property
    def out_channels(self):
        return self.lin.out_features

    def reset_parameters(self):
        self.lin.reset_parameters()
        if self.norm_kind == "layer":
            self.norm.reset_parameters()

    def forward(self, x, rows=None, add=None):
        ln = self.norm if self.norm_kind == "layer" else None
        out, self.route = _linear_rows(x, self.lin.weight, self.lin.bias, rows, self.relu, self.norm_kind,
                                       None if ln is None else ln.weight, None if ln is None else ln.bias, self.eps, add, None)
        return out

    def extra_repr(self):
        return "relu=%s, norm=%r, eps=%g" % (self.relu, self.norm_kind, self.eps)
