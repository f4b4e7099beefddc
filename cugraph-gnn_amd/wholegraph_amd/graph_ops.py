"""Sampled-subgraph ops with the names and behaviour of ``pylibwholegraph.torch.graph_ops``
(/root/reference/python/pylibwholegraph/pylibwholegraph/torch/graph_ops.py:15-95), on the HIP kernels
of ``libwholegraph_amd`` (``graph_append_unique`` / ``csr_add_self_loop``, include/wgamd_ops.h)."""
import torch

from . import _lib as L
from .env import TorchMemoryContext, get_stream, get_wholegraph_env_fns, wrap_torch_tensor


def _require_device_vectors(**tensors):
    for name, t in tensors.items():
        assert t.dim() == 1, f"{name} must be 1-D"
        assert t.is_cuda, f"{name} must live on the GPU"


def append_unique(target_node_tensor: torch.Tensor, neighbor_node_tensor: torch.Tensor,
                  need_neighbor_raw_to_unique: bool = False):
    """Renumbering step of a hop: ``unique = targets ++ (neighbours not among the targets)``.

    The targets keep their positions (ids ``0..T-1``); every other neighbour id appears once, in order
    of first appearance (the reference leaves that order unspecified).  With
    ``need_neighbor_raw_to_unique`` the int32 position of every neighbour inside ``unique`` is returned
    too.  Example (the reference's, graph_ops.py:21-29): targets ``[3, 11, 2, 10]``, neighbours
    ``[4, 5, 2, 11, 6, 9, 10, 5]`` give ``unique = [3, 11, 2, 10, 4, 5, 6, 9]`` and
    ``mapping = [4, 5, 2, 1, 6, 7, 3, 5]``.
    """
    _require_device_vectors(target_node_tensor=target_node_tensor, neighbor_node_tensor=neighbor_node_tensor)
    mapping = (torch.empty(neighbor_node_tensor.shape[0], dtype=torch.int32, device=neighbor_node_tensor.device)
               if need_neighbor_raw_to_unique else None)
    unique_ctx = TorchMemoryContext()           # the op allocates `unique` through the env callbacks
    handles = [wrap_torch_tensor(t) for t in (target_node_tensor, neighbor_node_tensor, mapping)]
    rc = L.lib().graph_append_unique(handles[0].c, handles[1].c, unique_ctx.get_c_context(), handles[2].c,
                                     get_wholegraph_env_fns(), get_stream())
    L.check(rc, "graph_append_unique")
    unique = unique_ctx.get_tensor()
    return (unique, mapping) if need_neighbor_raw_to_unique else unique


def add_csr_self_loop(csr_row_ptr_tensor: torch.Tensor, csr_col_ptr_tensor: torch.Tensor):
    """Row ``i`` of a sampled int32 CSR becomes ``[i] ++ row i`` (GAT-style self loops; graph_ops.py:63-95).
    Existing self loops are not detected.  Returns the new ``(row_ptr, col)``."""
    _require_device_vectors(csr_row_ptr_tensor=csr_row_ptr_tensor, csr_col_ptr_tensor=csr_col_ptr_tensor)
    n_rows = csr_row_ptr_tensor.shape[0] - 1
    new_row_ptr = torch.empty_like(csr_row_ptr_tensor)
    new_col = csr_col_ptr_tensor.new_empty(csr_col_ptr_tensor.shape[0] + n_rows)
    handles = [wrap_torch_tensor(t) for t in (csr_row_ptr_tensor, csr_col_ptr_tensor, new_row_ptr, new_col)]
    L.check(L.lib().csr_add_self_loop(*(h.c for h in handles), get_stream()), "csr_add_self_loop")
    return new_row_ptr, new_col


_ROWS_UNIQUE_WS = {}   # (device index, stream) -> the reusable workspace of wgamd_rows_first_unique (its ticket stays zeroed)


def rows_first_unique_supported(n_rows: int, row_len: int, n_ids: int) -> bool:
    """The domain of the row-wise de-duplication kernel (``wgamd_rows_first_unique_supported``, include/wgamd_ext.h)."""
    return bool(L.lib().wgamd_rows_first_unique_supported(int(n_rows), int(row_len), int(n_ids)))


def rows_first_unique(ends: torch.Tensor, n_ids: int):
    """Row-wise first-appearance de-duplication of ``ends`` int64 [G, S] (device, values in [0, n_ids)) in two launches, with no
    host synchronisation (``wgamd_rows_first_unique``): ``(uniq int64 [G S], seg int32 [G + 1], batch int32 [G S], local int64
    [G, S])`` — row g's distinct values in order of first position from ``seg[g]`` on, the row of every live entry, the position
    of every element in its row's list; both tails are zero.  Outside ``rows_first_unique_supported`` this is an error."""
    assert ends.dim() == 2 and ends.dtype == torch.int64 and ends.is_cuda, "ends: int64 [G, S] on the device"
    G, S = ends.shape
    if not rows_first_unique_supported(G, S, n_ids):
        raise ValueError(f"rows_first_unique: [{G}, {S}] with {n_ids} ids is outside the kernel's domain")
    ends = ends.contiguous()
    dev, lib, stream = ends.device, L.lib(), get_stream()
    uniq = torch.empty(G * S, dtype=torch.int64, device=dev)
    seg = torch.empty(G + 1, dtype=torch.int32, device=dev)
    batch = torch.empty(G * S, dtype=torch.int32, device=dev)
    local = torch.empty((G, S), dtype=torch.int64, device=dev)
    need = lib.wgamd_rows_first_unique_workspace_bytes(G, S)
    key = (dev.index, stream.value)
    ws = _ROWS_UNIQUE_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _ROWS_UNIQUE_WS[key] = torch.zeros(need, dtype=torch.uint8, device=dev)
    L.check(lib.wgamd_rows_first_unique(ends.data_ptr(), G, S, int(n_ids), uniq.data_ptr(), seg.data_ptr(), batch.data_ptr(),
                                        local.data_ptr(), ws.data_ptr(), ws.numel(), 1, stream), "wgamd_rows_first_unique")
    return uniq, seg, batch, local


def rows_first_values(local: torch.Tensor, seg: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """``values`` int64 [G, S] taken at the FIRST position of every distinct id of a row: with ``local`` [G, S] / ``seg`` int32
    [G + 1] as ``rows_first_unique`` returns them, int64 [G S] parallel to ``uniq`` — ``out[seg[g] + r]`` = the value at the
    first position s of row g with ``local[g, s] == r``; zero from ``seg[G]`` on.  (The seed time of a de-duplicated endpoint of
    a temporal link call group: the time of the first seed edge that names it.)  One launch and no read-back
    (``wgamd_rows_first_values``) on the device inside ``rows_first_unique_supported``; the torch formulation otherwise, with
    the same result."""
    assert local.dim() == 2 and local.shape == values.shape and values.dtype == torch.int64 and seg.shape[0] == local.shape[0] + 1
    G, S = local.shape
    dev = local.device
    if local.is_cuda and local.dtype == torch.int64 and seg.dtype == torch.int32 and rows_first_unique_supported(G, S, 1):
        local, seg, values = local.contiguous(), seg.contiguous(), values.contiguous()
        out = torch.empty(G * S, dtype=torch.int64, device=dev)
        L.check(L.lib().wgamd_rows_first_values(local.data_ptr(), seg.data_ptr(), values.data_ptr(), G, S, out.data_ptr(),
                                                get_stream()), "wgamd_rows_first_values")
        return out
    n = G * S
    at = (seg[:-1].to(torch.int64).view(G, 1) + local.to(torch.int64)).reshape(-1)
    first = torch.full((n,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, at, torch.arange(n, device=dev), reduce="amin")
    picked = values.reshape(-1)[first.clamp(max=max(n - 1, 0))]
    return torch.where(first < n, picked, torch.zeros_like(picked))
