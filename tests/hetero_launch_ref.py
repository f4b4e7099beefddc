"""float64 restatements of ONE launch of the heterogeneous layer kernels — the yardstick of the launch-level tests
(tests/test_gpu_hetero_sage_launch.py, tests/test_gpu_transformer_corners.py).  They take the tuples ``nn.hetero_sage_launch`` and
``nn.hetero_transformer_launch`` take and return ``(out, kept_rows, magnitude_sum)`` (the transformer one ``alpha`` per relation
as well):

    SAGE          C[i] = [ REDUCE_r1(i) | REDUCE_r2(i) | ... | x_dst[dst_ids[dst_rows[i]]] ]
                  REDUCE_r(i) = (mean ? 1 / max(deg_r(i), 1) : 1) sum_{e in row i of r} scale_r[col_r[e]] x_r[ids_r[col_r[e]]]
    transformer   A[i] = [ blk^r1_0 | ... | blk^r1_{H-1} | blk^r2_0 | ... | x_dst[...] ],  blk^r_h = sum_e alpha^r_eh [x | a | 1 | 0 pad]
                  alpha^r = softmax over the edges of row i of relation r of  u^r_ih . x_j + w^r_ih . a^r_e
    both          out[p(i)] = act( C[i] wt^T + bias + acc_in[i] ),  p(i) = out_rows ? out_rows[i] : i

``kept_rows`` is C (A) [n_rows, K]; ``magnitude_sum`` is sum_k |C_ik| |wt_nk| + |bias_n| + |acc_in_in| with C built from |x|, |scale|
(and |a|; alpha the true weights) — the scale of the project's 1e-5 bar —, placed like ``out``.  ``abs_terms=True`` returns the
absolute-value run itself: its ``kept_rows`` is the magnitude sum of every element of C (A).

``edge_case_hop`` builds a hop's CSR from an explicit per-row degree list.  No GPU is needed: everything follows the device of its
inputs."""


def edge_case_hop(n_rows, n_src, degrees, seed):
    """``(row_ptr int32 [n_rows + 1], col int32 [E])`` on the CPU: row i has ``degrees[i]`` edges whose sources are drawn from
    ``[0, n_src)`` with the generator seeded by ``seed`` (duplicates are ordinary edges)."""
    import torch
    degrees = [int(d) for d in degrees]
    assert len(degrees) == n_rows and all(d >= 0 for d in degrees) and n_src > 0
    row_ptr = torch.zeros(n_rows + 1, dtype=torch.int32)
    row_ptr[1:] = torch.cumsum(torch.tensor(degrees, dtype=torch.int64), 0).to(torch.int32)
    g = torch.Generator().manual_seed(seed)
    col = torch.randint(0, n_src, (int(row_ptr[-1]),), generator=g).to(torch.int32)
    return row_ptr, col


def _edge_rows(row_ptr, n_rows):
    import torch
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(n_rows, device=row_ptr.device), deg), deg


def _read(x, ids, j):
    return x[j if ids is None else ids.long()[j]]


def _finish(C, C_abs, wt, N, bias, relu, acc_in, out_rows, n_out, abs_terms):
    """``(out, magnitude sum)`` of the tile rows ``C`` (``C_abs``: built from absolute values), placed by ``out_rows`` into
    ``n_out`` rows (rows not named: NaN in ``out``, 0 in the magnitude sum)."""
    import torch
    K = C.shape[1]
    w = wt[:, :K].double()
    assert w.shape == (N, K)
    y, mag = C @ w.t(), C_abs @ w.abs().t()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    if acc_in is not None:
        y, mag = y + acc_in.double(), mag + acc_in.double().abs()
    if abs_terms:
        y = mag
    elif relu:
        y = torch.relu(y)
    if out_rows is not None:
        n_out = int(out_rows.max()) + 1 if n_out is None else n_out
        y = torch.full((n_out, N), float("nan"), dtype=torch.float64, device=y.device).index_copy(0, out_rows, y)
        mag = torch.zeros((n_out, N), dtype=torch.float64, device=y.device).index_copy(0, out_rows, mag)
    return y, mag


def _root_rows(root, n_rows, dev):
    import torch
    x_dst, dst_rows, dst_ids = root
    rows = torch.arange(n_rows, device=dev) if dst_rows is None else dst_rows.long()
    return _read(x_dst, dst_ids, rows).double()


def hetero_sage_launch_ref(rels, n_rows, wt, N, root=None, bias=None, relu=False, acc_in=None, out_rows=None, n_out=None,
                           abs_terms=False):
    """``nn.hetero_sage_launch`` in float64.  ``rels``: ``[(row_ptr, col, x, ids, scale, mean), ...]``."""
    import torch
    dev = wt.device
    blocks, blocks_abs = [], []
    for row_ptr, col, x, ids, scale, mean in rels:
        row, deg = _edge_rows(row_ptr, n_rows)
        j = col.long()[:int(row_ptr[-1])]
        v = _read(x, ids, j).double()
        if scale is not None:
            v = v * scale.double()[j].unsqueeze(1)
        div = deg.clamp(min=1).double().unsqueeze(1) if mean else 1.0
        zero = torch.zeros((n_rows, x.shape[1]), dtype=torch.float64, device=dev)
        blocks.append(zero.index_add(0, row, v) / div)
        blocks_abs.append(zero.index_add(0, row, v.abs()) / div)
    if root is not None:
        blocks.append(_root_rows(root, n_rows, dev))
        blocks_abs.append(blocks[-1].abs())
    C, C_abs = torch.cat(blocks, 1), torch.cat(blocks_abs, 1)
    out, mag = _finish(C, C_abs, wt, N, bias, relu, acc_in, out_rows, n_out, abs_terms)
    return out, (C_abs if abs_terms else C), mag


def block_width(F, D):
    """Floats of one head block ``[x | a | 1 | 0 pad]`` (``nn.transformer_block_width``)."""
    return (F + D + 1 + 3) // 4 * 4


def hetero_transformer_launch_ref(rels, n_rows, wt, N, root=None, bias=None, relu=False, acc_in=None, out_rows=None, n_out=None,
                                  abs_terms=False):
    """``nn.hetero_transformer_launch`` in float64.  ``rels``: ``[(row_ptr, col, x, ids, edge_attr, u, w, H, alpha), ...]`` (the
    last item, the launch's alpha buffer, is not read).  Returns ``(out, A, magnitude_sum, [alpha_r [E_r, H_r]])``."""
    import torch
    dev = wt.device
    blocks, blocks_abs, alphas = [], [], []
    for row_ptr, col, x, ids, ea, u, w, H, _ in rels:
        F, D = int(x.shape[1]), 0 if ea is None else int(ea.shape[1])
        W4 = block_width(F, D)
        row, deg = _edge_rows(row_ptr, n_rows)
        E = int(row_ptr[-1])
        xj = _read(x, ids, col.long()[:E]).double()                                           # [E, F]
        s = torch.einsum("ehf,ef->eh", u.double().view(n_rows, H, F)[row], xj)
        parts = [xj]
        if D:
            a = ea.double()[:E]
            s = s + torch.einsum("ehd,ed->eh", w.double().view(n_rows, H, D)[row], a)
            parts.append(a)
        parts += [torch.ones((E, 1), dtype=torch.float64, device=dev), torch.zeros((E, W4 - F - D - 1), dtype=torch.float64, device=dev)]
        smax = torch.full((n_rows, H), -float("inf"), dtype=torch.float64, device=dev).scatter_reduce(
            0, row.unsqueeze(1).expand(E, H), s, "amax", include_self=True)
        ex = (s - smax[row]).exp()
        den = torch.zeros((n_rows, H), dtype=torch.float64, device=dev).index_add(0, row, ex)
        alpha = ex / den[row]
        ext = torch.cat(parts, 1)                                                             # [E, W4]
        zero = torch.zeros((n_rows, H, W4), dtype=torch.float64, device=dev)
        blocks.append(zero.index_add(0, row, alpha.unsqueeze(2) * ext.unsqueeze(1)).reshape(n_rows, H * W4))
        blocks_abs.append(zero.index_add(0, row, alpha.unsqueeze(2) * ext.abs().unsqueeze(1)).reshape(n_rows, H * W4))
        alphas.append(alpha)
    if root is not None:
        blocks.append(_root_rows(root, n_rows, dev))
        blocks_abs.append(blocks[-1].abs())
    A, A_abs = torch.cat(blocks, 1), torch.cat(blocks_abs, 1)
    out, mag = _finish(A, A_abs, wt, N, bias, relu, acc_in, out_rows, n_out, abs_terms)
    return out, (A_abs if abs_terms else A), mag, alphas
