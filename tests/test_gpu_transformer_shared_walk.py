"""The two users of the transformer row walk (tconv_row_walk, csrc/wg_transformer_parts.hpp) agree bit for bit: one relation
through ``nn.hetero_transformer_launch`` (wgamd_hetero_transformer_layer_f32_train) against ``nn.transformer_layer_forward``
(wgamd_transformer_layer_f32) on the same CSR, u, w, wt, bias and ReLU — ``out``, ``alpha`` and the kept rows ``A`` must be
``torch.equal``.  37 rows are three tiles, the last with 5 rows; the row degrees cover the group-of-4 boundaries (0, 1, 4, 5, 9)
and, with one row of 70 edges, the 64-lane stride of the alpha pass; F = 20 leaves 5 lanes with a float4 of the source row."""
import functools
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_ROWS, F, F_DST, N, N_SRC = 37, 20, 8, 32, 53


@functools.lru_cache(maxsize=None)
def hop():
    """The CSR, the source and destination rows and the node lists, made once and left unchanged."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    deg = [[0, 1, 4, 5, 9, 3, 8][i % 7] for i in range(N_ROWS)]
    deg[17] = 70
    assert {0, 1, 4, 5, 9, 70} <= set(deg) and deg[N_ROWS - 1] > 0
    row_ptr = torch.zeros(N_ROWS + 1, dtype=torch.int32, device=dev)
    row_ptr[1:] = torch.cumsum(torch.tensor(deg, device=dev), 0).to(torch.int32)
    E = int(row_ptr[-1])
    col = torch.randint(0, N_SRC, (E,), generator=g, device=dev).to(torch.int32)
    table = torch.randn((200, F), generator=g, device=dev)           # the lazy source type: rows ids[j] of a table
    ids = torch.randperm(200, generator=g, device=dev)[:N_SRC].contiguous()
    x_dst = torch.randn((60, F_DST), generator=g, device=dev)
    dst_rows = torch.randperm(60, generator=g, device=dev)[:N_ROWS].contiguous()
    return dict(row_ptr=row_ptr, col=col, E=E, table=table, ids=ids, x=table[ids].contiguous(), x_dst=x_dst, dst_rows=dst_rows)


@pytest.mark.parametrize("source", ["resident", "int32", "int64"])
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("D", [0, 3])
def test_hetero_launch_equals_layer_forward_bit_for_bit(hiplib, D, H, source):
    import torch
    from wholegraph_amd import nn
    h = hop()
    dev = h["row_ptr"].device
    g = torch.Generator(device=dev).manual_seed(100 * D + 10 * H)
    K = H * nn.transformer_block_width(F, D) + F_DST
    u = torch.randn((N_ROWS, H * F), generator=g, device=dev) * 0.3
    w = torch.randn((N_ROWS, H * D), generator=g, device=dev) * 0.3 if D else None
    ea = torch.randn((h["E"], D), generator=g, device=dev) if D else None
    wt = torch.randn((N, K), generator=g, device=dev) * 0.1
    bias = torch.randn(N, generator=g, device=dev)
    x, ids = (h["x"], None) if source == "resident" else (h["table"], h["ids"].to(torch.int32 if source == "int32" else torch.int64))
    for relu in (False, True):
        alpha = [torch.full((h["E"], H), 7.0, device=dev) for _ in range(2)]
        A = [torch.full((N_ROWS, K), 7.0, device=dev) for _ in range(2)]
        before = nn.hetero_transformer_launches
        got = nn.hetero_transformer_launch([(h["row_ptr"], h["col"], x, ids, ea, u, w, H, alpha[0])], N_ROWS, wt, N,
                                           root=(h["x_dst"], h["dst_rows"], None), bias=bias, relu=relu, a_save=A[0])
        assert nn.hetero_transformer_launches - before == 1
        want = nn.transformer_layer_forward(h["row_ptr"], h["col"], x, u, wt, H, self_rows=h["dst_rows"], x_dst=h["x_dst"],
                                            edge_attr=ea, w=w, bias=bias, relu=relu, src_ids=ids, alpha=alpha[1], a_save=A[1])
        tag = (D, H, source, relu)
        assert torch.equal(A[0], A[1]), tag
        assert torch.equal(alpha[0], alpha[1]), tag
        assert torch.equal(got, want), tag
        assert bool(torch.isfinite(got).all()) and float(alpha[0].min()) >= 0.0 and float(alpha[0].max()) <= 1.0, tag
