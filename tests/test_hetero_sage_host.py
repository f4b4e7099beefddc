"""nn.HeteroConv over SAGEConv relations, the parts that need no GPU: the layer on CPU tensors (the library-ops route) against
the float64 restatement of tests/hetero_sage_ref.py, the launch planner of the one-kernel route, and what the layer refuses."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_sage_ref as ref  # noqa: E402


def csr(n_rows, n_src, degs, g):
    rp = torch.zeros(n_rows + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(torch.as_tensor(degs), 0)
    col = torch.randint(0, n_src, (int(rp[-1]),), generator=g, dtype=torch.int32)
    return rp, col


def hand_built(g):
    """Three node types, five relations, two hops; widths a: 12, b: 8, c: 6; the relation c -> a has no edges at all, and
    hop 1 of type ``a`` writes interleaved output rows."""
    from wholegraph_amd import nn
    n_in = {"a": 11, "b": 9, "c": 7}          # rows of the layer's input per type
    n_out = {"a": 7, "b": 4, "c": 0}
    ets = [("a", "to", "a"), ("b", "to", "a"), ("c", "to", "a"), ("a", "to", "b"), ("c", "to", "b")]
    rels = []
    # hop 0: type a rows 0, 2, 4, 6 of the output (3 entries ... ) and hop 1: the others — interleaved
    a0, a1 = torch.tensor([0, 2, 4, 6]), torch.tensor([1, 3, 5])
    dst_a0, dst_a1 = torch.tensor([0, 1, 2, 3]), torch.tensor([7, 5, 9])
    b0 = torch.tensor([2, 0, 3, 1])
    dst_b0 = torch.tensor([4, 0, 8, 2])
    for hop, rows, dst in ((0, a0, dst_a0), (1, a1, dst_a1)):
        n = len(rows)
        for et in ets[:3]:
            if et[0] == "c":
                degs = [0] * n
            else:
                degs = [int(v) for v in torch.randint(0, 4, (n,), generator=g)]
            rp, col = csr(n, n_in[et[0]], degs, g)
            rels.append(nn.RelationHop(et, hop, rp, col, dst, rows, int(rp[-1]), 3))
    for et in ets[3:]:
        degs = [2, 0, 3, 1]
        rp, col = csr(4, n_in[et[0]], degs, g)
        rels.append(nn.RelationHop(et, 1, rp, col, dst_b0, b0, int(rp[-1]), 3))
    return nn.HeteroLayerGraph(rels, n_out, ["a", "b", "c"]), n_in, ets


def make_layer(ets, widths, N):
    from wholegraph_amd import nn
    convs = {}
    for k, et in enumerate(ets):
        convs[et] = nn.SAGEConv((widths[et[0]], widths[et[2]]), N, aggr="sum" if k == 1 else "mean", root_weight=k != 3)
    return nn.HeteroConv(convs)


def test_cpu_layer_matches_float64_restatement_outputs_and_gradients():
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(5)
    graph, n_in, ets = hand_built(g)
    widths = {"a": 12, "b": 8, "c": 6}
    torch.manual_seed(1)
    layer = make_layer(ets, widths, 10)
    launches = nn.hetero_sage_launches
    xs = {t: torch.randn((n_in[t], widths[t]), generator=g) for t in n_in}
    for relu in (False, True):
        for p in layer.parameters():
            p.grad = None
        out = layer(xs, graph, act="relu" if relu else None)
        assert set(out) == {"a", "b"} and out["a"].shape == (7, 10) and out["b"].shape == (4, 10)
        gout = {t: torch.randn(out[t].shape, generator=g) for t in out}
        sum((out[t] * gout[t]).sum() for t in out).backward()
        p64 = ref.params_of(layer)
        leaves = {}
        for et, p in p64.items():
            for k in ("Wl", "bl", "Wr"):
                if p[k] is not None:
                    p[k] = leaves[(et, k)] = p[k].double().requires_grad_(True)
        want = ref.hetero_sage_forward(xs, graph, p64, relu=relu)
        sum((want[t] * gout[t].double()).sum() for t in want).backward()
        for t in out:
            assert float((out[t].detach().double() - want[t].detach()).abs().max()) <= 1e-5 * float(want[t].detach().abs().max()), t
        for (et, k), leaf in leaves.items():
            c = layer.conv(et)
            got = {"Wl": c.lin_l.weight, "bl": c.lin_l.bias, "Wr": None if c.lin_r is None else c.lin_r.weight}[k].grad
            assert got is not None, (et, k)
            assert float((got.double() - leaf.grad).abs().max()) <= 1e-5 * max(float(leaf.grad.abs().max()), 1e-30), (et, k)
    assert nn.hetero_sage_launches == launches    # CPU tensors: the library-ops route


@pytest.mark.parametrize("widths,F_dst,want", [
    ([128, 128, 128], 128, [(0, 3, True)]),                               # fits one launch
    ([256, 256, 256, 256], 256, [(0, 4, False), (4, 4, True)]),           # mag's paper at a hidden width of 256: 5 blocks
    ([256, 256, 256, 256, 256], 0, [(0, 4, False), (4, 5, False)]),
    ([128, 1024, 64], 64, [(0, 1, False), (1, 2, False), (2, 3, True)]),  # one relation wider than the rest
    ([4] * 9, 4, [(0, 8, False), (8, 9, True)]),                          # more relations than one launch describes
    ([], 64, [(0, 0, True)]),
])
def test_launch_planner(widths, F_dst, want):
    from wholegraph_amd import nn
    plan = nn.hetero_sage_plan(widths, F_dst)
    assert plan == want
    at = 0
    for k, (lo, hi, root) in enumerate(plan):
        assert lo == at and hi >= lo and hi - lo <= 8            # whole relations, in order, nothing skipped
        assert sum(widths[lo:hi]) + (F_dst if root else 0) <= 1024
        assert not root or k == len(plan) - 1                     # the root (with bias, ReLU, placement) on the last launch only
        at = hi
    assert at == len(widths) and (F_dst == 0 or plan[-1][2])


def test_launch_planner_refuses_a_block_wider_than_a_launch():
    from wholegraph_amd import nn
    with pytest.raises(ValueError):
        nn.hetero_sage_plan([128, 1028], 64)
    with pytest.raises(ValueError):
        nn.hetero_sage_plan([128], 2048)


def test_mixed_layer_classes_and_other_activations_are_refused():
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(2)
    graph, n_in, ets = hand_built(g)
    widths = {"a": 12, "b": 12, "c": 12}
    xs = {t: torch.randn((n_in[t], 12), generator=g) for t in n_in}
    mix = nn.HeteroConv({et: (nn.GATConv(12, 4, heads=1, add_self_loops=False) if k == 0 else nn.SAGEConv(12, 4))
                         for k, et in enumerate(ets)})
    with pytest.raises(NotImplementedError, match="GATConv.*SAGEConv"):
        mix(xs, graph)
    layer = make_layer(ets, widths, 4)
    with pytest.raises(ValueError, match="act"):
        layer(xs, graph, act="tanh")


def test_no_gradient_flows_into_a_lazy_table():
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(3)
    graph, n_in, ets = hand_built(g)
    widths = {"a": 12, "b": 8, "c": 6}
    layer = make_layer(ets, widths, 4)
    xs = {t: torch.randn((n_in[t], widths[t]), generator=g) for t in n_in}
    table = torch.randn((40, 12), generator=g).requires_grad_(True)
    xs["a"] = nn.LazyRows(table, torch.randint(0, 40, (n_in["a"],), generator=g))
    with pytest.raises(NotImplementedError, match="LazyRows"):
        layer(xs, graph)
