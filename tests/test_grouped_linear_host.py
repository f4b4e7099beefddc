"""Grouped Linear without a GPU: the torch route of ``grouped_linear``, ``HeteroDictLinear`` and ``HeteroLinear`` on CPU tensors
against the float64 restatement (tests/grouped_linear_ref.py), the modules' state-dict keys and shapes, and the argument
checks."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_linear_ref import grouped_linear_ref  # noqa: E402


def _close(got, ref, name):
    assert bool(((got.double() - ref[name]).abs() <= 1e-5 * ref[name + "_terms"]).all()), name


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("relu", [False, True])
def test_torch_route_matches_float64(layout, relu):
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(1)
    shapes = [(0, 8, 12), (5, 6, 8), (33, 20, 12)]
    xs = [torch.randn(n + 3, K, generator=g).requires_grad_(True) for n, K, N in shapes]
    ws = [torch.randn((N, K) if layout == "nk" else (K, N), generator=g).requires_grad_(True) for n, K, N in shapes]
    bs = [torch.randn(N, generator=g).requires_grad_(True) for n, K, N in shapes]
    adds = [torch.randn(n, N, generator=g).requires_grad_(True) for n, K, N in shapes]
    rows = [torch.randint(0, n + 3, (n,), generator=g) for n, K, N in shapes]
    gos = [torch.randn(n, N, generator=g) for n, K, N in shapes]
    outs = nn.grouped_linear(xs, ws, bs, rows=rows, adds=adds, relu=relu, weight_layout=layout)
    assert nn.grouped_linear.route == "torch" and isinstance(outs, list)
    torch.autograd.backward(outs, gos)
    for k in range(len(shapes)):
        ref = grouped_linear_ref(xs[k], ws[k], bs[k], adds[k], gos[k], layout, rows[k], (outs[k].detach() > 0) if relu else None)
        for got, name in ((outs[k].detach(), "out"), (xs[k].grad, "dx"), (ws[k].grad, "dw"), (bs[k].grad, "db"), (adds[k].grad, "dadd")):
            _close(got, ref, name)


def test_modules_keys_shapes_and_torch_route():
    from wholegraph_amd import nn
    m = nn.HeteroDictLinear({"paper": 12, "author": 8}, 16)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "lins.paper.weight": (16, 12), "lins.paper.bias": (16,), "lins.author.weight": (16, 8), "lins.author.bias": (16,)}
    assert list(nn.HeteroDictLinear(4, 8, types=["a", "b"], bias=False).state_dict()) == ["lins.a.weight", "lins.b.weight"]
    x = {"author": torch.randn(7, 8)}
    out = m(x, relu=True)
    assert m.route == "torch" and list(out) == ["author"]
    assert torch.allclose(out["author"], torch.nn.functional.linear(x["author"], m.lins["author"].weight, m.lins["author"].bias).relu())
    h = nn.HeteroLinear(8, 12, 3)
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == {"weight": (3, 8, 12), "bias": (3, 12)}
    assert list(nn.HeteroLinear(8, 12, 3, bias=False).state_dict()) == ["weight"]
    xv, tv = torch.randn(9, 8), torch.tensor([2, 0, 0, 2, 2, 0, 2, 0, 0])      # (type 1 is empty)
    got = h(xv, tv)
    want = torch.stack([xv[i] @ h.weight[tv[i]] + h.bias[tv[i]] for i in range(9)])
    assert h.route == "torch" and torch.allclose(got, want, atol=1e-6)
    srt = torch.argsort(tv, stable=True)
    assert torch.equal(h(xv[srt], tv[srt], ptr=[0, 5, 5, 9]), got[srt])


def test_argument_checks():
    from wholegraph_amd import nn
    with pytest.raises(ValueError, match="does not match weight"):
        nn.grouped_linear([torch.randn(3, 8)], [torch.randn(4, 12)])
    with pytest.raises(ValueError, match="does not match weight"):
        nn.grouped_linear([torch.randn(3, 8)], [torch.randn(4, 8)], weight_layout="kn")
    with pytest.raises(ValueError, match="weight_layout"):
        nn.grouped_linear([torch.randn(3, 8)], [torch.randn(4, 8)], weight_layout="t")
    h = nn.HeteroLinear(8, 4, 3)
    with pytest.raises(ValueError, match="in_channels"):
        h(torch.randn(3, 12), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="outside 0 .. 2"):
        h(torch.randn(3, 8), torch.tensor([0, 3, 1]))
    with pytest.raises(ValueError, match="ptr has 3 entries"):
        h(torch.randn(3, 8), torch.tensor([0, 1, 2]), ptr=[0, 1, 3])
    with pytest.raises(ValueError, match="types"):
        nn.HeteroDictLinear(8, 4)
