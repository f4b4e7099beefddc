"""Grouped Linear on the device (csrc/wg_grouped_linear.hip through ``wholegraph_amd.nn``: ``grouped_linear``, ``HeteroLinear``,
``HeteroDictLinear``) against the float64 restatement of tests/grouped_linear_ref.py.

Bound, element-wise and the project's own for every product (tests/test_gpu_row_linear.py): ``|got - ref| <= 1e-5 x sum|terms|``
for the forward and for dX, dW, db and d add against each gradient's own sum of absolute terms.  With ReLU the reference takes
the mask from the kernel route's own output (``out > 0``), so no element is left out of any comparison."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_linear_ref import grouped_linear_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = (0, 1, 15, 16, 17, 63, 64, 65, 130)      # around the 16-row wave tile and the 64-row workgroup tile; an empty segment


def _inputs(ns, Ks, N, layout, seed=0, extra_rows=0):
    """Per segment x [n + extra_rows, K], w (a product is O(1)), b, add [n, N], grad_out [n, N]: float32 leaves on the device."""
    g = torch.Generator().manual_seed(1000 * N + sum(Ks) + seed)
    leaf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda().requires_grad_(True)      # noqa: E731
    xs = [leaf(n + extra_rows, K) for n, K in zip(ns, Ks)]
    ws = [leaf(*((N, K) if layout == "nk" else (K, N)), scale=K ** -0.5) for K in Ks]
    bs, adds = [leaf(N) for _ in ns], [leaf(n, N) for n in ns]
    return xs, ws, bs, adds, [torch.randn(n, N, generator=g).cuda() for n in ns]


def _check(got, ref, name, tag):
    err, bound = (got.detach().double().cpu() - ref[name]).abs(), 1e-5 * ref[name + "_terms"]
    assert got.shape == ref[name].shape and bool((err <= bound).all()), "%s %s: worst |err| / bound = %g" % (
        tag, name, float((err / (bound + 1e-300)).max()))


def _check_segments(xs, ws, bs, adds, gos, outs, layout, relu, rows=None):
    for k in range(len(xs)):
        ref = grouped_linear_ref(xs[k], ws[k], bs[k], None if adds is None else adds[k], gos[k], layout,
                                 None if rows is None else rows[k], (outs[k].detach() > 0) if relu else None)
        named = [(outs[k], "out"), (xs[k].grad, "dx"), (ws[k].grad, "dw"), (bs[k].grad, "db")]
        for got, name in named + ([] if adds is None else [(adds[k].grad, "dadd")]):
            _check(got, ref, name, "segment %d" % k)


@pytest.mark.parametrize("relu,use_add", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("K,N", [(4, 4), (20, 12), (64, 64), (36, 272), (260, 20)])
def test_grouped_linear_against_float64(K, N, layout, relu, use_add):
    from wholegraph_amd import nn
    xs, ws, bs, adds, gos = _inputs(ROWS, [K] * len(ROWS), N, layout)
    adds = adds if use_add else None
    before = nn.grouped_linear_launches
    outs = nn.grouped_linear(xs, ws, bs, adds=adds, relu=relu, weight_layout=layout)
    assert nn.grouped_linear.route == "kernel" and nn.grouped_linear_launches == before + 1
    torch.autograd.backward(outs, gos)
    _check_segments(xs, ws, bs, adds, gos, outs, layout, relu)


def test_mixed_widths_rows_and_launch_count():
    from wholegraph_amd import nn
    Ks, ns = (8, 132, 64), (70, 40, 33)
    xs, ws, bs, adds, gos = _inputs(ns, Ks, 32, "nk", extra_rows=5)
    rows = [torch.arange(70).cuda(), torch.randint(0, 45, (40,), generator=torch.Generator().manual_seed(2)).cuda(),
            torch.randperm(38, generator=torch.Generator().manual_seed(3))[:33].cuda()]
    outs = nn.grouped_linear(xs, ws, bs, rows=rows, adds=adds, relu=True)
    assert nn.grouped_linear.route == "kernel"
    torch.autograd.backward(outs, gos)
    _check_segments(xs, ws, bs, adds, gos, outs, "nk", True, rows)
    x17, w17 = {k: xs[0].detach() for k in range(17)}, {k: ws[0].detach() for k in range(17)}
    before = nn.grouped_linear_launches
    out17 = nn.grouped_linear(x17, w17)
    assert nn.grouped_linear_launches == before + 2 and list(out17) == list(range(17))
    assert all(torch.equal(out17[k], out17[0]) for k in range(17))


@pytest.mark.parametrize("with_rows", [False, True])
def test_lazy_rows_read_through_their_ids(with_rows):
    from wholegraph_amd import nn
    (table,), ws, bs, _, _ = _inputs((50,), (20,), 12, "nk", seed=7)
    table = table.detach()
    ids = torch.randint(0, 50, (70,), generator=torch.Generator().manual_seed(8)).cuda()      # repeats
    rows = torch.randint(0, 70, (33,), generator=torch.Generator().manual_seed(9)).cuda() if with_rows else None
    go = torch.randn(33 if with_rows else 70, 12, generator=torch.Generator().manual_seed(10)).cuda()
    before = nn.grouped_linear_launches
    out, = nn.grouped_linear([nn.LazyRows(table, ids)], ws, bs, rows=[rows], relu=True)
    assert nn.grouped_linear.route == "kernel" and nn.grouped_linear_launches == before + 1
    out.backward(go)
    ref = grouped_linear_ref(table, ws[0], bs[0], None, go, "nk", ids[rows] if with_rows else ids, out.detach() > 0)
    for got, name in ((out, "out"), (ws[0].grad, "dw"), (bs[0].grad, "db")):
        _check(got, ref, name, "lazy")
    with pytest.raises(NotImplementedError):      # a lazily read table never gets a gradient
        nn.grouped_linear([nn.LazyRows(table.requires_grad_(True), ids)], ws, bs, rows=[rows])


@pytest.mark.parametrize("relu", [False, True])
def test_hetero_linear_sorted_unsorted_and_out_view(relu):
    from wholegraph_amd import nn
    torch.manual_seed(4)
    T, K, N, ptr = 5, 36, 20, [0, 70, 70, 87, 152, 153]      # type 1 is empty
    m = nn.HeteroLinear(K, N, T).cuda()
    tv = torch.repeat_interleave(torch.arange(T), torch.tensor([b - a for a, b in zip(ptr, ptr[1:])])).cuda()
    x, go = torch.randn(153, K).cuda().requires_grad_(True), torch.randn(153, N).cuda()
    f0, b0 = nn.grouped_linear_launches, nn.grouped_linear_backward_launches
    out = m(x, tv, ptr=ptr, relu=relu)
    out.backward(go)
    assert m.route == "kernel" and nn.grouped_linear_launches == f0 + 1 and nn.grouped_linear_backward_launches == b0 + 3

    def check(x, tv, go, out):      # sort by type, apply per type in float64, unsort
        order = torch.argsort(tv, stable=True)
        for t in range(T):
            idx = order[ptr[t]:ptr[t + 1]]
            ref = grouped_linear_ref(x[idx], m.weight[t], m.bias[t], None, go[idx], "kn", None, (out[idx].detach() > 0) if relu else None)
            for got, name in ((out[idx], "out"), (x.grad[idx], "dx"), (m.weight.grad[t], "dw"), (m.bias.grad[t], "db")):
                _check(got, ref, name, "type %d" % t)
    check(x, tv, go, out)
    # an unsorted type_vec
    shuffle = torch.randperm(153).cuda()
    x2 = x.detach()[shuffle].requires_grad_(True)
    m.zero_grad()
    out2 = m(x2, tv[shuffle], relu=relu)
    out2.backward(go[shuffle])
    assert m.route == "kernel"
    check(x2, tv[shuffle], go[shuffle], out2)
    # a slab of sentinel rows and columns around an `out` view stays untouched
    slab = torch.full((153 + 16, N + 8), 7.5).cuda()
    view = slab[8:161, 4:4 + N]
    nn.grouped_linear_forward(nn._HeteroLinear.descs(x2.detach(), m.weight.detach(), m.bias.detach(), view, ptr,
                                                     torch.argsort(tv[shuffle], stable=True)), relu)
    assert torch.equal(view, out2)
    slab[8:161, 4:4 + N] = 7.5
    assert bool((slab == 7.5).all())


def test_hetero_dict_linear_loads_hgt_projection():
    from wholegraph_amd import nn
    torch.manual_seed(5)
    conv = nn.HGTConv({"paper": 36, "author": 20}, 16, (["paper", "author"], [("author", "writes", "paper")]), heads=2).cuda()
    m = nn.HeteroDictLinear({"paper": 36, "author": 20}, 48).cuda()
    m.load_state_dict(conv.kqv_lin.state_dict(), strict=True)
    x = {"author": torch.randn(70, 20).cuda()}
    out = m(x)
    assert m.route == "kernel" and list(out) == ["author"]
    lin = conv.kqv_lin["author"]
    ref = grouped_linear_ref(x["author"], lin.weight, lin.bias, None, torch.zeros(70, 48))
    _check(out["author"], ref, "out", "author")
    with torch.no_grad():      # torch.nn.functional.linear itself, in float64
        want = torch.nn.functional.linear(x["author"].double(), lin.weight.double(), lin.bias.double())
    assert bool(((out["author"].double() - want).abs().cpu() <= 1e-5 * ref["out_terms"]).all())


def test_same_bits_on_every_run():
    from wholegraph_amd import nn
    runs = []
    for _ in range(2):
        xs, ws, bs, adds, gos = _inputs((5000, 130, 64), (260, 36, 64), 272, "kn", seed=9)
        outs = nn.grouped_linear(xs, ws, bs, adds=adds, relu=True, weight_layout="kn")
        torch.autograd.backward(outs, gos)
        runs.append([t.detach().clone() for t in outs] + [t.grad.clone() for t in xs + ws + bs + adds])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("case", ["width", "float64", "torch_ops"])
def test_torch_route_cases(case):
    from wholegraph_amd import nn
    K, N = (6, 8) if case == "width" else (8, 8)
    m = nn.HeteroDictLinear({"a": K, "b": K}, N).cuda()
    m.torch_ops = case == "torch_ops"
    dt = torch.float64 if case == "float64" else torch.float32
    m = m.to(dt)
    x = {t: torch.randn(33, K, dtype=dt).cuda().requires_grad_(True) for t in ("a", "b")}
    go = torch.randn(33, N, dtype=dt).cuda()
    out = m(x, relu=True)
    assert m.route == "torch"
    torch.autograd.backward([out["a"], out["b"]], [go, go])
    for t in ("a", "b"):
        lin = m.lins[t]
        ref = grouped_linear_ref(x[t], lin.weight, lin.bias, None, go, "nk", None, out[t].detach() > 0)
        for got, name in ((out[t], "out"), (x[t].grad, "dx"), (lin.weight.grad, "dw"), (lin.bias.grad, "db")):
            if case == "float64":
                assert float((got.detach().cpu() - ref[name]).abs().max()) <= 1e-12 * max(1.0, float(ref[name].abs().max())), name
            else:
                _check(got, ref, name, t)


def test_double_backward_agrees_with_torch_route():
    from wholegraph_amd import nn
    res = []
    for torch_ops in (False, True):
        torch.manual_seed(6)
        m = nn.HeteroDictLinear({"a": 36}, 20).cuda()
        m.torch_ops = torch_ops
        x = torch.randn(70, 36).cuda().requires_grad_(True)
        out = m({"a": x}, relu=True)["a"]
        assert m.route == ("torch" if torch_ops else "kernel")
        gx, = torch.autograd.grad(out.square().sum(), x, create_graph=True)
        gx.square().sum().backward()
        res.append((gx.detach(), x.grad, m.lins["a"].weight.grad))
    for got, want in zip(*res):
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
