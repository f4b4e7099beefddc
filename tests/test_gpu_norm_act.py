"""NormDropoutAct on the device (csrc/wg_norm_act.hip through ``wholegraph_amd.nn``) against the float64 restatement of
tests/norm_act_ref.py.

Forward bound, element-wise: ``|got - ref| <= 1e-5 (|w_c| (1 + |x^_rc|) kappa_r + |b_c|) / (1 - p)`` with ``kappa_r = max(1,
max_c |z_rc| / sigma_r)`` (``norm_act_ref.forward_bound``).  Whether the constant is fair was measured with torch's own float32
``F.layer_norm`` on the CPU over the inputs of this file (every shape of ``SHAPES`` with and without residual, and the rows of
``test_ill_conditioned_rows``): its largest error is 0.0074 of the bound (TORCH_F32_RATIO below, re-measured by
``test_bound_is_fair_to_torch_float32`` on every run), far under half of it, so the constant stays at 1e-5.  Gradients:
``|got - ref| <= 1e-5 x`` the sum of the magnitudes of the terms the element adds up (``dz_terms`` etc.).  Elements whose ReLU
sign float32 cannot decide (``|y_ref| < 1e-5 (|w_c| + |b_c|)``) are left out of the dz comparison and the reference takes the
kernel's sign there; they have to stay under 0.1 % of the elements (with |bias| >= 0.05 the float64 reference leaves out at most
9 of the 1 024 000 elements of the largest case and at most 0.004 % of any; ``test_undecided_elements_are_rare`` counts on the
CPU).
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_act_ref import forward_bound, norm_act_ref, undecided  # noqa: E402

SHAPES = [(n, C) for n in (1, 3, 64, 257, 1000) for C in (4, 36, 64, 100, 256, 260, 1024)]
EPS = 1e-5
TORCH_F32_RATIO = 0.0074     # measured: torch float32 F.layer_norm's largest |error| / bound over this file's inputs (CPU)

# (residual, norm, relu, weight, bias, column-sliced views, p)
MODES = [
    (True, True, True, True, True, False, 0.5),
    (False, True, True, True, True, False, 0.0),
    (True, True, False, True, False, False, 0.0),
    (False, False, True, False, False, False, 0.5),
    (True, False, False, False, False, False, 0.0),
    (True, True, True, True, True, True, 0.5),
    (False, True, True, False, False, False, 0.0),
    (False, True, False, False, True, True, 0.25),
]


def make_inputs(n, C, device, seed=0):
    """x, residual, weight, bias (|bias| >= 0.05), grad_out: float32 randn, the same for a given (n, C, seed) on every device."""
    g = torch.Generator().manual_seed(1000 * n + C + seed)
    x, res, go = (torch.randn(n, C, generator=g) for _ in range(3))
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    b = torch.where(b >= 0, 0.05 + 0.5 * b.abs(), -0.05 - 0.5 * b.abs())
    return tuple(t.to(device) for t in (x, res, w, b, go))


def ill_conditioned_rows(C, device):
    """Row 0: mean 1e3, sigma 1 (a one-pass variance loses it all); row 1: constant; the rest randn."""
    g = torch.Generator().manual_seed(C)
    x = torch.randn(8, C, generator=g)
    x[0] += 1e3
    x[1] = 0.37
    return x.to(device)


def _wide(t, pad=8):
    """``t`` as a column-sliced view of a wider tensor: rows ``C + pad`` floats apart, starting 16 B into the row."""
    big = torch.full((t.shape[0], t.shape[1] + pad), 7.0, dtype=t.dtype, device=t.device)
    big[:, 4:4 + t.shape[1]] = t
    return big[:, 4:4 + t.shape[1]]


def _keep(nn, n, C, p, seed, wide=False):
    ones = torch.ones(n, C, device="cuda")
    out = nn.norm_dropout_act(_wide(ones) if wide else ones, norm=False, relu=False, p=p, training=True, seed=seed)
    scale = (torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
    assert bool(((out == 0) | (out == float(scale))).all()), "kept elements carry 1 / (1 - p) in float32"
    return out != 0


def _check_mode(nn, n, C, mode):
    has_res, norm, relu, has_w, has_b, views, p = mode
    x, res, w, b, go = make_inputs(n, C, "cuda")
    seed = 77 + n + C
    keep = _keep(nn, n, C, p, seed) if p > 0 else None
    leaf = lambda t: (_wide(t) if views and t.dim() == 2 else t.clone()).requires_grad_(True)      # noqa: E731
    xg, rg = leaf(x), leaf(res) if has_res else None
    wg, bg = leaf(w) if has_w and norm else None, leaf(b) if has_b and norm else None
    out = nn.norm_dropout_act(xg, wg, bg, residual=rg, norm=norm, eps=EPS, p=p, training=True, relu=relu, seed=seed)
    assert out.shape == (n, C) and out.dtype == torch.float32
    out.backward(go)
    kw = dict(residual=res if has_res else None, weight=w if has_w else None, bias=b if has_b else None, keep=keep, p=p, norm=norm,
              relu=relu, eps=EPS)
    ref = norm_act_ref(x, **kw)
    und = undecided(ref) & bool(relu)
    assert int(und.sum()) <= 1e-3 * und.numel(), (int(und.sum()), und.numel())
    sign = torch.where(und, out.detach() > 0, ref["y"] > 0) if relu else None
    ref = norm_act_ref(x, relu_sign=sign, grad_out=go, **kw)
    tag = "n=%d C=%d mode=%s" % (n, C, mode)
    err = (out.detach().double() - ref["out"]).abs()
    assert bool((err <= forward_bound(ref, p)).all()), ("forward", tag, float((err / forward_bound(ref, p)).max()))
    dz = xg.grad
    assert dz is not None and dz.shape == (n, C)
    if has_res:
        assert torch.equal(dz, rg.grad), "dz is the gradient of x and of the residual"
    err = (dz.double() - ref["dz"]).abs()
    assert bool(((err <= 1e-5 * ref["dz_terms"]) | und).all()), ("dz", tag, float((err / (1e-5 * ref["dz_terms"] + 1e-300))[~und].max()))
    if wg is not None:
        err = (wg.grad.double() - ref["dw"]).abs()
        assert bool((err <= 1e-5 * ref["dw_terms"]).all()), ("dweight", tag, float((err / (1e-5 * ref["dw_terms"] + 1e-300)).max()))
    if bg is not None:
        err = (bg.grad.double() - ref["db"]).abs()
        assert bool((err <= 1e-5 * ref["db_terms"]).all()), ("dbias", tag, float((err / (1e-5 * ref["db_terms"] + 1e-300)).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("n,C", SHAPES)
def test_forward_and_gradients_against_float64(hiplib, n, C):
    from wholegraph_amd import nn
    for mode in MODES:
        _check_mode(nn, n, C, mode)


@pytest.mark.gpu
def test_module_takes_the_kernel_route_and_empty_input(hiplib):
    from wholegraph_amd import nn
    m = nn.NormDropoutAct(64, p=0.5).cuda()
    x = torch.randn(10, 64, device="cuda")
    before = nn.norm_act_launches
    m(x, seed=1)
    assert m.route == "kernel" and nn.norm_act_launches == before + 1
    plain = nn.NormDropoutAct(64, elementwise_affine=False).cuda()
    plain(x.double())
    assert plain.route == "torch"
    plain(torch.randn(64, 10, device="cuda").t())            # column stride != 1
    assert plain.route == "torch"
    plain(x)
    assert plain.route == "kernel"
    assert nn.NormDropoutAct(68).cuda()(torch.randn(4, 68, device="cuda")) is not None
    big = nn.NormDropoutAct(1028).cuda()
    big(torch.randn(4, 1028, device="cuda"))
    assert big.route == "torch"                              # a width outside norm_dropout_act_supported
    # n = 0: an empty result, zero parameter gradients, no fault
    x0 = torch.zeros(0, 64, device="cuda", requires_grad=True)
    out = m(x0, torch.zeros(0, 64, device="cuda"), seed=3)
    assert out.shape == (0, 64) and m.route == "kernel"
    out.sum().backward()
    assert x0.grad.shape == (0, 64) and torch.equal(m.weight.grad, torch.zeros(64, device="cuda"))
    assert torch.equal(m.bias.grad, torch.zeros(64, device="cuda"))
    # norm=False without residual or active dropout is torch.relu: no launch
    before = nn.norm_act_launches
    plain = nn.NormDropoutAct(64, norm=False, p=0.5).cuda().eval()
    assert torch.equal(plain(x), torch.relu(x)) and nn.norm_act_launches == before and plain.route == "torch"


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 260])
def test_ill_conditioned_rows(hiplib, C):
    """A row with mean 1e3 and sigma 1 (E[z^2] - mean^2 in float32 would lose the variance) and a constant row: rstd = eps^-1/2,
    out = relu(bias), dz finite."""
    from wholegraph_amd import nn
    x = ill_conditioned_rows(C, "cuda")
    _, _, w, b, go = make_inputs(8, C, "cuda")
    outs, stats = nn.norm_act_forward([(x, None, w, b)], True, True, EPS, 0.0, 0, save_stats=True)
    ref = norm_act_ref(x, weight=w, bias=b, eps=EPS, grad_out=go)
    err = (outs[0].double() - ref["out"]).abs()
    assert bool((err <= forward_bound(ref)).all()), float((err / forward_bound(ref)).max())
    assert abs(float(stats[0][0, 0]) - float(x[0].double().mean())) <= 1e-3
    assert abs(float(stats[0][0, 1]) / float(1.0 / x[0].double().std(unbiased=False)) - 1.0) <= 1e-3
    assert abs(float(stats[0][1, 1]) * math.sqrt(EPS) - 1.0) <= 1e-3
    assert bool((outs[0][1].double() - torch.relu(b.double())).abs().le(forward_bound(ref)[1]).all())
    xg = x.clone().requires_grad_(True)
    nn.norm_dropout_act(xg, w, b, eps=EPS).backward(go)
    assert bool(torch.isfinite(xg.grad).all())


def test_bound_is_fair_to_torch_float32():
    """torch's own float32 layer_norm (CPU) through the forward bound on this file's inputs: it has to stay under half of it,
    or the constant would have to be widened to twice its ratio (see the docstring).  Prints the ratio."""
    worst = 0.0
    cases = [(make_inputs(n, C, "cpu"), r) for n, C in SHAPES for r in (False, True)]
    cases += [((ill_conditioned_rows(C, "cpu"),) + make_inputs(8, C, "cpu")[1:], False) for C in (64, 260)]
    for (x, res, w, b, _), with_res in cases:
        z = x + res if with_res else x
        got = F.layer_norm(z, (z.shape[1],), w, b, EPS)
        ref = norm_act_ref(x, residual=res if with_res else None, weight=w, bias=b, relu=False, eps=EPS)
        worst = max(worst, float(((got.double() - ref["out"]).abs() / forward_bound(ref)).max()))
    print("torch float32 layer_norm: largest |error| / bound = %.4f" % worst)
    assert worst <= 0.5, worst


def test_undecided_elements_are_rare():
    """With |bias| >= 0.05 the float64 reference itself leaves out far fewer than 0.1 % of the elements: under 0.01 %."""
    for n, C in SHAPES:
        x, res, w, b, _ = make_inputs(n, C, "cpu")
        for r in (None, res):
            und = undecided(norm_act_ref(x, residual=r, weight=w, bias=b, eps=EPS))
            assert int(und.sum()) <= 1e-4 * und.numel(), (n, C, int(und.sum()))


# ---- the mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mask_depends_on_seed_row_and_column_only(hiplib):
    from wholegraph_amd import nn
    n, C, p, seed = 300, 100, 0.5, 99
    keep = _keep(nn, n, C, p, seed)
    assert torch.equal(keep, _keep(nn, n, C, p, seed)), "same seed, second call"
    assert torch.equal(keep, _keep(nn, n, C, p, seed, wide=True)), "another leading dimension"
    assert not torch.equal(keep, _keep(nn, n, C, p, seed + 1))
    # a prefix of the rows, and the rows of a taller call: row r of the segment, whatever the launch's shape
    assert torch.equal(keep[:37], _keep(nn, 37, C, p, seed)) and torch.equal(keep, _keep(nn, 1000, C, p, seed)[:n])
    # with norm, relu and residual switched on: the reference fed that mask
    x, res, w, b, _ = make_inputs(n, C, "cuda")
    out = nn.norm_dropout_act(x, w, b, residual=res, p=p, training=True, seed=seed, eps=EPS)
    ref = norm_act_ref(x, residual=res, weight=w, bias=b, keep=keep, p=p, eps=EPS)
    und = undecided(ref)
    assert bool((((out.double() - ref["out"]).abs() <= forward_bound(ref, p))).all())
    assert torch.equal((out != 0) | und, (keep & (ref["y"] > 0)) | und)


@pytest.mark.gpu
def test_dict_call_is_the_per_type_calls(hiplib):
    from wholegraph_amd import nn
    seed, p = 4242, 0.5
    shapes = {"paper": (257, 64), "nobody": (0, 36), "author": (100, 260)}
    xs, rs, ws, bs = {}, {}, {}, {}
    for t, (n, C) in shapes.items():
        xs[t], rs[t], ws[t], bs[t], _ = make_inputs(n, C, "cuda")
    del rs["author"]                                       # a type without residual
    before = nn.norm_act_launches
    out = nn.norm_dropout_act(xs, ws, bs, residual=rs, p=p, training=True, seed=seed)
    assert nn.norm_act_launches == before + 1 and list(out) == list(shapes)
    for k, t in enumerate(shapes):
        one = nn.norm_dropout_act(xs[t], ws[t], bs[t], residual=rs.get(t), p=p, training=True, seed=nn.segment_seed(seed, k))
        assert torch.equal(out[t], one), t
    # gradients too, bit for bit
    leaves = {t: xs[t].clone().requires_grad_(True) for t in xs}
    wl = {t: ws[t].clone().requires_grad_(True) for t in ws}
    out = nn.norm_dropout_act(leaves, wl, bs, residual=rs, p=p, training=True, seed=seed)
    sum(o.square().sum() for o in out.values()).backward()
    for k, t in enumerate(shapes):
        x1, w1 = xs[t].clone().requires_grad_(True), ws[t].clone().requires_grad_(True)
        nn.norm_dropout_act(x1, w1, bs[t], residual=rs.get(t), p=p, training=True, seed=nn.segment_seed(seed, k)).square().sum().backward()
        assert torch.equal(leaves[t].grad, x1.grad) and torch.equal(wl[t].grad, w1.grad), t
    # nine types: two launches, the ninth type is segment 8 of the seed
    many = {"t%d" % k: torch.ones(40, 8, device="cuda") for k in range(9)}
    before = nn.norm_act_launches
    out = nn.norm_dropout_act(many, norm=False, relu=False, p=p, training=True, seed=seed)
    assert nn.norm_act_launches == before + 2
    for k, t in enumerate(many):
        assert torch.equal(out[t] != 0, _keep(nn, 40, 8, p, nn.segment_seed(seed, k))), t


def _within(count, trials, prob, sigmas):
    return abs(count - trials * prob) <= sigmas * math.sqrt(trials * prob * (1.0 - prob))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_mask_statistics(hiplib, p):
    """[4096, 256]: the total within 5 sigma of Binomial(N, 1 - p); every row's and column's keep count within 6 sigma of its own
    (4352 tests: family-wise false alarms below 1e-5); agreement of neighbouring pairs, of the pairs inside a float4, of seeds s
    and s + 1 and of segments 0 and 1 within 6 sigma of p^2 + (1 - p)^2."""
    from wholegraph_amd import nn
    n, C, seed = 4096, 256, 2024
    p32 = float(torch.tensor(p, dtype=torch.float32))          # the kernel's p is a float32
    q = 1.0 - math.floor(p32 * 2 ** 32) / 2 ** 32
    keep = _keep(nn, n, C, p, seed)
    assert _within(int(keep.sum()), n * C, q, 5)
    rows, cols = keep.sum(1).cpu(), keep.sum(0).cpu()
    sr, sc = 6 * math.sqrt(C * q * (1 - q)), 6 * math.sqrt(n * q * (1 - q))
    assert bool(((rows - C * q).abs() <= sr).all()), float((rows - C * q).abs().max() / sr * 6)
    assert bool(((cols - n * q).abs() <= sc).all()), float((cols - n * q).abs().max() / sc * 6)
    agree = q * q + (1 - q) * (1 - q)

    def pairs(a, b, what):
        assert _within(int((a == b).sum()), a.numel(), agree, 6), what

    pairs(keep[:, :-1], keep[:, 1:], "horizontal neighbours")
    pairs(keep[:-1], keep[1:], "vertical neighbours")
    k4 = keep.view(n, C // 4, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            pairs(k4[:, :, i], k4[:, :, j], "words %d and %d of a float4" % (i, j))
    pairs(k4[:, :-1, 3], k4[:, 1:, 0], "across a float4 boundary")
    pairs(keep, _keep(nn, n, C, p, seed + 1), "seeds s and s + 1")
    ones = torch.ones(n, C, device="cuda")
    both = nn.norm_dropout_act({"a": ones, "b": ones}, norm=False, relu=False, p=p, training=True, seed=seed)
    pairs(both["a"] != 0, both["b"] != 0, "segments 0 and 1")


@pytest.mark.gpu
def test_p_zero_and_p_one(hiplib):
    from wholegraph_amd import nn
    x, res, w, b, go = make_inputs(257, 100, "cuda")
    ev = nn.norm_dropout_act(x, w, b, residual=res, p=0.5, training=False)
    assert torch.equal(nn.norm_dropout_act(x, w, b, residual=res, p=0.0, training=True, seed=5), ev)
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
    out = nn.norm_dropout_act(xg, wg, bg, residual=res, p=1.0, training=True, seed=5)
    assert torch.equal(out, torch.zeros_like(out))
    out.backward(go)
    for t in (xg, wg, bg):
        assert torch.equal(t.grad, torch.zeros_like(t))


# ---- determinism, capture, modules -------------------------------------------------------------------------------------------
def _run_once(nn, x, res, w, b, go, seed):
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
    out = nn.norm_dropout_act(xg, wg, bg, residual=res, p=0.5, training=True, seed=seed)
    out.backward(go)
    return out.detach(), xg.grad, wg.grad, bg.grad


@pytest.mark.gpu
def test_bit_reproducible(hiplib):
    """Forward, dz, dweight and dbias over three runs at [1000, 260], then once more over reused memory holding a non-zero
    pattern (what WGAMD_TEST_POISON does before a test)."""
    from wholegraph_amd import nn
    args = make_inputs(1000, 260, "cuda")
    first = _run_once(nn, *args, 31)
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(first, _run_once(nn, *args, 31)))
    blocks = [torch.empty(k, dtype=torch.int32, device="cuda").fill_(0x7F7F7F7F) for k in (1 << 22, 1 << 20, 1 << 18, 1 << 16)]
    del blocks
    assert all(torch.equal(a, b) for a, b in zip(first, _run_once(nn, *args, 31)))


@pytest.mark.gpu
def test_hip_graph_capture(hiplib):
    """Eval mode captures and replays to the eager result; training with p > 0 is refused under capture."""
    from wholegraph_amd import nn
    x, res, w, b, _ = make_inputs(257, 64, "cuda")
    m = nn.NormDropoutAct(64, p=0.5).cuda().eval()
    with torch.no_grad():
        m.weight.copy_(w), m.bias.copy_(b)
        eager = m(x, res)
        sx, sr = x.clone(), res.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(sx, sr)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m(sx, sr)
        sx.copy_(x * 2), sr.copy_(res * 2)
        graph.replay()
        assert torch.equal(captured, m(x * 2, res * 2))
        sx.copy_(x), sr.copy_(res)
        graph.replay()
        assert torch.equal(captured, eager)
        m.train()
        graph2 = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="HIP-graph capture"):
            with torch.cuda.graph(graph2):
                sx.add_(0.0)
                m(sx, sr, seed=1)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_hetero_module_against_torch_layer_norm(hiplib):
    from wholegraph_amd import nn
    widths = {"paper": 64, "author": 36, "venue": 260}
    rows = {"paper": 300, "author": 17, "venue": 64}
    torch.manual_seed(0)
    lns = {t: torch.nn.LayerNorm(c).cuda() for t, c in widths.items()}
    for ln in lns.values():
        with torch.no_grad():
            ln.weight.uniform_(-1, 1), ln.bias.uniform_(-1, 1)
    h = nn.HeteroNormDropoutAct(widths, p=0.5).cuda().eval()
    h.load_state_dict({"norms.%s.%s" % (t, k): v for t, ln in lns.items() for k, v in ln.state_dict().items()})
    xs = {t: torch.randn(rows[t], widths[t], device="cuda") for t in ("venue", "paper", "author")}
    gs = {t: torch.randn_like(v) for t, v in xs.items()}
    before = nn.norm_act_launches
    out = h(xs)
    assert h.route == "kernel" and nn.norm_act_launches == before + 1 and list(out) == list(xs)
    sum((out[t] * gs[t]).sum() for t in xs).backward()
    for t in xs:
        want = torch.relu(lns[t](xs[t]))
        (want * gs[t]).sum().backward()
        assert float((out[t] - want).detach().abs().max()) <= 1e-5 * max(1.0, float(want.detach().abs().max())), t
        for got, ref in ((h.norms[t].weight.grad, lns[t].weight.grad), (h.norms[t].bias.grad, lns[t].bias.grad)):
            assert float((got - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max())), t
    assert list(h({"paper": xs["paper"]})) == ["paper"]


@pytest.mark.gpu
def test_double_backward_runs_the_torch_formula(hiplib):
    from wholegraph_amd import nn
    x, res, w, b, go = make_inputs(64, 36, "cuda")

    def second(fn, dt):
        xg, wg = x.detach().to(dt).clone().requires_grad_(True), w.detach().to(dt).clone().requires_grad_(True)
        out = fn(xg, wg)
        gx, = torch.autograd.grad(out, xg, go.to(dt), create_graph=True)
        gx.square().sum().backward()
        return wg.grad, xg.grad

    got = second(lambda xg, wg: nn.norm_dropout_act(xg, wg, b, residual=res, relu=False), torch.float32)
    want = second(lambda xg, wg: F.layer_norm(xg + res.double(), (36,), wg, b.double(), 1e-5), torch.float64)
    for a, r in zip(got, want):
        assert float((a.double() - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("n,C", [(1, 64), (257, 100)])
def test_expanded_gradient_and_expanded_input(hiplib, n, C):
    """A column readout ``out.sum(0) * v`` hands the backward a gradient whose rows are 0 floats apart: it is copied into rows
    the kernel reads.  An input with such rows is outside the kernel's domain and takes the torch route."""
    from wholegraph_amd import nn
    x, res, w, b, _ = make_inputs(n, C, "cuda")
    v = torch.randn(C, generator=torch.Generator().manual_seed(5)).cuda()
    xg, rg, wg, bg = (t.clone().requires_grad_(True) for t in (x, res, w, b))
    m_out, route = nn._norm_dropout_act(xg, wg, bg, rg, True, EPS, 0.0, False, True, None)
    assert route == "kernel"
    m_out.sum(0).mul(v).sum().backward()
    go = v.expand(n, C)
    assert n == 1 or go.stride(0) == 0
    ref = norm_act_ref(x, residual=res, weight=w, bias=b, eps=EPS)
    und = undecided(ref)
    sign = torch.where(und, m_out.detach() > 0, ref["y"] > 0)
    ref = norm_act_ref(x, residual=res, weight=w, bias=b, eps=EPS, relu_sign=sign, grad_out=go)
    assert torch.equal(xg.grad, rg.grad)
    assert bool((((xg.grad.double() - ref["dz"]).abs() <= 1e-5 * ref["dz_terms"]) | und).all())
    assert bool(((wg.grad.double() - ref["dw"]).abs() <= 1e-5 * ref["dw_terms"]).all())
    assert bool(((bg.grad.double() - ref["db"]).abs() <= 1e-5 * ref["db_terms"]).all())
    # rows that overlap: an expanded x, an expanded residual
    row = x[:1].expand(max(n, 2), C)
    out, route = nn._norm_dropout_act(row, w, b, None, True, EPS, 0.0, False, True, None)
    assert route == "torch" and torch.equal(out[0], out[1])
    full = x[:1].expand(max(n, 2), C).contiguous()
    out2, route = nn._norm_dropout_act(full, w, b, row, True, EPS, 0.0, False, True, None)
    assert route == "torch"
    want, route = nn._norm_dropout_act(full, w, b, full.clone(), True, EPS, 0.0, False, True, None)
    assert route == "kernel"
    assert bool(((out2.double() - want.double()).abs() <= 2 * forward_bound(norm_act_ref(full, residual=full, weight=w, bias=b, eps=EPS))).all())


@pytest.mark.gpu
def test_dict_with_and_without_trainable_parameters(hiplib):
    """One type with a trainable weight and bias, one without either, one with frozen ones: the weight-gradient launch takes
    the first alone, and every gradient is the per-type call's, bit for bit."""
    from wholegraph_amd import nn
    seed, p = 17, 0.5
    shapes = {"a": (257, 64), "b": (100, 36), "c": (64, 260)}
    data = {t: make_inputs(n, C, "cuda") for t, (n, C) in shapes.items()}

    def leaves():
        xs = {t: d[0].clone().requires_grad_(True) for t, d in data.items()}
        ws = {"a": data["a"][2].clone().requires_grad_(True), "c": data["c"][2].clone()}
        bs = {"a": data["a"][3].clone().requires_grad_(True), "c": data["c"][3].clone()}
        return xs, ws, bs

    xs, ws, bs = leaves()
    out = nn.norm_dropout_act(xs, ws, bs, p=p, training=True, seed=seed)
    torch.autograd.backward([out[t] for t in shapes], [data[t][4] for t in shapes])
    assert ws["c"].grad is None and bs["c"].grad is None
    x1, w1, b1 = leaves()
    for k, t in enumerate(shapes):
        one = nn.norm_dropout_act(x1[t], w1.get(t), b1.get(t), p=p, training=True, seed=nn.segment_seed(seed, k))
        assert torch.equal(one, out[t]), t
        one.backward(data[t][4])
        assert torch.equal(x1[t].grad, xs[t].grad), t
    assert torch.equal(w1["a"].grad, ws["a"].grad) and torch.equal(b1["a"].grad, bs["a"].grad)
    keep = _keep(nn, 257, 64, p, nn.segment_seed(seed, 0))
    ref = norm_act_ref(data["a"][0], weight=data["a"][2], bias=data["a"][3], keep=keep, p=p, eps=EPS)
    sign = torch.where(undecided(ref), out["a"].detach() > 0, ref["y"] > 0)
    ref = norm_act_ref(data["a"][0], weight=data["a"][2], bias=data["a"][3], keep=keep, p=p, eps=EPS, relu_sign=sign, grad_out=data["a"][4])
    assert bool(((ws["a"].grad.double() - ref["dw"]).abs() <= 1e-5 * ref["dw_terms"]).all())
    assert bool(((bs["a"].grad.double() - ref["db"]).abs() <= 1e-5 * ref["db_terms"]).all())
    # no type with a trainable parameter at all: the backward is one launch
    xs = {t: d[0].clone().requires_grad_(True) for t, d in data.items()}
    out = nn.norm_dropout_act(xs, p=p, training=True, seed=seed)
    torch.autograd.backward([out[t] for t in shapes], [data[t][4] for t in shapes])
    assert all(bool(torch.isfinite(xs[t].grad).all()) for t in shapes)
    # the identity shortcut still hands out a fresh tensor
    x = data["a"][0]
    same = nn.norm_dropout_act(x, norm=False, relu=False)
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()
