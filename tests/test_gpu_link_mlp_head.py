"""GPU: the MLP edge decoder — ``wholegraph_amd.nn.pair_mlp`` / ``link_mlp_bce_with_logits`` / ``EdgeDecoder``
(csrc/wg_link_mlp.hip: one launch forward; backward one launch over the kept hidden rows, then the dot head's incidence-list sum
per side, library GEMMs and the split-K weight gradient; no float atomics) — against float64 torch autograd of

    a_p = [x_src[i_p] | x_dst[j_p]],  z_p = a_p W1^T + b1,  h_p = relu(z_p),  s_p = h_p . w2 + b2.

Bars, all from the float64 reference (tests/link_mlp_ref.py: ``m_pn = sum_k |a_pk W1_nk| + |b1_n|``,
``M_p = sum_n |w2_n| m_pn + |b2|``), the project's 1e-5 x magnitude sum once per chained fp32 sum:
  * a score within ``2e-5 M_p`` (two chained products);
  * the loss within ``1e-5 (sum w 2 M / sum w + |ref|)`` (tests/test_gpu_link_head.py's bar with 2 M for M);
  * a gradient element within ``4e-5 x`` its own formula with every factor replaced by its absolute value (``h_pn`` by
    ``m_pn``, the sum it is), one 1e-5 for each of up to four chained sums: product 1, the score behind the sigmoid, the sum
    over a row's pairs, and the GEMM or split-K.  In the BCE form ``|g_p|`` is ``|g_p| + 0.25 (w_p / W) upstream 2 M_p``: what
    the score's error does to the sigmoid, whose slope is <= 1/4.
  * The ReLU kink: a hidden entry with ``|z_pn| < 1e-4 m_pn`` in float64 may have the other mask in fp32.  No comparison is
    dropped for it; the FULL absolute term of that (p, n) is added to the bar of every gradient element it feeds.  Asserted on
    the reference in every case: at most 1 % of the entries are such (randn inputs and Linear's initialisation give 0 - 0.2 %).
Rows no pair touches get exactly zero, a second call gives the same bits, an out-of-range index gives NaN, reads nothing and adds
nothing to any gradient."""
import pytest

from link_mlp_ref import reference
from test_gpu_link_head import _pairs, _tables, _untouched

pytestmark = pytest.mark.gpu

NAMES = ("x_src", "x_dst", "w1", "b1", "w2", "b2")


def _tables2(n_src, n_dst, C_src, C_dst, shared, scale, pad, gen):
    """``_tables`` of the dot head's test for two widths (one call per table keeps its stride / alignment variants)."""
    xs, _ = _tables(n_src, n_src, C_src, True, scale, pad, gen)
    return xs, (xs if shared else _tables(n_dst, n_dst, C_dst, True, scale, pad, gen)[0])


def _decoder(C_src, C_dst, H, bias, seed):
    """``(w1, b1, w2, b2)`` on the device with torch.nn.Linear's own initialisation (b1 = b2 = None without bias)."""
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    dec = nn.EdgeDecoder(H, in_channels=(C_src, C_dst), bias=bias).cuda()
    return [None if p is None else p.detach() for p in (dec.lin1.weight, dec.lin1.bias, dec.lin2.weight, dec.lin2.bias)]


def _reference(xs, xd, index, params, shared, label=None, weight=None, reduction="mean", upstream=1.0, grad_score=None):
    """float64, over pairs that are all in range.  Returns a dict: ``s``, ``M``, ``loss``, ``loss_bar``, and per name in
    NAMES the gradient ``grad[name]`` and its bar ``bar[name]`` (``x_dst`` absent when ``shared``; a missing bias absent).
    With ``grad_score`` the scores are differentiated against it; otherwise the BCE loss times ``upstream``."""
    import torch
    import torch.nn.functional as F
    w1, b1, w2, b2 = params
    a = xs.detach().double().requires_grad_(True)
    b = a if shared else xd.detach().double().requires_grad_(True)
    p64 = [None if t is None else t.detach().double().requires_grad_(True) for t in params]
    W1, B1, W2, B2 = p64
    cat = torch.cat([a[index[0]], b[index[1]]], dim=1)
    z = cat @ W1.t() + (0 if B1 is None else B1)
    s = z.relu() @ W2.reshape(-1) + (0 if B2 is None else B2.reshape(()))
    s_ref, z_ref, m, M = reference(xs, xd, index, w1, b1, w2, b2)
    assert torch.equal(s.detach(), s_ref) or bool(((s.detach() - s_ref).abs() <= 1e-12 * M).all())
    out = {"s": s.detach(), "M": M}
    if grad_score is None:
        w = torch.ones_like(s) if weight is None else weight.double()
        W = float(w.sum()) if reduction == "mean" else 1.0
        loss = (F.binary_cross_entropy_with_logits(s, label.double(), reduction="none") * w).sum() / W
        (loss * upstream).backward()
        out["loss"] = loss.detach()
        out["loss_bar"] = 1e-5 * (float((w * 2 * M).sum()) / W + abs(float(loss.detach())))
        g = upstream * w * (torch.sigmoid(s.detach()) - label.double()) / W
        geff = g.abs() + 0.25 * (w / W) * upstream * 2 * M
    else:
        s.backward(grad_score.double())
        geff = grad_score.double().abs()
    # the ReLU kink: entries whose mask fp32 may decide the other way
    kink = z_ref.abs() < 1e-4 * m
    share = float(kink.double().mean())
    print("kink share %.4f %%" % (100 * share))
    assert share <= 0.01, share
    live = ((z_ref > 0) | kink).double()
    kink = kink.double()
    w2abs, w1abs, A = W2.detach().abs().reshape(-1), W1.detach().abs(), cat.detach().abs()
    D = geff[:, None] * w2abs[None, :] * live            # |dZ|, and the part of it at the kink
    Dk = D * kink
    Cs = xs.shape[1]

    def both(f):
        return 4e-5 * f(D) + f(Dk)

    def rows(n, idx, cols):
        return lambda d: torch.zeros(n, cols.shape[1], dtype=torch.float64, device=d.device).index_add_(0, idx, d @ cols)

    bar = {"w2": (4e-5 * (geff[:, None] * m * live).sum(0) + (geff[:, None] * m * kink).sum(0)).reshape(w2.shape),
           "b2": 4e-5 * geff.sum().reshape(1),
           "b1": both(lambda d: d.sum(0)),
           "w1": both(lambda d: d.t() @ A)}
    bar_src = both(rows(a.shape[0], index[0], w1abs[:, :Cs]))
    bar_dst = both(rows(b.shape[0], index[1], w1abs[:, Cs:]))
    grad = {"w1": W1.grad, "w2": W2.grad}
    if shared:
        grad["x_src"], bar["x_src"] = a.grad, bar_src + bar_dst
    else:
        grad["x_src"], grad["x_dst"], bar["x_src"], bar["x_dst"] = a.grad, b.grad, bar_src, bar_dst
    if B1 is not None:
        grad["b1"] = B1.grad
    if B2 is not None:
        grad["b2"] = B2.grad
    out["grad"], out["bar"] = grad, {k: v for k, v in bar.items() if k in grad}
    return out


def _leaves(xs, xd, params, shared):
    a = xs.detach().requires_grad_(True)
    b = a if shared else xd.detach().requires_grad_(True)
    return a, b, [None if t is None else t.detach().clone().requires_grad_(True) for t in params]


def _grads(a, b, p, shared):
    got = {"x_src": a.grad, "w1": p[0].grad, "w2": p[2].grad}
    if not shared:
        got["x_dst"] = b.grad
    if p[1] is not None:
        got["b1"] = p[1].grad
    if p[3] is not None:
        got["b2"] = p[3].grad
    return got


def _check_grads(got, ref):
    import torch
    assert set(got) == set(ref["grad"])
    for name in NAMES:
        if name in got:
            e = (got[name].double() - ref["grad"][name]).abs()
            bar = ref["bar"][name]
            worst = float((e / (bar + 1e-300)).max())
            print("d %s: worst error / bar %.3f" % (name, worst))
            assert bool(torch.isfinite(got[name]).all()) and bool((e <= bar).all()), (name, worst)


def _check_scores(score, ref):
    err = (score.double() - ref["s"]).abs()
    worst = float((err / (2e-5 * ref["M"] + 1e-300)).max())
    print("score: worst error / bar %.3f" % worst)
    assert bool((err <= 2e-5 * ref["M"]).all()), worst


CASES = {
    # name: (P, n_src, n_dst, C_src, C_dst, H, shared, hub)
    "one": (1, 1, 1, 4, 4, 1, False, False),                  # a tile of one row, one hidden column
    "tile15": (15, 9, 7, 4, 8, 20, False, False),             # K = 12 padded to 16; H no multiple of 16
    "tile16": (16, 9, 7, 4, 8, 20, False, False),
    "tile17": (17, 9, 7, 4, 8, 20, False, False),             # a second tile with one row
    "uneven": (1000, 300, 200, 16, 48, 64, False, False),     # C_src != C_dst: the split of W1 in every gradient
    "shared": (1000, 300, 300, 64, 64, 64, True, False),      # x_src is x_dst: two sides summed into one gradient
    "widest": (33, 20, 20, 512, 512, 256, False, False),      # K = 1024, H = 256: the LDS budget, all 16 column tiles
    "hub": (20000, 64, 64, 32, 32, 32, False, True),          # incidence lists across many 64-entry chunks
    "sparse": (40, 500, 400, 16, 16, 16, False, False),       # rows without pairs: gradient exactly 0
    # outside the kernel's domain: through torch
    "fallback_c3": (50, 20, 30, 3, 4, 8, False, False),
    "fallback_h257": (50, 20, 30, 4, 4, 257, False, False),
}
KERNEL = [n for n in CASES if not n.startswith("fallback")]
RUNS = ([(n, "plain") for n in CASES]
        + [("tile17", "x4"), ("uneven", "x4"), ("widest", "x4"),
           ("uneven", "sum"), ("shared", "sum"),
           ("uneven", "upstream"), ("hub", "upstream"),
           ("tile16", "stride+4"), ("shared", "stride+4"), ("uneven", "stride+4"),
           ("uneven", "stride+5"),                                                  # rows not 16-byte aligned: through torch
           ("uneven", "weights"), ("hub", "weights"), ("tile15", "weights"),
           ("shared", "soft"), ("tile15", "soft"),
           ("tile17", "nobias"), ("uneven", "nobias"), ("shared", "nobias")])


@pytest.mark.parametrize("name,variant", RUNS)
def test_link_mlp_bce_matches_float64(hiplib, name, variant):
    import torch
    from wholegraph_amd import nn
    P, n_src, n_dst, C_src, C_dst, H, shared, hub = CASES[name]
    gen = torch.Generator().manual_seed(len(name) * 131 + P)
    scale = 4.0 if variant == "x4" else 1.0
    pad = {"stride+4": 4, "stride+5": 5}.get(variant, 0)
    reduction = "sum" if variant == "sum" else "mean"
    upstream = 1.7 if variant == "upstream" else 1.0
    xs, xd = _tables2(n_src, n_dst, C_src, C_dst, shared, scale, pad, gen)
    index = _pairs(P, n_src, n_dst, hub, gen)
    label = (torch.rand(P, generator=gen) if variant == "soft" else torch.randint(0, 2, (P,), generator=gen).float()).cuda()
    weight = None
    if variant == "weights":        # half of them zero
        weight = (torch.randint(0, 2, (P,), generator=gen).float() * (0.5 + torch.rand(P, generator=gen))).cuda()
        weight[0] = 1.0             # (the weights never sum to zero)
    params = _decoder(C_src, C_dst, H, variant != "nobias", seed=P + H)
    ref = _reference(xs, xd, index, params, shared, label, weight, reduction, upstream)
    on_kernel = name in KERNEL and variant != "stride+5"

    def run():
        a, b, p = _leaves(xs, xd, params, shared)
        loss = nn.link_mlp_bce_with_logits(a, b, index, label, *p, pair_weight=weight, reduction=reduction)
        assert (type(loss.grad_fn).__name__ == "_PairMlpBackward") == on_kernel
        (loss * upstream).backward()
        return loss.detach(), _grads(a, b, p, shared)

    loss, got = run()
    score = nn.pair_mlp(xs, xd, index, *params)
    _check_scores(score, ref)
    err = abs(float(loss) - float(ref["loss"]))
    print("loss %.9g ref %.9g error %.3g bar %.3g" % (float(loss), float(ref["loss"]), err, ref["loss_bar"]))
    assert torch.isfinite(loss) and err <= ref["loss_bar"]
    _check_grads(got, ref)
    if on_kernel:
        # rows without pairs: exactly zero
        assert bool((got["x_src"][_untouched(n_src, index if shared else index[0])] == 0).all())
        if not shared:
            assert bool((got["x_dst"][_untouched(n_dst, index[1])] == 0).all())
        # run-to-run: the same bits, the loss and all six gradients
        loss2, got2 = run()
        assert torch.equal(loss, loss2) and all(torch.equal(got[k], got2[k]) for k in got)
        # without grad mode: the same scores bit for bit
        a, b, p = _leaves(xs, xd, params, shared)
        with_grad = nn.pair_mlp(a, b, index, *p)
        assert with_grad.requires_grad and torch.equal(with_grad.detach(), score)
        with torch.no_grad():
            assert torch.equal(nn.pair_mlp(a, b, index, *p), score)


@pytest.mark.parametrize("name", ["tile17", "uneven", "shared", "hub", "widest"])
def test_pair_mlp_gradient_matches_float64(hiplib, name):
    """The decoder alone under an arbitrary upstream gradient per pair."""
    import torch
    from wholegraph_amd import nn
    P, n_src, n_dst, C_src, C_dst, H, shared, hub = CASES[name]
    gen = torch.Generator().manual_seed(P + 7)
    xs, xd = _tables2(n_src, n_dst, C_src, C_dst, shared, 1.0, 0, gen)
    index = _pairs(P, n_src, n_dst, hub, gen)
    up = torch.randn(P, generator=gen).cuda()
    params = _decoder(C_src, C_dst, H, True, seed=P)
    ref = _reference(xs, xd, index, params, shared, grad_score=up)

    def run():
        a, b, p = _leaves(xs, xd, params, shared)
        score = nn.pair_mlp(a, b, index, *p)
        assert type(score.grad_fn).__name__ == "_PairMlpBackward"
        score.backward(up)
        return score.detach(), _grads(a, b, p, shared)

    score, got = run()
    _check_scores(score, ref)
    _check_grads(got, ref)
    score2, got2 = run()
    assert torch.equal(score, score2) and all(torch.equal(got[k], got2[k]) for k in got)


def test_dead_hidden_units_give_b2_and_zero_gradients(hiplib):
    """b1 = -1e4: every hidden unit is off, so every score is b2 bit for bit and dx, dW1, db1, dw2 are exactly zero."""
    import torch
    from wholegraph_amd import nn
    P, n_src, n_dst, C_src, C_dst, H, shared, hub = CASES["uneven"]
    gen = torch.Generator().manual_seed(5)
    xs, xd = _tables2(n_src, n_dst, C_src, C_dst, shared, 1.0, 0, gen)
    index = _pairs(P, n_src, n_dst, hub, gen)
    label = torch.randint(0, 2, (P,), generator=gen).float().cuda()
    params = _decoder(C_src, C_dst, H, True, seed=9)
    params[1] = torch.full_like(params[1], -1e4)
    score = nn.pair_mlp(xs, xd, index, *params)
    assert torch.equal(score, params[3].expand(P))
    a, b, p = _leaves(xs, xd, params, shared)
    nn.link_mlp_bce_with_logits(a, b, index, label, *p).backward()
    got = _grads(a, b, p, shared)
    for name in ("x_src", "x_dst", "w1", "b1", "w2"):
        assert bool((got[name] == 0).all()), name
    # db2 = mean(sigmoid(b2) - y)
    want = float((torch.sigmoid(params[3].double()) - label.double()).mean())
    assert abs(float(got["b2"]) - want) <= 4e-5


def test_an_index_outside_its_table_gives_nan_reads_nothing_and_adds_nothing(hiplib):
    """The tables are the middle rows of larger allocations whose other rows hold 1e30: one index[0] points at the row just
    past the view and one index[1] at the row just before it — memory that is there, so a missing bounds check would read it
    and give a finite (huge) score."""
    import torch
    from wholegraph_amd import nn
    gen = torch.Generator().manual_seed(11)
    n_src, n_dst, P, C_src, C_dst, H = 30, 40, 200, 16, 48, 20
    big_s = torch.full((n_src + 16, C_src), 1e30).cuda()
    big_d = torch.full((n_dst + 16, C_dst), 1e30).cuda()
    big_s[8:8 + n_src] = torch.randn(n_src, C_src, generator=gen).cuda()
    big_d[8:8 + n_dst] = torch.randn(n_dst, C_dst, generator=gen).cuda()
    xs, xd = big_s[8:8 + n_src], big_d[8:8 + n_dst]
    clean = _pairs(P, n_src, n_dst, False, gen)
    index = clean.clone()
    bad = [17, 33]
    index[0, 17] = n_src
    index[1, 33] = -1
    keep = torch.ones(P, dtype=torch.bool, device="cuda")
    keep[bad] = False
    params = _decoder(C_src, C_dst, H, True, seed=4)
    label = torch.randint(0, 2, (P,), generator=gen).float().cuda()
    score = nn.pair_mlp(xs, xd, index, *params)
    assert bool(torch.isnan(score[bad]).all())
    # every other score: the bits of the run without the two
    assert torch.equal(score[keep], nn.pair_mlp(xs, xd, clean, *params)[keep])
    assert bool(torch.isnan(nn.link_mlp_bce_with_logits(xs, xd, index, label, *params)))
    # weight 0 on the two: a finite loss, and the gradients of the other pairs alone
    weight = keep.float()
    ref = _reference(xs, xd, index[:, keep], params, False, label[keep])
    a, b, p = _leaves(xs, xd, params, False)
    loss = nn.link_mlp_bce_with_logits(a, b, index, label, *p, pair_weight=weight)
    assert type(loss.grad_fn).__name__ == "_PairMlpBackward"
    assert bool(torch.isfinite(loss)) and abs(float(loss.detach()) - float(ref["loss"])) <= ref["loss_bar"]
    loss.backward()
    _check_grads(_grads(a, b, p, False), ref)
    # the decoder alone: whatever comes down the two NaN scores is dropped
    up = torch.randn(P, generator=gen).cuda()
    ref = _reference(xs, xd, index[:, keep], params, False, grad_score=up[keep])
    a, b, p = _leaves(xs, xd, params, False)
    nn.pair_mlp(a, b, index, *p).backward(up)
    _check_grads(_grads(a, b, p, False), ref)


def test_edge_decoder_loss_end_to_end(hiplib):
    """The module: gradients arrive on lin1.* and lin2.* and on the embeddings, the loss is the functional form's."""
    import torch
    from wholegraph_amd import nn
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    dec = nn.EdgeDecoder(32).cuda()
    z = torch.randn(100, 32, generator=gen).cuda().requires_grad_(True)
    index = _pairs(500, 100, 100, False, gen)
    label = torch.randint(0, 2, (500,), generator=gen).float().cuda()
    loss = dec.loss(z, z, index, label)
    assert type(loss.grad_fn).__name__ == "_PairMlpBackward"
    params = [dec.lin1.weight, dec.lin1.bias, dec.lin2.weight, dec.lin2.bias]
    ref = _reference(z, z, index, [t.detach() for t in params], True, label)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= ref["loss_bar"]
    loss.backward()
    got = {"x_src": z.grad, "w1": params[0].grad, "b1": params[1].grad, "w2": params[2].grad, "b2": params[3].grad}
    assert all(g is not None and g.shape == t.shape for g, t in zip(got.values(), [z] + params))
    _check_grads(got, ref)
    _check_scores(dec(z, z, index).detach(), ref)


def test_weight_gradient_over_more_than_128_row_ranges(hiplib):
    """``gcn_wgrad(max_split=1024)`` — the head's dW1 / db1 over a whole table — where the split exceeds the 128 ranges of a
    hop's call: 70,001 rows are 137 ranges of 512.  Each element within 1e-5 x the magnitude sum of its terms (one fp32 sum),
    the same bits on a second call."""
    import torch
    from wholegraph_amd import nn
    gen = torch.Generator().manual_seed(3)
    n, F_, N = 70001, 12, 5
    x, g = torch.randn(n, F_, generator=gen).cuda(), torch.randn(n, N, generator=gen).cuda()

    def run():
        gw, gb = torch.empty(N, F_, device="cuda"), torch.empty(N, device="cuda")
        nn.gcn_wgrad(x, g, gw, gb, max_split=1024)
        return gw, gb

    gw, gb = run()
    ew = (gw.double() - g.double().t() @ x.double()).abs() / (1e-5 * (g.double().abs().t() @ x.double().abs()))
    eb = (gb.double() - g.double().sum(0)).abs() / (1e-5 * g.double().abs().sum(0))
    print("dW: worst error / bar %.3f   db: %.3f" % (float(ew.max()), float(eb.max())))
    assert float(ew.max()) <= 1 and float(eb.max()) <= 1
    gw2, gb2 = run()
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
