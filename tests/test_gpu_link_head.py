"""GPU: the link-prediction head — ``wholegraph_amd.nn.pair_dot`` / ``link_bce_with_logits`` (csrc/wg_link.hip: one launch
forward; backward one launch per side over its incidence list, no float atomics) — against float64 torch.

Bars (the project's 1e-5 x magnitude sum): a score within ``1e-5 M_p``, ``M_p = sum_c |a_c b_c|``; the loss within
``1e-5 (sum w M / sum w + |ref|)`` (``sum w M`` for reduction="sum": the same bound before the division); a gradient element
within 1e-5 x the sum over its incident pairs of ``(|c_p| + 0.25 (w_p / W) M_p) |x|`` — ``c_p`` the pair's float64 coefficient with
the upstream factor in it, the second part what a ``1e-5 M_p`` error of a logit does to the sigmoid (whose slope is <= 1/4).
Rows no pair touches get exactly zero, a second call gives the same bits, an out-of-range index gives NaN and reads nothing."""
import pytest

pytestmark = pytest.mark.gpu


def _tables(n_src, n_dst, C, shared, scale, pad, gen):
    """float32 tables on the device; ``pad`` > 0: column views of [n, C + pad] tensors (row stride C + pad; from column 1 when
    the stride is odd, so that the rows are not 16-byte aligned either)."""
    import torch

    def one(n):
        wide = (torch.randn(n, C + pad, generator=gen) * scale).cuda()
        first = 1 if pad % 2 else 0
        return wide[:, first:first + C] if pad else wide

    xs = one(n_src)
    return xs, (xs if shared else one(n_dst))


def _pairs(P, n_src, n_dst, hub, gen):
    import torch
    i = torch.randint(0, n_src, (P,), generator=gen)
    j = torch.randint(0, n_dst, (P,), generator=gen)
    if hub:      # three quarters of the pairs on source row 0: its list spans many chunks
        i[torch.rand(P, generator=gen) < 0.75] = 0
    return torch.stack([i, j]).cuda()


def _reference(xs, xd, index, label, weight, reduction, upstream, shared):
    """float64: (scores, M, loss, loss bar, [grad per table], [gradient bar per table])."""
    import torch
    import torch.nn.functional as F
    a = xs.detach().double().requires_grad_(True)
    b = a if shared else xd.detach().double().requires_grad_(True)
    s = (a[index[0]] * b[index[1]]).sum(-1)
    M = (a[index[0]] * b[index[1]]).abs().sum(-1).detach()
    w = torch.ones_like(s) if weight is None else weight.double()
    W = float(w.sum()) if reduction == "mean" else 1.0
    loss = (F.binary_cross_entropy_with_logits(s, label.double(), reduction="none") * w).sum() / W
    (loss * upstream).backward()
    loss_bar = 1e-5 * (float((w * M).sum()) / W + abs(float(loss.detach())))
    c = upstream * w * (torch.sigmoid(s.detach()) - label.double()) / W
    per_pair = c.abs() + 0.25 * upstream * (w / W) * M
    bar_src = torch.zeros_like(a).index_add_(0, index[0], per_pair[:, None] * b.detach()[index[1]].abs())
    bar_dst = torch.zeros_like(b).index_add_(0, index[1], per_pair[:, None] * a.detach()[index[0]].abs())
    if shared:
        return s.detach(), M, loss.detach(), loss_bar, [a.grad], [1e-5 * (bar_src + bar_dst)]
    return s.detach(), M, loss.detach(), loss_bar, [a.grad, b.grad], [1e-5 * bar_src, 1e-5 * bar_dst]


def _untouched(n, idx):
    import torch
    seen = torch.zeros(n, dtype=torch.bool, device=idx.device)
    seen[idx.reshape(-1)] = True
    return ~seen


CASES = {
    # name: (P, n_src, n_dst, C, shared, weights, soft labels, hub)
    "one": (1, 1, 1, 1, False, False, False, False),
    "tiny": (5, 3, 4, 3, False, False, False, False),
    "shared64": (1000, 300, 300, 64, True, False, False, False),
    "weights100": (4096, 700, 500, 100, False, True, False, False),
    "soft256": (2000, 50, 60, 256, False, False, True, False),
    "shared260": (3000, 40, 40, 260, True, False, False, False),
    "scalar67": (777, 90, 80, 67, False, False, False, False),
    "hub32": (20000, 64, 64, 32, False, False, False, True),
    "sparse": (40, 500, 400, 16, False, False, False, False),       # most rows have no pair
}


@pytest.mark.parametrize("variant", ["plain", "x4", "x6", "sum", "upstream", "stride+4", "stride+5"])
@pytest.mark.parametrize("name", list(CASES))
def test_link_bce_matches_float64(hiplib, name, variant):
    import torch
    from wholegraph_amd import nn
    P, n_src, n_dst, C, shared, weighted, soft, hub = CASES[name]
    gen = torch.Generator().manual_seed(len(name) * 131 + P)
    scale = {"x4": 4.0, "x6": 6.0}.get(variant, 1.0)
    pad = {"stride+4": 4, "stride+5": 5}.get(variant, 0)
    reduction = "sum" if variant == "sum" else "mean"
    upstream = 1.7 if variant == "upstream" else 1.0
    xs, xd = _tables(n_src, n_dst, C, shared, scale, pad, gen)
    index = _pairs(P, n_src, n_dst, hub, gen)
    label = (torch.rand(P, generator=gen) if soft else torch.randint(0, 2, (P,), generator=gen).float()).cuda()
    weight = (torch.randint(0, 2, (P,), generator=gen).float().cuda() if weighted else None)
    if weight is not None:
        weight[0] = 1.0        # (the weights never sum to zero)
    s64, M, loss64, loss_bar, grads64, bars = _reference(xs, xd, index, label, weight, reduction, upstream, shared)

    def run():
        a = xs.detach().requires_grad_(True)
        b = a if shared else xd.detach().requires_grad_(True)
        loss = nn.link_bce_with_logits(a, b, index, label, weight, reduction=reduction)
        (loss * upstream).backward()
        return loss.detach(), ([a.grad] if shared else [a.grad, b.grad])

    loss, grads = run()
    score = nn.pair_dot(xs, xd, index)
    err = (score.double() - s64).abs()
    print("score: worst error / bar %.3f" % float((err / (1e-5 * M + 1e-300)).max()))
    assert bool((err <= 1e-5 * M).all()), float((err / (1e-5 * M + 1e-300)).max())
    print("loss %.9g ref %.9g error %.3g bar %.3g" % (float(loss), float(loss64), abs(float(loss) - float(loss64)), loss_bar))
    assert torch.isfinite(loss) and abs(float(loss) - float(loss64)) <= loss_bar
    tables = [(n_src, index if shared else index[0])] + ([] if shared else [(n_dst, index[1])])
    for got, want, bar, (n, idx) in zip(grads, grads64, bars, tables):
        e = (got.double() - want).abs()
        print("gradient: worst error / bar %.3f" % float((e / (bar + 1e-300)).max()))
        assert bool((e <= bar).all()), float((e / (bar + 1e-300)).max())
        assert bool((got[_untouched(n, idx)] == 0).all())       # rows without pairs: exactly zero
    # run-to-run: the same bits
    loss2, grads2 = run()
    assert torch.equal(loss, loss2) and all(torch.equal(g, h) for g, h in zip(grads, grads2))


@pytest.mark.parametrize("name", ["tiny", "shared64", "scalar67", "hub32", "shared260"])
def test_pair_dot_gradient_matches_float64(hiplib, name):
    """The decoder alone: an upstream gradient per pair; every gradient element within 1e-5 x the magnitude sum of its terms."""
    import torch
    from wholegraph_amd import nn
    P, n_src, n_dst, C, shared, _, _, hub = CASES[name]
    gen = torch.Generator().manual_seed(P + 7)
    xs, xd = _tables(n_src, n_dst, C, shared, 1.0, 0, gen)
    index = _pairs(P, n_src, n_dst, hub, gen)
    up = torch.randn(P, generator=gen).cuda()

    def run():
        a = xs.detach().requires_grad_(True)
        b = a if shared else xd.detach().requires_grad_(True)
        nn.pair_dot(a, b, index).backward(up)
        return [a.grad] if shared else [a.grad, b.grad]

    a64 = xs.double().requires_grad_(True)
    b64 = a64 if shared else xd.double().requires_grad_(True)
    (a64[index[0]] * b64[index[1]]).sum(-1).backward(up.double())
    bar_src = torch.zeros_like(a64).index_add_(0, index[0], up.abs().double()[:, None] * b64.detach()[index[1]].abs())
    bar_dst = torch.zeros_like(b64).index_add_(0, index[1], up.abs().double()[:, None] * a64.detach()[index[0]].abs())
    want = [a64.grad] if shared else [a64.grad, b64.grad]
    bars = [bar_src + bar_dst] if shared else [bar_src, bar_dst]
    got = run()
    for g, w, bar in zip(got, want, bars):
        assert bool(((g.double() - w).abs() <= 1e-5 * bar).all())
    assert all(torch.equal(g, h) for g, h in zip(got, run()))


@pytest.mark.parametrize("C", [64, 67])
def test_an_index_outside_its_table_gives_nan_and_reads_nothing(hiplib, C):
    """The tables are the first rows of larger allocations and one index points at the row just past the view — memory that
    is there, so a missing bounds check would read it and give a finite score."""
    import torch
    from wholegraph_amd import nn
    gen = torch.Generator().manual_seed(11)
    n_src, n_dst, P = 30, 40, 200
    big_s, big_d = torch.randn(n_src + 8, C, generator=gen).cuda(), torch.randn(n_dst + 8, C, generator=gen).cuda()
    xs, xd = big_s[:n_src].requires_grad_(True), big_d[:n_dst].requires_grad_(True)
    index = _pairs(P, n_src, n_dst, False, gen)
    index[0, 17] = n_src
    score = nn.pair_dot(xs, xd, index)
    assert bool(torch.isnan(score[17])) and bool(torch.isfinite(torch.cat([score[:17], score[18:]])).all())
    label = torch.randint(0, 2, (P,), generator=gen).float().cuda()
    assert bool(torch.isnan(nn.link_bce_with_logits(xs, xd, index, label)))
    # the pair adds nothing to either gradient: the gradients of the other pairs, finite
    score.backward(torch.ones(P, device="cuda"))
    keep = torch.arange(P, device="cuda") != 17
    a64, b64 = xs.detach().double().requires_grad_(True), xd.detach().double().requires_grad_(True)
    (a64[index[0][keep]] * b64[index[1][keep]]).sum().backward()
    i, j = index[0][keep], index[1][keep]
    bar_src = torch.zeros_like(a64).index_add_(0, i, b64.detach()[j].abs())
    bar_dst = torch.zeros_like(b64).index_add_(0, j, a64.detach()[i].abs())
    for got, want, bar in ((xs.grad, a64.grad, bar_src), (xd.grad, b64.grad, bar_dst)):
        assert bool(torch.isfinite(got).all())
        assert bool(((got.double() - want).abs() <= 1e-5 * bar).all())


def test_fallbacks_return_what_torch_returns(hiplib):
    import torch
    import torch.nn.functional as F
    from wholegraph_amd import nn
    gen = torch.Generator().manual_seed(2)
    xs, xd = torch.randn(20, 8, generator=gen).double().cuda(), torch.randn(30, 8, generator=gen).double().cuda()
    index = _pairs(50, 20, 30, False, gen)
    label = torch.randint(0, 2, (50,), generator=gen).double().cuda()
    s = (xs[index[0]] * xd[index[1]]).sum(-1)
    assert nn.pair_dot(xs, xd, index).dtype == torch.float64 and torch.equal(nn.pair_dot(xs, xd, index), s)
    assert torch.equal(nn.link_bce_with_logits(xs, xd, index, label), F.binary_cross_entropy_with_logits(s, label))
    w = torch.rand(50, generator=gen).double().cuda()
    want = F.binary_cross_entropy_with_logits(s, label, weight=w, reduction="sum")
    assert torch.equal(nn.link_bce_with_logits(xs, xd, index, label, w, reduction="sum"), want)
    assert torch.equal(nn.link_bce_with_logits(xs, xd, index, label, w), want / w.sum())
    # no pairs
    xf = xs.float()
    empty = index[:, :0]
    assert nn.pair_dot(xf, xf, empty).shape == (0,)
    none = label[:0].float()
    assert torch.equal(nn.link_bce_with_logits(xf, xf, empty, none, reduction="sum"),
                       F.binary_cross_entropy_with_logits(none, none, reduction="sum"))
    assert bool(torch.isnan(nn.link_bce_with_logits(xf, xf, empty, none))) == \
        bool(torch.isnan(F.binary_cross_entropy_with_logits(none, none)))
