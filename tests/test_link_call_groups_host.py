"""Host: the index arithmetic of a link call group (``cugraph_pyg_amd.loader.link_call_group.link_group_index``) and the
torch formulation ``wholegraph_amd.nn.link_bce_with_logits`` falls back to — its ``reduction`` / ``pair_weight`` semantics held
against ``F.binary_cross_entropy_with_logits``, and GAE's ``recon_loss`` expressed through it."""
import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("G,n_pos,n_neg", [(1, 1, 0), (3, 4, 2), (2, 5, 0), (4, 3, 7)])
def test_link_group_index_is_the_batch_local_index_shifted_by_batch_ptr(G, n_pos, n_neg):
    from cugraph_pyg_amd.loader.link_call_group import link_group_index
    gen = torch.Generator().manual_seed(G * 100 + n_pos * 10 + n_neg)
    half = n_pos + n_neg
    sizes = torch.randint(1, 2 * half + 1, (G,), generator=gen)              # unique endpoints per batch
    batch_ptr = torch.zeros(G + 1, dtype=torch.int32)
    batch_ptr[1:] = torch.cumsum(sizes, 0)
    local = torch.stack([torch.randint(0, int(sizes[b]), (2 * half,), generator=gen) for b in range(G)])
    index, label_ptr = link_group_index(local, batch_ptr, n_pos, n_neg)
    assert index.dtype == torch.int64 and index.shape == (2, G * half)
    assert label_ptr.dtype == torch.int64 and label_ptr.tolist() == [b * half for b in range(G + 1)]
    for b in range(G):       # batch b's pairs: what the per-batch loader emits (stack of the two halves of the inverse map), shifted
        mine = index[:, label_ptr[b]:label_ptr[b + 1]]
        want = torch.stack([local[b, :half], local[b, half:]]) + int(batch_ptr[b])
        assert torch.equal(mine, want)
        assert int(mine.min()) >= int(batch_ptr[b]) and int(mine.max()) < int(batch_ptr[b + 1])
        # positives first inside a batch: pair k < n_pos is seed edge k
        assert torch.equal(mine[0, :n_pos] - int(batch_ptr[b]), local[b, :n_pos])
        assert torch.equal(mine[1, :n_pos] - int(batch_ptr[b]), local[b, half:half + n_pos])


def _problem(dtype=torch.float32):
    gen = torch.Generator().manual_seed(5)
    xs, xd = torch.randn(9, 6, generator=gen).to(dtype), torch.randn(7, 6, generator=gen).to(dtype)
    index = torch.stack([torch.randint(0, 9, (40,), generator=gen), torch.randint(0, 7, (40,), generator=gen)])
    label = torch.rand(40, generator=gen).to(dtype)
    weight = torch.rand(40, generator=gen).to(dtype)
    return xs, xd, index, label, weight


def test_pair_dot_on_the_host_is_the_torch_formulation():
    from wholegraph_amd import nn
    xs, xd, index, _, _ = _problem()
    assert torch.equal(nn.pair_dot(xs, xd, index), (xs[index[0]] * xd[index[1]]).sum(-1))
    with pytest.raises(ValueError):
        nn.pair_dot(xs, xd[:, :5], index)


def test_link_bce_reduction_and_pair_weight_semantics():
    from wholegraph_amd import nn
    xs, xd, index, label, weight = _problem(torch.float64)
    s = (xs[index[0]] * xd[index[1]]).sum(-1)
    per_pair = F.binary_cross_entropy_with_logits(s, label, reduction="none")
    assert torch.equal(nn.link_bce_with_logits(xs, xd, index, label), F.binary_cross_entropy_with_logits(s, label))
    assert torch.equal(nn.link_bce_with_logits(xs, xd, index, label, reduction="sum"),
                       F.binary_cross_entropy_with_logits(s, label, reduction="sum"))
    # weights: "sum" is torch's weighted sum, "mean" divides it by the sum of the weights (not by the number of pairs)
    torch.testing.assert_close(nn.link_bce_with_logits(xs, xd, index, label, weight, reduction="sum"), (weight * per_pair).sum())
    torch.testing.assert_close(nn.link_bce_with_logits(xs, xd, index, label, weight), (weight * per_pair).sum() / weight.sum())
    assert torch.equal(nn.link_bce_with_logits(xs, xd, index, label, weight, reduction="sum"),
                       F.binary_cross_entropy_with_logits(s, label, weight=weight, reduction="sum"))
    # 0 / 1 weights under "mean": the mean over the kept pairs
    keep = weight > 0.5
    torch.testing.assert_close(nn.link_bce_with_logits(xs, xd, index, label, keep.double()), per_pair[keep].mean())
    with pytest.raises(ValueError):
        nn.link_bce_with_logits(xs, xd, index, label, reduction="none")
    # differentiable in both tables
    a, b = xs.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    nn.link_bce_with_logits(a, b, index, label, weight).backward()
    a2, b2 = xs.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    ((weight * F.binary_cross_entropy_with_logits((a2[index[0]] * b2[index[1]]).sum(-1), label, reduction="none")).sum()
     / weight.sum()).backward()
    torch.testing.assert_close(a.grad, a2.grad)
    torch.testing.assert_close(b.grad, b2.grad)


def test_gae_recon_loss_through_link_bce():
    """GAE's reconstruction loss (restated here): ``-mean log(sigmoid(z_i . z_j) + eps)`` over the positive edges plus
    ``-mean log(1 - sigmoid(z_i . z_j) + eps)`` over the negative ones, eps = 1e-15 — "sum" with weights 1 / n_pos and 1 / n_neg."""
    from wholegraph_amd import nn
    gen = torch.Generator().manual_seed(8)
    z = torch.randn(30, 8, generator=gen, dtype=torch.float64) * 0.5
    pos = torch.randint(0, 30, (2, 25), generator=gen)
    neg = torch.randint(0, 30, (2, 40), generator=gen)
    eps = 1e-15
    dot = lambda e: (z[e[0]] * z[e[1]]).sum(-1)    # noqa: E731
    recon = -torch.log(torch.sigmoid(dot(pos)) + eps).mean() - torch.log(1 - torch.sigmoid(dot(neg)) + eps).mean()
    index = torch.cat([pos, neg], 1)
    label = torch.cat([torch.ones(25), torch.zeros(40)]).double()
    weight = torch.cat([torch.full((25,), 1 / 25, dtype=torch.float64), torch.full((40,), 1 / 40, dtype=torch.float64)])
    got = nn.link_bce_with_logits(z, z, index, label, weight, reduction="sum")
    torch.testing.assert_close(got, recon, rtol=1e-9, atol=1e-12)
