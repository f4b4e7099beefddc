"""CPU: the MLP edge decoder's Python surface — ``wholegraph_amd.nn.EdgeDecoder`` / ``pair_mlp`` / ``link_mlp_bce_with_logits`` /
``pair_mlp_supported`` — and the float64 restatement the GPU test compares against (tests/link_mlp_ref.py)."""
import pytest
import torch
import torch.nn.functional as F

from link_mlp_ref import reference
from wholegraph_amd import nn
from wholegraph_amd.nn import EdgeDecoder


def _formula(dec, zs, zd, index):
    z = torch.cat([zs[index[0]], zd[index[1]]], dim=-1)
    return dec.lin2(dec.lin1(z).relu()).view(-1)


def test_state_dict_is_the_reference_class_layout():
    dec = EdgeDecoder(8)
    sd = dec.state_dict()
    assert list(sd) == ["lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"]
    assert sd["lin1.weight"].shape == (8, 16) and sd["lin1.bias"].shape == (8,)
    assert sd["lin2.weight"].shape == (1, 8) and sd["lin2.bias"].shape == (1,)


def test_loads_a_reference_checkpoint():
    class Reference(torch.nn.Module):       # the class of the reference's movielens / taobao examples, written out
        def __init__(self, hidden_channels):
            super().__init__()
            self.lin1 = torch.nn.Linear(2 * hidden_channels, hidden_channels)
            self.lin2 = torch.nn.Linear(hidden_channels, 1)

    torch.manual_seed(3)
    ref = Reference(8)
    dec = EdgeDecoder(8)
    dec.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(dec.state_dict().values(), ref.state_dict().values()))


def test_two_input_widths_and_no_bias():
    dec = EdgeDecoder(5, in_channels=(4, 12))
    assert dec.lin1.weight.shape == (5, 16) and dec.lin2.weight.shape == (1, 5)
    assert EdgeDecoder(5, in_channels=6).lin1.weight.shape == (5, 12)
    assert list(EdgeDecoder(8, bias=False).state_dict()) == ["lin1.weight", "lin2.weight"]


def test_reset_parameters_changes_the_weights():
    torch.manual_seed(0)
    dec = EdgeDecoder(8)
    before = [p.detach().clone() for p in dec.parameters()]
    dec.reset_parameters()
    assert all(not torch.equal(a, b) for a, b in zip(before, dec.parameters()))


@pytest.mark.parametrize("bias", [True, False])
def test_cpu_forward_and_loss_equal_the_formula(bias):
    torch.manual_seed(1)
    dec = EdgeDecoder(6, in_channels=(4, 8), bias=bias)
    zs, zd = torch.randn(7, 4), torch.randn(9, 8)
    index = torch.stack([torch.randint(0, 7, (20,)), torch.randint(0, 9, (20,))])
    label = torch.randint(0, 2, (20,)).float()
    want = _formula(dec, zs, zd, index)
    assert torch.equal(dec(zs, zd, index), want)
    assert torch.equal(dec.loss(zs, zd, index, label), F.binary_cross_entropy_with_logits(want, label))
    w = torch.rand(20)
    total = F.binary_cross_entropy_with_logits(want, label, weight=w, reduction="sum")
    assert torch.equal(dec.loss(zs, zd, index, label, pair_weight=w, reduction="sum"), total)
    assert torch.equal(dec.loss(zs, zd, index, label, pair_weight=w), total / w.sum())
    # differentiable through the fallback
    dec.loss(zs, zd, index, label).backward()
    assert all(p.grad is not None for p in dec.parameters())


def test_reference_helper_on_a_case_computed_by_hand():
    """Three pairs, H = 2, one column per table.  a = (1, 3), (2, 3), (2, -1); W1 = [[1, -1], [-1, -1]], b1 = (0.5, -0.5):
    z[:, 0] = (-1.5, -0.5, 3.5), z[:, 1] = (-4.5, -5.5, -1.5) — unit 1 is dead everywhere (its w2 = 7 must not show), unit 0
    on pairs 0 and 1.  w2 = (2, 7), b2 = -1: s = (-1, -1, 2 * 3.5 - 1 = 6).  m = |a| |W1|^T + |b1| = (4.5, 5.5, 3.5) for both
    units; M = 9 m + 1 = (41.5, 50.5, 32.5)."""
    xs, xd = torch.tensor([[1.0], [2.0]]), torch.tensor([[3.0], [-1.0]])
    index = torch.tensor([[0, 1, 1], [0, 0, 1]])
    w1, b1 = torch.tensor([[1.0, -1.0], [-1.0, -1.0]]), torch.tensor([0.5, -0.5])
    w2, b2 = torch.tensor([[2.0, 7.0]]), torch.tensor([-1.0])
    s, z, m, M = reference(xs, xd, index, w1, b1, w2, b2)
    assert s.dtype == torch.float64
    assert s.tolist() == [-1.0, -1.0, 6.0]
    assert z.tolist() == [[-1.5, -4.5], [-0.5, -5.5], [3.5, -1.5]]
    assert m.tolist() == [[4.5, 4.5], [5.5, 5.5], [3.5, 3.5]]
    assert M.tolist() == [41.5, 50.5, 32.5]
    assert nn.pair_mlp(xs, xd, index, w1, b1, w2, b2).tolist() == [-1.0, -1.0, 6.0]
    # no biases
    s, z, m, M = reference(xs, xd, index, w1, None, w2, None)
    assert z.tolist() == [[-2.0, -4.0], [-1.0, -5.0], [3.0, -1.0]] and s.tolist() == [0.0, 0.0, 6.0]
    assert M.tolist() == [36.0, 45.0, 27.0]
    assert nn.pair_mlp(xs, xd, index, w1, None, w2).tolist() == [0.0, 0.0, 6.0]


def test_wrong_shapes_raise_value_error():
    dec = EdgeDecoder(4, in_channels=(4, 8))
    zs, zd = torch.randn(5, 4), torch.randn(6, 8)
    index = torch.zeros(2, 3, dtype=torch.int64)
    label = torch.zeros(3)
    w1, b1, w2, b2 = dec.lin1.weight, dec.lin1.bias, dec.lin2.weight, dec.lin2.bias
    with pytest.raises(ValueError):
        nn.pair_mlp(zs, zd, index.t(), w1, b1, w2, b2)                      # index not [2, P]
    with pytest.raises(ValueError):
        nn.pair_mlp(zs, zd, index[0], w1, b1, w2, b2)
    with pytest.raises(ValueError):
        nn.pair_mlp(zs, zd[:, :4], index, w1, b1, w2, b2)                   # w1 width != C_src + C_dst
    with pytest.raises(ValueError):
        nn.link_mlp_bce_with_logits(zs, zd, index, label[:2], w1, b1, w2, b2)      # label length != P
    with pytest.raises(ValueError):
        nn.link_mlp_bce_with_logits(zs, zd, index, label, w1, b1, w2, b2, pair_weight=torch.ones(2))
    with pytest.raises(ValueError):
        nn.link_mlp_bce_with_logits(zs, zd, index, label, w1, b1, w2, b2, reduction="none")


def test_kernel_domain_edges(hiplib):
    for shape in [(4, 4, 1), (512, 512, 256), (4, 8, 20)]:
        assert nn.pair_mlp_supported(*shape), shape
    for shape in [(3, 4, 8), (516, 512, 8), (4, 4, 257), (4, 4, 0)]:
        assert not nn.pair_mlp_supported(*shape), shape
