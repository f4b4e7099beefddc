"""wholegraph_amd.nn.SegmentMultiheadAttention and GPSConv on the host: the torch route in float64 against
torch.nn.MultiheadAttention over the padded batch, the state-dict names, and the arguments that are refused."""
import pytest
import torch

from wholegraph_amd import nn

SIZES = [1, 5, 9]


def test_matches_multihead_attention_over_the_padded_batch():
    C, H, n = 12, 3, sum(SIZES)
    torch.manual_seed(0)
    theirs = torch.nn.MultiheadAttention(C, H, batch_first=True).double()
    with torch.no_grad():
        theirs.in_proj_bias.uniform_(-1, 1)
        theirs.out_proj.bias.uniform_(-1, 1)
    ours = nn.SegmentMultiheadAttention(C, H).double()
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    x = torch.rand((n, C), dtype=torch.float64) * 2 - 1
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    ptr = torch.tensor([0] + SIZES).cumsum(0)
    dense = torch.zeros((len(SIZES), max(SIZES), C), dtype=torch.float64)
    mask = torch.arange(max(SIZES))[None, :] < torch.tensor(SIZES)[:, None]
    dense[mask] = x
    mix = torch.randperm(n)
    with torch.no_grad():
        want = theirs(dense, dense, dense, key_padding_mask=~mask, need_weights=False)[0][mask]
        for kwargs in ({"ptr": ptr}, {"batch": batch}):
            got = ours(x, **kwargs)
            assert ours.route == "torch" and float((got - want).abs().max()) <= 1e-12
        assert float((ours(x[mix], batch=batch[mix]) - want[mix]).abs().max()) <= 1e-12
        assert float((ours(x[:1]) - want[:1]).abs().max()) <= 1e-12      # no batch: one graph


def test_gpsconv_state_dict_names():
    lin = torch.nn.Linear
    conv = nn.GPSConv(8, nn.GINConv(torch.nn.Sequential(lin(8, 8), torch.nn.ReLU(), lin(8, 8))), heads=2)
    norms = [p % k for k in (1, 2, 3) for p in ("norm%d.module.weight", "norm%d.module.bias", "norm%d.module.running_mean",
                                                "norm%d.module.running_var", "norm%d.module.num_batches_tracked")]
    assert list(conv.state_dict()) == [
        "conv.eps", "conv.nn.0.weight", "conv.nn.0.bias", "conv.nn.2.weight", "conv.nn.2.bias",
        "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
        "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"] + norms
    assert not any(k.startswith("norm") for k in nn.GPSConv(8, None, heads=2, norm=None).state_dict())


@pytest.mark.parametrize("kwargs", [{"norm": "layer_norm"}, {"act": "gelu"}, {"attn_type": "performer"}, {"dropout": 1.5},
                                    {"norm_kwargs": {"affine": False}}, {"attn_kwargs": {"kdim": 4}}, {"heads": 3}])
def test_refused_arguments(kwargs):
    with pytest.raises(ValueError, match=next(iter(kwargs)) if "heads" not in kwargs else "num_heads"):
        nn.GPSConv(8, None, **kwargs)


def test_layer_graph_is_refused():
    conv = nn.GPSConv(8, None, heads=2)
    with pytest.raises(NotImplementedError, match="whole graphs"):
        conv(torch.zeros((4, 8)), nn.LayerGraph([]))
