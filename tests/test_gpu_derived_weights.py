"""The derived forms of the weights (``nn._derived``) as the layers use them on the GPU: a layer's output follows its parameters
through the version counter and through ``bump_weight_generation``, a hit is the stored object, a capturing stream builds its
own forms and leaves the kept ones alone, and ``sage_layer_fused_forward(prepared=...)`` refuses an ``out`` the bf16x3 kernel
cannot write before it launches anything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from layer_graphs import empty_hop_graph  # noqa: E402

pytestmark = pytest.mark.gpu


def _fresh_sage(nn, conv, F, N):
    other = nn.SAGEConv(F, N).cuda()
    other.load_state_dict(conv.state_dict())
    return other


@pytest.mark.parametrize("N", [16, 64])      # 16: the padded head (runs as 64 columns); 64: the kernel's own width
def test_sage_layer_follows_its_weights(hiplib, N):
    from wholegraph_amd import nn
    F = 32
    assert nn.sage_layer_fused_preferred(F, N) and nn._padded_width(N) == 64
    lg, _, _ = empty_hop_graph(200, seed=21 + N)
    torch.manual_seed(N)
    conv = nn.SAGEConv(F, N).cuda()
    x = torch.randn((200, F), device="cuda")
    with torch.no_grad():
        y0 = conv(x, lg)
        assert y0.shape == (120, N)
        conv.lin_l.weight.add_(0.5)                       # an optimizer's in-place step: the version moves
        y1 = conv(x, lg)
        assert not torch.equal(y1, y0) and torch.equal(y1, _fresh_sage(nn, conv, F, N)(x, lg))
        conv.lin_l.weight.data.add_(0.25)                 # behind the counter (what a graph replay does): the kept forms are stale ...
        assert torch.equal(conv(x, lg), y1)
        nn.bump_weight_generation()                       # ... until the generation moves
        y2 = conv(x, lg)
        assert not torch.equal(y2, y1) and torch.equal(y2, _fresh_sage(nn, conv, F, N)(x, lg))


def test_hits_are_the_stored_objects(hiplib):
    from wholegraph_amd import nn
    conv = nn.SAGEConv(32, 16).cuda()
    w_t = conv._weight_t()
    assert conv._weight_t() is w_t and w_t.shape == (64, 16) and not w_t.requires_grad
    assert nn.sage_weight_planes(w_t) is nn.sage_weight_planes(w_t)
    head = nn._padded_head(w_t, conv.lin_l.bias, 64)
    assert nn._padded_head(w_t, conv.lin_l.bias, 64) is head and head[0].shape == (64, 64) and head[1].shape == (64,)
    assert torch.equal(head[0][:, :16], w_t) and not head[0][:, 16:].any() and torch.equal(head[1][:16], conv.lin_l.bias.detach())
    # the backward's weight, reached through a layer only above 16384 rows
    assert nn.sage_layer_fused_supported(16, 32)
    w_bwd = conv._weight_bwd()
    assert conv._weight_bwd() is w_bwd and w_bwd.shape == (32, 32) and not w_bwd.requires_grad
    assert torch.equal(w_bwd[:16], conv.lin_l.weight.detach()) and torch.equal(w_bwd[16:], conv.lin_r.weight.detach())
    with torch.no_grad():
        conv.lin_r.weight.mul_(2.0)
    assert conv._weight_bwd() is not w_bwd and torch.equal(conv._weight_bwd()[16:], conv.lin_r.weight.detach())
    assert conv._weight_t() is not w_t
    wide = nn.SAGEConv(260, 16).cuda()
    assert not nn.sage_layer_fused_supported(16, 260) and wide._weight_bwd() is None


def test_gat_transform_follows_its_weight(hiplib):
    from wholegraph_amd import nn
    F, H, C, n = 64, 1, 64, 16
    assert nn.gat_transform_supported(F, H, C) and not nn.gat_transform_supported(F // 2, H, C) \
        and not nn.gat_transform_supported(F, H, C // 2)
    g = torch.Generator(device="cuda").manual_seed(8)
    agg = torch.rand((n, H * F), generator=g, device="cuda") - 0.5
    w = (torch.rand((F, H * C), generator=g, device="cuda") - 0.5) * 0.2
    y0 = nn.gat_transform_heads_fused(agg, w, H)
    tiles = nn._gat_weight_tiles(w, H)
    assert nn._gat_weight_tiles(w, H) is tiles
    w.add_(0.5)                                           # the version moves
    y1 = nn.gat_transform_heads_fused(agg, w, H)
    assert nn._gat_weight_tiles(w, H) is not tiles
    assert not torch.equal(y1, y0) and torch.equal(y1, nn.gat_transform_heads_fused(agg, w.clone(), H))
    w.data.add_(0.25)                                     # behind the counter: stale ...
    assert torch.equal(nn.gat_transform_heads_fused(agg, w, H), y1)
    nn.bump_weight_generation()                           # ... until the generation moves
    y2 = nn.gat_transform_heads_fused(agg, w, H)
    assert not torch.equal(y2, y1) and torch.equal(y2, nn.gat_transform_heads_fused(agg, w.clone(), H))


def test_a_capturing_stream_builds_its_own_forms(hiplib):
    from wholegraph_amd import nn
    conv = nn.SAGEConv(32, 64).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # (warm-up on a side stream, as torch asks before a capture)
        nn.sage_weight_planes(torch.cat([conv.lin_l.weight.detach(), conv.lin_r.weight.detach()], 1).t().contiguous())
    torch.cuda.current_stream().wait_stream(side)
    w_t = conv._weight_t()                                # primed eagerly
    planes = nn.sage_weight_planes(w_t)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inside = nn._capturing()
        w_t_c = conv._weight_t()
        w_t_c2 = conv._weight_t()
        planes_c = nn.sage_weight_planes(w_t_c)
        planes_p = nn.sage_weight_planes(w_t)             # (the kept tensor as the holder: still neither read nor stored)
    assert inside and not nn._capturing()
    assert w_t_c is not w_t and w_t_c2 is not w_t_c and w_t_c.data_ptr() != w_t.data_ptr()
    assert planes_c is not planes and planes_p is not planes
    assert not hasattr(w_t_c, "_wgamd_derived")
    assert conv._weight_t() is w_t and nn.sage_weight_planes(w_t) is planes      # eager code still hits what it primed


def test_prepared_refuses_an_out_the_bf16x3_kernel_cannot_write(hiplib):
    from wholegraph_amd import nn
    F, N = 32, 64
    lg, _, _ = empty_hop_graph(200, seed=5)
    hop = lg.hops[0]
    conv = nn.SAGEConv(F, N).cuda()
    x = torch.randn((200, F), device="cuda")
    prepared = nn.sage_layer_planes(conv.lin_l.weight.detach(), conv.lin_r.weight.detach(), conv.lin_l.bias.detach(), N)
    buf = torch.full((hop.n_rows, N + 1), 7.0, device="cuda")
    out = buf[:, 1:]                                      # [n, N], row stride N + 1: rows are not 16-B aligned
    assert out.shape == (hop.n_rows, N) and (out.stride(0) % 4 != 0 or out.data_ptr() % 16 != 0)
    with pytest.raises(ValueError, match="16-B aligned"):
        nn.sage_layer_fused_forward(hop.row_ptr, hop.col, x, hop.self_rows, None, prepared=prepared, out=out)
    assert bool((buf == 7.0).all())                       # nothing was launched
    # the same call with an `out` of its own runs: the layer against the float64 formula at 1e-5 x sum|terms| (fp32-class)
    good = nn.sage_layer_fused_forward(hop.row_ptr, hop.col, x, hop.self_rows, None, prepared=prepared)
    deg = (hop.row_ptr[1:] - hop.row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(hop.n_rows, device="cuda"), deg)
    xd, wl, wr, b = x.double(), conv.lin_l.weight.detach().double(), conv.lin_r.weight.detach().double(), conv.lin_l.bias.detach().double()
    mean = torch.zeros((hop.n_rows, F), dtype=torch.float64, device="cuda").index_add_(0, dst, xd[hop.col.long()])
    mean = mean / deg.clamp(min=1).double().unsqueeze(1)
    ref = mean @ wl.t() + xd[hop.self_rows] @ wr.t() + b
    mag = mean.abs() @ wl.abs().t() + xd[hop.self_rows].abs() @ wr.abs().t() + b.abs()
    assert float(((good.double() - ref).abs() / mag).max()) <= 1e-5
