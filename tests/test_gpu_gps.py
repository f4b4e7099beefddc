"""wholegraph_amd.nn.segment_attention, SegmentMultiheadAttention and GPSConv on the GPU against the float64 restatement
(tests/segment_attention_ref.py).  Bars, the project's own (tests/test_gpu_hgt.py): forward |err| <= 1e-5 x magnitude sum + 1e-7
per element; gradients max |err| <= 1e-4 x max |ref| per tensor, bitwise equal across two runs.

Segment sizes: a one-node graph, an empty one, several graphs inside one 16-row tile, boundaries at 16 and 64 both +-1, a
130-node graph over three key tiles that shares its first and last workgroup with neighbours, n = 368 (a partial last 64-row
tile).  In the 130-node graph the queries are positive and the graph's LAST key row is scaled so that its logit leads every
other by about 30: the running maximum rises in the last key tile.  "late": a first graph of 70 rows, so the queries of the
next graph share a workgroup with rows 64 .. 69 and see a fully masked first key tile.

The issue lists (H, D) = (3, 20) as outside the kernels' domain; by the domain it states (D % 4 == 0, 4 <= D <= 64, H D <= 256)
it lies inside, so that case is held to the same bar on whatever route ``segment_attention_supported`` selects, and (2, 6) —
D no multiple of 4 — is the case that must take the torch route."""
import functools
import math

import pytest

from segment_attention_ref import gps_forward, mha_forward, params_of, segment_attention_ref

pytestmark = pytest.mark.gpu
SIZES = {"mixed": [1, 0, 3, 16, 17, 63, 64, 65, 130, 2, 1, 1, 5], "late": [70, 9, 30]}
SHAPES = [(1, 4), (2, 12), (4, 16), (4, 64)]      # the smallest; padded columns; one 16-column block; C = 256, the widest


def check_forward(got, ref, mag, what):
    err = (got.double().cpu() - ref).abs()
    bar = 1e-5 * mag + 1e-7
    print("%s: max |err| %.3e, max bar %.3e" % (what, float(err.max()), float(bar.max())))
    assert got.shape == ref.shape and bool((err <= bar).all()), (what, float((err - bar).max()))


def check_grads(pairs, sums=None):
    """``sums`` {name: terms}: a gradient that is a column sum whose terms cancel (a bias in front of a training-mode batch norm:
    zero in exact arithmetic) is held to 1e-4 x the largest column sum of |terms| — a float32 sum of 368 terms is off by at most
    367 x 2^-24 = 2.2e-5 of that."""
    for name, got, want in pairs:
        err, ref = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        if sums and name in sums:
            ref = float(sums[name].abs().sum(0).max())
        print("%s: max |err| %.3e, largest reference gradient %.3e" % (name, err, ref))
        assert err <= 1e-4 * ref, (name, err, ref)


@functools.lru_cache(maxsize=None)
def case(H, D, which):
    """The packed [n, 3C] input, its segments, the upstream gradient, and the float64 output, magnitude sum and gradient."""
    import torch
    sizes, C = SIZES[which], H * D
    n = sum(sizes)
    g = torch.Generator().manual_seed(1000 * H + 10 * D + len(sizes))
    qkv, gout = torch.rand((n, 3 * C), generator=g) * 2 - 1, torch.rand((n, C), generator=g) * 2 - 1
    if which == "mixed":
        a = sum(sizes[:8])
        qkv[a:a + 130, :C] = qkv[a:a + 130, :C].abs()
        qkv[a + 129, C:2 * C] = 1 + 60 / math.sqrt(D)
    x64 = qkv.double().requires_grad_(True)
    ref, mag = segment_attention_ref(x64[:, :C], x64[:, C:2 * C], x64[:, 2 * C:], sizes, H)
    (ref * gout.double()).sum().backward()
    ptr = torch.tensor([0] + sizes).cumsum(0)
    return qkv, ptr, gout, ref.detach(), mag, x64.grad


def run(qkv, ptr, H, gout=None):
    import torch
    from wholegraph_amd import nn
    C = qkv.shape[1] // 3
    x = qkv.cuda().requires_grad_(gout is not None)
    before = nn.segment_attention_launches
    with torch.set_grad_enabled(gout is not None):
        out = nn.segment_attention(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], ptr.cuda(), H)      # strided views, no copies
    if gout is not None:
        (out * gout.cuda()).sum().backward()
    return out.detach(), x.grad, nn.segment_attention.route, nn.segment_attention_launches - before


@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("which", sorted(SIZES))
def test_forward(hiplib, H, D, which):
    import torch
    qkv, ptr, _, ref, mag, _ = case(H, D, which)
    out, _, route, launches = run(qkv, ptr, H)
    assert route == "kernel" and launches == 1
    check_forward(out, ref, mag, "H %d D %d %s" % (H, D, which))
    ones = [int(ptr[g]) for g, m in enumerate(SIZES[which]) if m == 1]
    assert torch.equal(out[ones].cpu(), qkv[ones, 2 * H * D:])      # a one-node graph: its v row, exactly


@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("which", sorted(SIZES))
def test_gradients(hiplib, H, D, which):
    import torch
    qkv, ptr, gout, _, _, want = case(H, D, which)
    C = H * D
    (_, got, route, launches), (_, again, _, _) = run(qkv, ptr, H, gout), run(qkv, ptr, H, gout)
    assert route == "kernel" and launches == 3 and torch.equal(got, again)
    check_grads([(name, got[:, k * C:(k + 1) * C], want[:, k * C:(k + 1) * C]) for k, name in enumerate(("dq", "dk", "dv"))])


@pytest.mark.parametrize("training", [False, True])
def test_gpsconv(hiplib, training):
    import torch
    from wholegraph_amd import nn
    H, C, sizes = 4, 64, SIZES["mixed"]
    n = sum(sizes)
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    conv = nn.GPSConv(C, nn.GINConv(torch.nn.Sequential(torch.nn.Linear(C, C), torch.nn.ReLU(), torch.nn.Linear(C, C))),
                      heads=H).cuda().train(training)
    ptr = torch.tensor([0] + sizes).cumsum(0)
    edges = torch.cat([s + torch.randint(0, m, (2, 2 * m), generator=g) for s, m in zip(ptr.tolist(), sizes) if m > 0], 1)
    x, gout = torch.rand((n, C), generator=g) * 2 - 1, torch.rand((n, C), generator=g) * 2 - 1
    p64 = {k: v.requires_grad_(v.is_floating_point() and k in dict(conv.named_parameters())) for k, v in params_of(conv).items()}
    x64 = x.double().requires_grad_(True)
    taps = {}
    ref, mag = gps_forward(p64, x64, edges, sizes, H, training, taps)
    (ref * gout.double()).sum().backward()
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        out = conv(xg, edges.cuda(), ptr=ptr.cuda())
        assert conv.route == "kernel"
        (out * gout.cuda()).sum().backward()
        runs.append([out.detach(), xg.grad] + [q.grad for q in conv.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    check_forward(runs[0][0], ref.detach(), mag, "GPSConv training=%s" % training)
    check_grads([("x", runs[0][1], x64.grad)] + [(k, q.grad, p64[k].grad) for k, q in conv.named_parameters()],
                {k: t.grad for k, t in taps.items()} if training else None)


@pytest.mark.parametrize("H,D", [(3, 20), (2, 6)])
def test_shapes_at_the_domain_edge(hiplib, H, D):
    from wholegraph_amd import nn
    qkv, ptr, _, ref, mag, _ = case(H, D, "mixed")
    out, _, route, launches = run(qkv, ptr, H)
    assert route == ("kernel" if nn.segment_attention_supported(H, D) else "torch") and launches == (route == "kernel")
    assert route == "torch" or D % 4 == 0
    check_forward(out, ref, mag, "H %d D %d on the %s route" % (H, D, route))


def test_unsorted_batch_takes_the_torch_route(hiplib):
    import torch
    from wholegraph_amd import nn
    H, C, sizes = 4, 64, SIZES["late"]
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(3)
    attn = nn.SegmentMultiheadAttention(C, H).cuda()
    x = torch.rand((sum(sizes), C), generator=g) * 2 - 1
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ref, mag = mha_forward(params_of(attn), x.double(), sizes, H)
    mix = torch.randperm(x.shape[0], generator=g)
    with torch.no_grad():
        out = attn(x[mix].cuda(), batch=batch[mix].cuda())
        assert attn.route == "torch"
        check_forward(out, ref[mix], mag[mix], "unsorted batch")
        out = attn(x.cuda(), batch=batch.cuda())
        assert attn.route == "kernel"
        check_forward(out, ref, mag, "sorted batch")
