"""RowLinear without a GPU: the module's parameters and state dicts, ``wrap``, the torch route on CPU tensors (bit for bit torch's
own ops), a CPU ``LazyRows`` over a 16-bit table, the supported widths, the ValueErrors, and the C entries' refusals, which all
come before any device call."""
import pytest
import torch
import torch.nn.functional as F


def _params(m):
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-1, 1)
    return m


def test_state_dict_and_initialisation_are_torchs():
    from wholegraph_amd import nn
    torch.manual_seed(3)
    m = nn.RowLinear(12, 8, norm="layer")
    torch.manual_seed(3)
    lin, ln = torch.nn.Linear(12, 8), torch.nn.LayerNorm(8)
    assert list(m.state_dict()) == ["lin.weight", "lin.bias", "norm.weight", "norm.bias"]
    assert torch.equal(m.lin.weight, lin.weight) and torch.equal(m.lin.bias, lin.bias)
    assert torch.equal(m.norm.weight, torch.ones(8)) and torch.equal(m.norm.bias, torch.zeros(8)) and m.norm.eps == ln.eps == 1e-5
    assert isinstance(m.lin, torch.nn.Linear) and isinstance(m.norm, torch.nn.LayerNorm)
    _params(m)
    torch.manual_seed(3)
    m.reset_parameters()
    assert torch.equal(m.lin.weight, lin.weight) and torch.equal(m.norm.weight, torch.ones(8))
    assert list(nn.RowLinear(12, 8).state_dict()) == ["lin.weight", "lin.bias"]
    assert list(nn.RowLinear(12, 8, bias=False, relu=True, norm="l2").state_dict()) == ["lin.weight"]
    assert list(nn.RowLinear(12, 8, norm="layer", elementwise_affine=False).state_dict()) == ["lin.weight", "lin.bias"]
    assert nn.RowLinear(12, 8, norm="l2").eps == 1e-12 and nn.RowLinear(12, 8, norm="layer", eps=1e-3).norm.eps == 1e-3
    # a separate Linear / LayerNorm pair's state loads (no Sequential around them)
    _params(lin), _params(ln)
    state = {"lin." + k: v for k, v in lin.state_dict().items()}
    state.update({"norm." + k: v for k, v in ln.state_dict().items()})
    m.load_state_dict(state)
    assert torch.equal(m.lin.weight, lin.weight) and torch.equal(m.norm.bias, ln.bias)


def test_wrap_shares_the_parameters():
    from wholegraph_amd import nn
    lin, ln = _params(torch.nn.Linear(16, 8)), _params(torch.nn.LayerNorm(8, eps=1e-4))
    m = nn.RowLinear.wrap(lin, ln)
    assert m.lin is lin and m.norm is ln and m.lin.weight is lin.weight and m.norm.bias is ln.bias and m.eps == 1e-4
    assert list(m.state_dict()) == ["lin.weight", "lin.bias", "norm.weight", "norm.bias"]
    x = torch.randn(5, 16)
    assert torch.equal(m(x), ln(lin(x))) and m.route == "torch"
    tail = nn.RowLinear.wrap(lin, relu=True, l2=True)
    assert tail.lin.weight is lin.weight and list(tail.state_dict()) == ["lin.weight", "lin.bias"]
    assert torch.equal(tail(x), F.normalize(lin(x).relu(), p=2, dim=-1))
    with pytest.raises(ValueError):
        nn.RowLinear.wrap(lin, ln, l2=True)
    with pytest.raises(ValueError):
        nn.RowLinear.wrap(lin, torch.nn.LayerNorm(4))


def test_cpu_tensors_take_the_torch_route(hiplib):
    from wholegraph_amd import nn
    torch.manual_seed(0)
    x = torch.randn(9, 16, requires_grad=True)
    rows = torch.tensor([8, 0, 3, 3, 5])
    add = torch.randn(5, 8, requires_grad=True)
    proj = _params(nn.RowLinear(16, 8, norm="layer"))
    out = proj(x, rows)
    assert proj.route == "torch"
    assert torch.equal(out, F.layer_norm(F.linear(x[rows], proj.lin.weight, proj.lin.bias), (8,), proj.norm.weight, proj.norm.bias, 1e-5))
    tail = _params(nn.RowLinear(16, 8, relu=True, norm="l2"))
    out2 = tail(x, rows, add=add)
    assert torch.equal(out2, F.normalize(F.linear(x[rows], tail.lin.weight, tail.lin.bias).relu(), p=2, dim=-1) + add)
    plain = _params(nn.RowLinear(16, 8))
    assert torch.equal(plain(x), F.linear(x, plain.lin.weight, plain.lin.bias)) and plain.route == "torch"
    assert torch.equal(nn.linear_rows(x, plain.lin.weight, relu=True, rows=rows.int()), F.linear(x[rows], plain.lin.weight).relu())
    (out.sum() + out2.sum()).backward()
    for p in list(proj.parameters()) + list(tail.parameters()) + [x, add]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    buf = torch.zeros(5, 8)
    assert nn.linear_rows(x.detach(), plain.lin.weight.detach(), rows=rows, out=buf) is buf
    assert torch.equal(buf, F.linear(x.detach()[rows], plain.lin.weight))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cpu_lazy_rows_over_a_16_bit_table(hiplib, dtype):
    from wholegraph_amd import nn
    torch.manual_seed(1)
    table = torch.randn(20, 16).to(dtype)
    ids = torch.tensor([19, 2, 2, 7, 0, 11], dtype=torch.int32)
    rows = torch.tensor([5, 1, 1, 0])
    m = _params(nn.RowLinear(16, 8, relu=True, norm="layer"))
    lazy = nn.LazyRows(table, ids)
    xr = table.float()[ids.long()[rows]]
    want = F.layer_norm(F.linear(xr, m.lin.weight, m.lin.bias).relu(), (8,), m.norm.weight, m.norm.bias, 1e-5)
    assert torch.equal(m(lazy, rows), want) and m.route == "torch"
    assert torch.equal(m(lazy), F.layer_norm(F.linear(table.float()[ids.long()], m.lin.weight, m.lin.bias).relu(), (8,),
                                             m.norm.weight, m.norm.bias, 1e-5))


def test_supported_widths(hiplib):
    from wholegraph_amd import nn
    shapes = [(0, 4), (2, 4), (4, 4), (6, 8), (1024, 256), (1028, 256), (64, 260), (64, 6)]
    assert [nn.linear_rows_supported(K, N) for K, N in shapes] == [False, False, True, False, True, False, False, False]


def test_value_errors(hiplib):
    from wholegraph_amd import nn
    with pytest.raises(ValueError, match="norm"):
        nn.RowLinear(8, 8, norm="batch")
    with pytest.raises(ValueError, match="elementwise_affine"):
        nn.RowLinear(8, 8, norm="l2", elementwise_affine=True)
    with pytest.raises(ValueError, match="elementwise_affine"):
        nn.RowLinear(8, 8, norm="l2", elementwise_affine=False)
    x, w = torch.randn(6, 8), torch.randn(4, 8)
    with pytest.raises(ValueError, match="norm"):
        nn.linear_rows(x, w, norm="rms")
    with pytest.raises(ValueError, match="add"):
        nn.linear_rows(x, w, add=torch.zeros(6, 8))
    with pytest.raises(ValueError, match="add"):
        nn.linear_rows(x, w, rows=torch.tensor([0, 1]), add=torch.zeros(6, 4))
    with pytest.raises(ValueError, match="out of range"):
        nn.linear_rows(x, w, rows=torch.tensor([0, 6]))
    with pytest.raises(ValueError, match="out of range"):
        nn.linear_rows(x, w, rows=torch.tensor([-1]))
    with pytest.raises(ValueError, match="weight"):
        nn.linear_rows(x, torch.randn(4, 12))


FAKE = 0x100000      # never dereferenced: every refusal comes before a device call


def _fwd(hiplib, L, **kw):
    a = dict(x=FAKE, x_dtype=L.DT_FLOAT, ldx=8, ids=None, ids_dtype=0, n=4, K=8, weight=FAKE + 0x1000, ldw=8, N=8, bias=None, relu=1,
             norm=L.ROW_LINEAR_NORM_LAYER, gamma=None, beta=None, eps=1e-5, add=None, ld_add=0, out=FAKE + 0x2000, ldo=8, kept_x=None,
             ld_kx=0, kept_y=None, ld_ky=0)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return hiplib.wgamd_row_linear_f32(*a.values(), None)


def test_forward_entry_refuses_before_touching_a_device(hiplib):
    from wholegraph_amd import _lib as L
    bad, logic = L.WHOLEMEMORY_INVALID_INPUT, L.WHOLEMEMORY_LOGIC_ERROR
    assert _fwd(hiplib, L, x=None) == bad and _fwd(hiplib, L, weight=None) == bad and _fwd(hiplib, L, out=None) == bad
    assert _fwd(hiplib, L, ldx=4) == bad and _fwd(hiplib, L, ldo=4) == bad and _fwd(hiplib, L, ldw=4) == bad
    assert _fwd(hiplib, L, add=FAKE + 0x3000, ld_add=4) == bad and _fwd(hiplib, L, kept_x=FAKE + 0x3000, ld_kx=4) == bad
    assert _fwd(hiplib, L, K=6) == logic and _fwd(hiplib, L, K=1028, ldx=1028, ldw=1028) == logic and _fwd(hiplib, L, K=0) == logic
    assert _fwd(hiplib, L, N=6) == logic and _fwd(hiplib, L, N=260, ldo=260) == logic
    assert _fwd(hiplib, L, x=FAKE + 4) == logic                                   # a misaligned row pointer
    assert _fwd(hiplib, L, ldx=10) == logic                                       # rows 40 B apart: every other one misaligned
    assert _fwd(hiplib, L, out=FAKE + 0x2008) == logic and _fwd(hiplib, L, gamma=FAKE + 0x4004) == logic
    assert _fwd(hiplib, L, x=FAKE + 8) == logic                                   # float32 rows 8-B aligned only
    for dt in (L.DT_HALF, L.DT_BF16):
        assert _fwd(hiplib, L, x_dtype=dt, x=FAKE + 4) == logic                   # a 16-bit table 4-B but not 8-B aligned
        assert _fwd(hiplib, L, x_dtype=dt, ldx=10) == logic
    assert _fwd(hiplib, L, x_dtype=L.DT_DOUBLE) == bad
    assert _fwd(hiplib, L, n=-1) == bad
    assert _fwd(hiplib, L, ids=FAKE + 0x5000, ids_dtype=L.DT_FLOAT) == bad         # a bad id kind
    assert _fwd(hiplib, L, ids=FAKE + 0x5000, ids_dtype=L.IDS_BYTE_OFFSETS) == bad
    assert _fwd(hiplib, L, norm=3) == bad and _fwd(hiplib, L, eps=-1.0) == bad
    assert _fwd(hiplib, L, n=0) == L.WHOLEMEMORY_SUCCESS and _fwd(hiplib, L, n=0, x=None, out=None) == L.WHOLEMEMORY_SUCCESS


def test_backward_entries_refuse_before_touching_a_device(hiplib):
    from wholegraph_amd import _lib as L
    bad, logic = L.WHOLEMEMORY_INVALID_INPUT, L.WHOLEMEMORY_LOGIC_ERROR

    def bwd(**kw):
        a = dict(kept_y=FAKE, ld_ky=8, grad_out=FAKE + 0x1000, ldg=8, n=4, N=8, relu=1, norm=L.ROW_LINEAR_NORM_LAYER, gamma=None,
                 eps=1e-5, dy=FAKE + 0x2000, ld_dy=8, partials=None)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return hiplib.wgamd_row_linear_bwd_f32(*a.values(), None)

    assert bwd(kept_y=None) == bad and bwd(grad_out=None) == bad and bwd(dy=None) == bad
    assert bwd(ldg=4) == bad and bwd(ld_dy=4) == bad and bwd(ld_ky=4) == bad and bwd(n=-1) == bad and bwd(norm=-1) == bad
    assert bwd(N=6) == logic and bwd(N=260, ldg=260, ld_dy=260, ld_ky=260) == logic
    assert bwd(grad_out=FAKE + 0x1004) == logic and bwd(ld_ky=10) == logic and bwd(partials=FAKE + 0x3008) == logic
    assert bwd(n=0) == L.WHOLEMEMORY_SUCCESS and bwd(n=0, kept_y=None, dy=None) == L.WHOLEMEMORY_SUCCESS
    ag = hiplib.wgamd_row_linear_affine_grad_f32
    assert ag(None, 4, 8, FAKE, FAKE + 0x100, None) == bad                        # rows, gradients wanted, no partials
    assert ag(FAKE, -1, 8, FAKE, FAKE + 0x100, None) == bad
    assert ag(FAKE, 4, 6, FAKE, FAKE + 0x100, None) == logic
    assert ag(FAKE, 4, 8, None, None, None) == L.WHOLEMEMORY_SUCCESS              # neither gradient wanted: nothing to do
    assert hiplib.wgamd_row_linear_bwd_blocks(0, 64) == 0 and hiplib.wgamd_row_linear_bwd_blocks(16, 64) == 1
    assert hiplib.wgamd_row_linear_bwd_blocks(17, 64) == 2                        # 16 rows per workgroup pass
    assert hiplib.wgamd_row_linear_bwd_blocks(10 ** 9, 64) == 1024                # bounded: the affine launch stays small
    assert hiplib.wgamd_row_linear_bwd_blocks(5, 6) == 0
