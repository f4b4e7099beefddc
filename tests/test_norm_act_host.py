"""NormDropoutAct without a GPU: the modules' parameters and state dicts, the torch route on CPU tensors, the host-side answers
(supported widths, segment seeds, the seed sequence, the split of a dict call into launches) and the C entries' refusals, which
all come before any device call."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


def test_state_dict_is_layer_norms():
    from wholegraph_amd import nn
    C = 12
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.uniform_(-1, 1), ln.bias.uniform_(-1, 1)
    m = nn.NormDropoutAct(C)
    assert list(m.state_dict()) == list(ln.state_dict()) == ["weight", "bias"]
    assert torch.equal(m.weight, torch.ones(C)) and torch.equal(m.bias, torch.zeros(C))
    m.load_state_dict(ln.state_dict())
    assert torch.equal(m.weight, ln.weight) and torch.equal(m.bias, ln.bias)
    m.reset_parameters()
    assert torch.equal(m.weight, torch.ones(C)) and torch.equal(m.bias, torch.zeros(C))
    h = nn.HeteroNormDropoutAct({"paper": 8, "author": 4})
    assert sorted(h.state_dict()) == ["norms.author.bias", "norms.author.weight", "norms.paper.bias", "norms.paper.weight"]
    assert h.norms["paper"].weight.shape == (8,) and h.norms["author"].bias.shape == (4,)


def test_affine_variants():
    from wholegraph_amd import nn
    assert list(nn.NormDropoutAct(8, elementwise_affine=False).state_dict()) == []
    assert list(nn.NormDropoutAct(8, bias=False).state_dict()) == ["weight"]
    assert list(nn.NormDropoutAct(8, norm=False).state_dict()) == []
    x = torch.randn(5, 8)
    m = nn.NormDropoutAct(8, bias=False).eval()
    with torch.no_grad():
        m.weight.uniform_(-1, 1)
    assert torch.equal(m(x), torch.relu(F.layer_norm(x, (8,), m.weight, None, 1e-5)))
    m = nn.NormDropoutAct(8, elementwise_affine=False, relu=False).eval()
    assert torch.equal(m(x), F.layer_norm(x, (8,)))
    with pytest.raises(ValueError):
        nn.NormDropoutAct(8, p=1.5)


def test_cpu_tensors_take_the_torch_route(hiplib):
    from wholegraph_amd import nn
    torch.manual_seed(0)
    x, res = torch.randn(7, 16), torch.randn(7, 16)
    m = nn.NormDropoutAct(16, p=0.5).eval()
    with torch.no_grad():
        m.weight.uniform_(-1, 1), m.bias.uniform_(-1, 1)
    out = m(x, res)
    assert m.route == "torch"
    assert torch.equal(out, torch.relu(F.layer_norm(x + res, (16,), m.weight, m.bias, 1e-5)))
    plain = nn.NormDropoutAct(16, norm=False, p=0.0)      # (training mode, but p = 0)
    assert torch.equal(plain(x), torch.relu(x)) and plain.route == "torch"
    assert torch.equal(nn.norm_dropout_act(x, norm=False, p=0.5, training=False), torch.relu(x))
    # training on the torch route: torch's own dropout stream, an unbiased scale, gradients through ordinary autograd
    m.train()
    xg = x.clone().requires_grad_(True)
    torch.manual_seed(1)
    a = m(xg, res)
    torch.manual_seed(1)
    want = torch.relu(F.dropout(F.layer_norm(x + res, (16,), m.weight, m.bias, 1e-5), 0.5, True))
    assert torch.equal(a, want)
    a.sum().backward()
    assert xg.grad is not None and m.weight.grad is not None
    # the dict form on CPU
    h = nn.HeteroNormDropoutAct({"a": 16, "b": 4}).eval()
    xs = {"b": torch.randn(3, 4), "a": x}
    out = h(xs, {"a": res})
    assert list(out) == ["b", "a"] and h.route == "torch"
    assert torch.equal(out["a"], torch.relu(F.layer_norm(x + res, (16,)))) and torch.equal(out["b"], torch.relu(F.layer_norm(xs["b"], (4,))))
    assert list(h({"a": x})) == ["a"]                      # a type absent from x_dict is skipped


def test_supported_widths(hiplib):
    from wholegraph_amd import nn
    assert [nn.norm_dropout_act_supported(C) for C in (0, 2, 4, 6, 1024, 1028)] == [False, False, True, False, True, False]


def test_segment_seed(hiplib):
    from wholegraph_amd import nn
    seeds = [nn.segment_seed(1234, k) for k in range(16)]
    assert seeds == [nn.segment_seed(1234, k) for k in range(16)] and len(set(seeds)) == 16
    assert all(0 <= s < 2 ** 64 for s in seeds)
    assert nn.segment_seed(1234, 0) != nn.segment_seed(1235, 0)
    hiplib.wgamd_norm_act_segment_seed.restype = ctypes.c_ulonglong
    for seed, k in [(0, 0), (1234, 5), (2 ** 64 - 1, 7), (0x9E3779B97F4A7C15, 3)]:       # the host twin of the launch's own
        assert nn.segment_seed(seed, k) == hiplib.wgamd_norm_act_segment_seed(ctypes.c_ulonglong(seed), k)


def test_default_seed_sequence_repeats_after_manual_seed():
    from wholegraph_amd import nn
    torch.manual_seed(11)
    a = [nn._norm_act_auto_seed() for _ in range(4)]
    torch.manual_seed(11)
    b = [nn._norm_act_auto_seed() for _ in range(4)]
    torch.manual_seed(12)
    c = [nn._norm_act_auto_seed() for _ in range(4)]
    assert a == b and len(set(a)) == 4 and not set(a) & set(c)


def test_dict_call_splits_into_launches_of_eight():
    from wholegraph_amd import nn
    assert [list(r) for r in nn._norm_act_chunks(9)] == [list(range(8)), [8]]
    assert [list(r) for r in nn._norm_act_chunks(8)] == [list(range(8))]
    assert [list(r) for r in nn._norm_act_chunks(17)] == [list(range(8)), list(range(8, 16)), [16]]
    assert nn._norm_act_chunks(0) == []


def _segment(L, **kw):
    fake = 0x10000       # never dereferenced: every refusal comes before a device call
    s = L.NormActSegment()
    s.x, s.ldx, s.out, s.ldo, s.n_rows, s.C, s.seed_index = fake, 8, fake + 0x1000, 8, 4, 8, -1
    s.grad_out, s.ldg, s.grad_in, s.ld_gi = fake + 0x2000, 8, fake + 0x3000, 8
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("entry", ["wgamd_norm_act_f32", "wgamd_norm_act_bwd_f32"])
def test_c_entries_refuse_before_touching_a_device(hiplib, entry):
    from wholegraph_amd import _lib as L
    fn = getattr(hiplib, entry)

    def call(segs, n=None, flags=L.NORM_ACT_RELU):
        arr = (L.NormActSegment * max(len(segs), 1))(*segs)
        return fn(arr, len(segs) if n is None else n, 1e-5, 0.5, 7, flags, None)

    assert call([_segment(L)], n=0) == L.WHOLEMEMORY_INVALID_INPUT
    assert call([_segment(L)] * 9) == L.WHOLEMEMORY_INVALID_INPUT
    assert fn(None, 1, 1e-5, 0.5, 7, 0, None) == L.WHOLEMEMORY_INVALID_INPUT
    assert call([_segment(L, x=None)]) == L.WHOLEMEMORY_INVALID_INPUT
    assert call([_segment(L, C=6)]) == L.WHOLEMEMORY_LOGIC_ERROR
    assert call([_segment(L, C=1028, ldx=1028, ldo=1028)]) == L.WHOLEMEMORY_LOGIC_ERROR
    assert call([_segment(L, ldx=4)]) == L.WHOLEMEMORY_INVALID_INPUT
    assert call([_segment(L, x=0x10004)]) == L.WHOLEMEMORY_LOGIC_ERROR           # a misaligned row pointer
    assert call([_segment(L, ldx=10)]) == L.WHOLEMEMORY_LOGIC_ERROR              # rows 40 B apart: every other one misaligned
    assert call([_segment(L, residual=0x20008, ld_res=8)]) == L.WHOLEMEMORY_LOGIC_ERROR
    assert call([_segment(L, n_rows=-1)]) == L.WHOLEMEMORY_INVALID_INPUT
    assert call([_segment(L)], flags=L.NORM_ACT_NORM | L.NORM_ACT_SAVE_STATS) == L.WHOLEMEMORY_INVALID_INPUT      # null stats
    assert fn((L.NormActSegment * 1)(_segment(L)), 1, 1e-5, 1.5, 7, 0, None) == L.WHOLEMEMORY_INVALID_INPUT       # p > 1
    # nothing to do is not an error: every segment empty -> no launch
    assert call([_segment(L, n_rows=0, x=None), _segment(L, n_rows=0)]) == L.WHOLEMEMORY_SUCCESS


def test_wgrad_entry_refuses(hiplib):
    from wholegraph_amd import _lib as L
    arr = (L.NormActSegment * 1)(_segment(L))
    assert hiplib.wgamd_norm_act_wgrad_f32(arr, 0, None) == L.WHOLEMEMORY_INVALID_INPUT
    assert hiplib.wgamd_norm_act_wgrad_f32(arr, 9, None) == L.WHOLEMEMORY_INVALID_INPUT
    assert hiplib.wgamd_norm_act_wgrad_f32(arr, 1, None) == L.WHOLEMEMORY_SUCCESS          # neither dweight nor dbias: skipped
    arr = (L.NormActSegment * 1)(_segment(L, dweight=0x40000))
    assert hiplib.wgamd_norm_act_wgrad_f32(arr, 1, None) == L.WHOLEMEMORY_INVALID_INPUT    # a gradient wanted, rows, no partials
    assert hiplib.wgamd_norm_act_bwd_blocks(0, 64) == 0 and hiplib.wgamd_norm_act_bwd_blocks(1, 64) == 1
    assert hiplib.wgamd_norm_act_bwd_blocks(17, 64) == 2                  # 16 rows of 16 lanes per 256-thread workgroup pass
    assert hiplib.wgamd_norm_act_bwd_blocks(10 ** 9, 64) == 1024          # bounded: the weight-gradient launch stays small
    assert hiplib.wgamd_norm_act_bwd_blocks(5, 6) == 0
