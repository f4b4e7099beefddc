"""Host-side checks of wholegraph_amd.nn.MLP and the batch-norm route of GINConv (no GPU): PyG's state-dict keys of
``MLP([...])`` and a strict round trip, the CPU forward in train and eval mode bit for bit against a ``torch.nn.Sequential`` over
the same parameters (running statistics included), the route every ``MLP`` form selects, the refused arguments, and the new C
entries' refusals before any device call."""
import pytest
import torch

from wholegraph_amd.nn import MLP, GINConv

T = torch.nn
PYG_KEYS = ["lins.0.bias", "lins.0.weight", "lins.1.bias", "lins.1.weight", "norms.0.module.bias", "norms.0.module.num_batches_tracked",
            "norms.0.module.running_mean", "norms.0.module.running_var", "norms.0.module.weight"]


def test_state_dict_keys_are_pygs():
    mlp = MLP([64, 32, 8])
    assert sorted(mlp.state_dict()) == PYG_KEYS
    assert type(mlp.lins[0]) is T.Linear and type(mlp.norms[0].module) is T.BatchNorm1d and len(mlp.norms) == 1
    assert sorted(GINConv(mlp).state_dict()) == ["eps"] + ["nn." + k for k in PYG_KEYS]
    assert sorted(MLP([64, 32, 8], norm=None).state_dict()) == PYG_KEYS[:4]
    deep = MLP([8, 16, 16, 4], plain_last=False, norm_kwargs={"eps": 1e-3, "momentum": 0.2})
    assert len(deep.lins) == 3 and len(deep.norms) == 3 and deep.norms[2].module.eps == 1e-3 and deep.norms[0].module.momentum == 0.2
    assert deep.dropout == [0.0, 0.0, 0.0] and MLP([8, 16, 4], dropout=0.5).dropout == [0.5, 0.0]


def test_state_dict_round_trip_strict():
    torch.manual_seed(0)
    a, b = MLP([64, 32, 8]), MLP([64, 32, 8])
    a.train()
    a(torch.randn(50, 64))                       # non-trivial running statistics
    want = {k: v.clone() for k, v in a.state_dict().items()}
    assert list(want) and int(want["norms.0.module.num_batches_tracked"]) == 1
    res = b.load_state_dict(want, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in b.state_dict().items():
        assert torch.equal(v, want[k]), k
    with pytest.raises(RuntimeError):
        b.load_state_dict({k: v for k, v in want.items() if k != "lins.1.bias"}, strict=True)


@pytest.mark.parametrize("kw", [{}, {"act_first": True}, {"norm": None}, {"act": None}, {"plain_last": False}])
def test_cpu_forward_equals_a_sequential_over_the_same_parameters(kw):
    torch.manual_seed(1)
    mlp = MLP([12, 20, 20, 6], **kw)
    seq = T.Sequential(*mlp.flat_modules())
    kinds = [type(m).__name__ for m in seq]
    if not kw:
        assert kinds == ["Linear", "BatchNorm1d", "ReLU", "Linear", "BatchNorm1d", "ReLU", "Linear"]
    if kw.get("act_first"):
        assert kinds[:3] == ["Linear", "ReLU", "BatchNorm1d"]
    x = torch.randn(40, 12)
    # the Sequential shares the BatchNorm modules: compare the running statistics of separate, identical steps
    state = {k: v.clone() for k, v in mlp.state_dict().items()}
    mlp.train()
    got = mlp(x)
    after = {k: v.clone() for k, v in mlp.state_dict().items()}
    mlp.load_state_dict(state)
    seq.train()
    want = seq(x)
    assert torch.equal(got, want)
    for k, v in mlp.state_dict().items():
        assert torch.equal(v, after[k]), k
    if kw.get("norm", "batch_norm") is not None:
        assert int(after["norms.0.module.num_batches_tracked"]) == 1
        assert not torch.equal(after["norms.0.module.running_mean"], state["norms.0.module.running_mean"])
    mlp.eval()
    seq.eval()
    assert torch.equal(mlp(x), seq(x))
    # dropout: the flat list carries it in the module's training mode
    drop = MLP([12, 20, 6], dropout=0.5)
    assert [type(m).__name__ for m in drop.flat_modules()] == ["Linear", "BatchNorm1d", "ReLU", "Dropout", "Linear"]
    assert drop.flat_modules()[3].training and not drop.eval().flat_modules()[3].training
    torch.manual_seed(5)
    a = drop.train()(x)
    torch.manual_seed(5)
    b = T.Sequential(*drop.flat_modules())(x)
    assert a.shape == (40, 6) and torch.equal(a.detach(), b.detach())     # the same mask, the same batch statistics


def test_reset_parameters():
    mlp = MLP([4, 8, 4])
    with torch.no_grad():
        mlp.lins[1].bias.fill_(100.0)
        mlp.norms[0].module.weight.fill_(3.0)
        mlp.norms[0].module.running_mean.fill_(7.0)
    mlp.reset_parameters()
    assert float(mlp.lins[1].bias.detach().abs().max()) <= 0.5 and float(mlp.norms[0].module.weight.detach().min()) == 1.0
    assert float(mlp.norms[0].module.running_mean.abs().max()) == 0.0


def test_routes(hiplib):
    Seq, Lin = T.Sequential, T.Linear
    assert GINConv(MLP([64, 32, 8])).route == "mlp_bn"
    assert GINConv(MLP([100, 256, 256])).route == "mlp_bn" and GINConv(MLP([4, 4, 1])).route == "mlp_bn"
    assert GINConv(MLP([64, 32, 8], norm_kwargs={"eps": 1e-3, "momentum": 0.3})).route == "mlp_bn"
    plan = GINConv(MLP([64, 32, 8], norm=None))._plan()
    assert plan[0] == "mlp" and plan[2] is True and plan[4] == []
    # outside the route's domain: the existing rules over the flat module list
    for mlp, flat_tail in ((MLP([64, 32, 8], dropout=0.5), ["BatchNorm1d", "ReLU", "Dropout", "Linear"]),
                           (MLP([64, 32, 32, 8]), ["BatchNorm1d", "ReLU", "Linear", "BatchNorm1d", "ReLU", "Linear"]),
                           (MLP([64, 30, 8]), ["BatchNorm1d", "ReLU", "Linear"]),
                           (MLP([64, 32, 8], plain_last=False), ["BatchNorm1d", "ReLU", "Linear", "BatchNorm1d", "ReLU"]),
                           (MLP([64, 32, 8], act=None), ["BatchNorm1d", "Linear"])):
        conv = GINConv(mlp)
        plan = conv._plan()
        assert conv.route == "linear" and plan[2] is False and [type(m).__name__ for m in plan[4]] == flat_tail, flat_tail
        same = GINConv(Seq(*mlp.flat_modules()))._plan()
        assert plan[0] == same[0] and plan[1] is same[1] and plan[2] == same[2]
    plan = GINConv(MLP([64, 32, 8], act_first=True))._plan()           # Linear, ReLU, BatchNorm1d, Linear: the ReLU rides along
    assert plan[0] == "linear" and plan[2] is True and [type(m).__name__ for m in plan[4]] == ["BatchNorm1d", "Linear"]
    assert GINConv(MLP([300, 64, 64])).route == "aggregate"
    assert GINConv(MLP([300, 64, 64], norm=None)).route == "aggregate"
    assert GINConv(MLP([64, 30, 8], norm=None)).route == "linear"
    bn = MLP([64, 32, 8])
    bn.norms[0].module.momentum = None                                  # cumulative average: not the route's
    assert GINConv(bn).route == "linear"
    # the plain Sequential keeps its route
    conv = GINConv(Seq(Lin(64, 32), T.BatchNorm1d(32), T.ReLU(), Lin(32, 8)))
    assert conv.route == "linear" and [type(m).__name__ for m in conv._plan()[4]] == ["BatchNorm1d", "ReLU", "Linear"]


def test_bad_arguments_are_named():
    for kw, name in (({"norm": "layer_norm"}, "norm"), ({"act": "elu"}, "act"), ({"norm_kwargs": {"affine": False}}, "norm_kwargs"),
                     ({"dropout": 1.5}, "dropout"), ({"bias": [True, False]}, "bias")):
        with pytest.raises(ValueError, match=name):
            MLP([8, 8, 8], **kw)
    with pytest.raises(ValueError, match="channel_list"):
        MLP([8])


def test_cpu_layer_runs_the_mlp_after_the_aggregate():
    torch.manual_seed(2)
    x = torch.randn(6, 8)
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 0], [1, 2, 3, 4, 5, 0, 3]])
    conv = GINConv(MLP([8, 12, 4]), eps=0.5)
    agg = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]]) + 1.5 * x
    lin1, bn, lin2 = conv.nn.lins[0], conv.nn.norms[0].module, conv.nn.lins[1]
    z = lin1(agg)
    want = lin2(torch.relu((z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + bn.eps)))
    got = conv(x, ei)
    assert torch.allclose(got, want, atol=1e-5) and int(bn.num_batches_tracked) == 1
    conv.eval()
    want = torch.relu(lin2(torch.relu((z - bn.running_mean) / torch.sqrt(bn.running_var + bn.eps))))
    assert torch.allclose(conv(x, ei, act="relu"), want, atol=1e-5) and int(bn.num_batches_tracked) == 1


FAKE = 0x100000      # never dereferenced: every refusal comes before a device call


def test_new_entries_are_exported_and_refuse_before_touching_a_device(hiplib):
    from wholegraph_amd import _lib as L
    bad, logic = L.WHOLEMEMORY_INVALID_INPUT, L.WHOLEMEMORY_LOGIC_ERROR
    for name in ("wgamd_batch_norm_supported", "wgamd_bn_bwd_blocks", "wgamd_gin_layer_f32_stats", "wgamd_bn_partials_f32",
                 "wgamd_bn_finalize_f32", "wgamd_bn_act_linear_f32", "wgamd_bn_bwd_reduce_f32", "wgamd_bn_bwd_apply_f32"):
        assert hasattr(hiplib, name), name
    sup = hiplib.wgamd_batch_norm_supported
    assert sup(4) and sup(36) and sup(256) and not sup(0) and not sup(30) and not sup(260)
    blocks = hiplib.wgamd_bn_bwd_blocks
    assert blocks(0, 64) == 0 and blocks(16, 64) == 1 and blocks(17, 64) == 2 and blocks(10 ** 9, 64) == 1024 and blocks(5, 6) == 0
    P = [FAKE + 0x1000 * k for k in range(12)]

    def stats(**kw):
        a = dict(row_ptr=P[0], col=P[1], n=4, x=P[2], ldx=8, F=8, ids=None, ids_dtype=0, self_rows=None, x_dst=None, ldx_dst=0, eps=None,
                 w1=P[3], ldw1=8, H=8, b1=None, z=P[4], ldz=8, agg=None, ld_agg=0, partials=P[5], counts=P[6], tile0=0)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return hiplib.wgamd_gin_layer_f32_stats(*a.values(), None)
    assert stats(x=None) == bad and stats(w1=None) == bad and stats(z=None) == bad and stats(partials=None) == bad
    assert stats(counts=None) == bad and stats(row_ptr=None) == bad
    assert stats(ldx=4) == bad and stats(ldw1=4) == bad and stats(ldz=4) == bad and stats(agg=P[7], ld_agg=4) == bad
    assert stats(n=-1) == bad and stats(tile0=-1) == bad
    assert stats(H=6) == logic and stats(H=260, ldz=260) == logic and stats(F=6) == logic
    assert stats(z=P[4] + 4) == logic and stats(ldz=10) == logic and stats(x=P[2] + 8) == logic
    assert stats(n=0) == L.WHOLEMEMORY_SUCCESS

    part = hiplib.wgamd_bn_partials_f32
    assert part(None, 8, 4, 8, P[1], P[2], 0, None) == bad and part(P[0], 8, 4, 8, None, P[2], 0, None) == bad
    assert part(P[0], 8, 4, 8, P[1], None, 0, None) == bad and part(P[0], 4, 4, 8, P[1], P[2], 0, None) == bad
    assert part(P[0], 8, 4, 6, P[1], P[2], 0, None) == logic and part(P[0] + 4, 8, 4, 8, P[1], P[2], 0, None) == logic
    assert part(P[0], 8, 0, 8, P[1], P[2], 0, None) == L.WHOLEMEMORY_SUCCESS

    def fin(partials=P[0], counts=P[1], T=3, H=8, mean=P[2], eps=1e-5):
        return hiplib.wgamd_bn_finalize_f32(partials, counts, T, H, None, None, eps, 0.1, None, None, mean, None, None, None, None, None)
    assert fin(partials=None) == bad and fin(counts=None) == bad and fin(mean=None) == bad and fin(T=-1) == bad and fin(eps=-1.0) == bad
    assert fin(H=6) == logic and fin(H=0) == logic and fin(partials=P[0] + 8) == logic

    def tail(**kw):
        a = dict(z=P[0], ldz=8, n=4, H=8, scale=P[1], shift=P[2], w2=P[3], ldw2=8, N=8, b2=None, relu=0, out=P[4], ldo=8, hidden=None,
                 ld_hidden=0)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return hiplib.wgamd_bn_act_linear_f32(*a.values(), None)
    assert tail(z=None) == bad and tail(scale=None) == bad and tail(shift=None) == bad and tail(w2=None) == bad and tail(out=None) == bad
    assert tail(ldz=4) == bad and tail(ldw2=4) == bad and tail(ldo=4) == bad and tail(hidden=P[5], ld_hidden=4) == bad
    assert tail(H=6) == logic and tail(N=0) == logic and tail(N=260, ldo=260) == logic and tail(w2=P[3] + 4) == logic
    assert tail(scale=P[1] + 4) == logic and tail(ldz=10) == logic
    assert tail(n=0) == L.WHOLEMEMORY_SUCCESS

    def bwd(entry, **kw):
        a = dict(dh=P[0], ld_dh=8, hidden=P[1], ld_hidden=8, z=P[2], ldz=8, n=4, H=8, mean=P[3], rstd=P[4])
        tails = {"reduce": dict(partials=P[5], dgamma=P[6], dbeta=P[7]),
                 "apply": dict(gamma=P[8], dgamma=P[6], dbeta=P[7], dz=P[9], ld_dz=8)}
        a.update(tails[entry])
        assert set(kw) <= set(a), kw
        a.update(kw)
        return getattr(hiplib, "wgamd_bn_bwd_%s_f32" % entry)(*a.values(), None)
    for entry in ("reduce", "apply"):
        assert bwd(entry, dh=None) == bad and bwd(entry, hidden=None) == bad and bwd(entry, z=None) == bad
        assert bwd(entry, mean=None) == bad and bwd(entry, rstd=None) == bad and bwd(entry, dgamma=None) == bad
        assert bwd(entry, ld_dh=4) == bad and bwd(entry, ld_hidden=4) == bad and bwd(entry, ldz=4) == bad and bwd(entry, n=-1) == bad
        assert bwd(entry, H=6) == logic and bwd(entry, H=260) == logic and bwd(entry, z=P[2] + 4) == logic and bwd(entry, ldz=10) == logic
    assert bwd("reduce", partials=None) == bad and bwd("apply", dz=None) == bad and bwd("apply", ld_dz=4) == bad
    assert bwd("apply", dz=P[9] + 4) == logic and bwd("apply", n=0) == L.WHOLEMEMORY_SUCCESS
