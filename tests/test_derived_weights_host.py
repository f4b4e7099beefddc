"""``nn._derived``, the one cache of the weights' derived forms (transposed, padded, stacked, folded, split), on CPU tensors: the
helper alone with a counting ``build``, then through the layers that keep their forms with it — a hit is the stored object
itself, a form is stale exactly when a parameter changed behind the version counter and fresh again after
``bump_weight_generation``, and ``grad=True`` builds under autograd and keeps nothing."""
import pytest
import torch

ETS = [("a", "r1", "a"), ("b", "r2", "a")]


class Counting:
    """``build`` of a derived form of ``p``: ``2 p`` (differentiable), counting its calls."""

    def __init__(self, p):
        self.p, self.calls = p, 0

    def __call__(self):
        self.calls += 1
        return self.p * 2.0


class Holder:
    pass


class NoDict:
    __slots__ = ()


@pytest.fixture
def nn():
    from wholegraph_amd import nn
    return nn


def test_hit_is_the_stored_object(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    a = nn._derived(h, "f", (p,), build)
    assert nn._derived(h, "f", (p,), build) is a and build.calls == 1
    assert torch.equal(a, torch.full((3,), 2.0))


def test_miss_after_a_version_bump(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    a = nn._derived(h, "f", (p,), build)
    with torch.no_grad():
        p.add_(1)
    b = nn._derived(h, "f", (p,), build)
    assert b is not a and build.calls == 2 and torch.equal(b, torch.full((3,), 4.0))


def test_miss_after_the_storage_moved(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    a = nn._derived(h, "f", (p,), build)
    p.data = p.data.clone()
    assert nn._derived(h, "f", (p,), build) is not a and build.calls == 2


def test_stale_behind_the_version_counter_until_the_generation_bump(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    v0 = p._version
    a = nn._derived(h, "f", (p,), build)
    p.data.add_(1)
    assert p._version == v0                                  # .data leaves the version alone ...
    assert nn._derived(h, "f", (p,), build) is a             # ... so the form is stale: 2, not 4
    nn.bump_weight_generation()
    b = nn._derived(h, "f", (p,), build)
    assert b is not a and build.calls == 2 and torch.equal(b, torch.full((3,), 4.0))
    with torch.no_grad():
        p.add_(1)
    assert p._version == v0 + 1


def test_extra_is_part_of_the_key(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    a = nn._derived(h, "f", (p,), build, extra=64)
    assert nn._derived(h, "f", (p,), build, extra=128) is not a and build.calls == 2
    assert nn._derived(h, "f", (p,), build, extra=128) is nn._derived(h, "f", (p,), build, extra=128) and build.calls == 2


def test_names_do_not_share_a_slot(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    a, b = nn._derived(h, "f", (p,), build), nn._derived(h, "g", (p,), build)
    assert a is not b and nn._derived(h, "f", (p,), build) is a and nn._derived(h, "g", (p,), build) is b and build.calls == 2


def test_a_none_param(nn):
    p, q, h = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.zeros(3)), Holder()
    build = Counting(p)
    a = nn._derived(h, "f", (p, None), build)
    assert nn._derived(h, "f", (p, None), build) is a and build.calls == 1
    assert nn._derived(h, "f", (p, q), build) is not a and build.calls == 2      # (a bias that appeared)


def test_a_holder_without_dict_rebuilds_every_time(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), NoDict()
    build = Counting(p)
    a, b = nn._derived(h, "f", (p,), build), nn._derived(h, "f", (p,), build)
    assert a is not b and build.calls == 2 and torch.equal(a, b)


def test_a_tensor_holds_its_own_forms(nn):
    w = torch.ones(3)
    build = Counting(w)
    a = nn._derived(w, "f", (w,), build)
    assert nn._derived(w, "f", (w,), build) is a and build.calls == 1
    w.add_(1)
    assert torch.equal(nn._derived(w, "f", (w,), build), torch.full((3,), 4.0)) and build.calls == 2


def test_grad_builds_under_autograd_and_stores_nothing(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    build = Counting(p)
    with torch.no_grad():                                    # (enable_grad is the helper's own)
        a = nn._derived(h, "f", (p,), build, grad=True)
    assert a.grad_fn is not None and not hasattr(h, "_wgamd_derived")
    a.sum().backward()
    assert torch.equal(p.grad, torch.full((3,), 2.0))
    b = nn._derived(h, "f", (p,), build, grad=True)
    assert b is not a and build.calls == 2
    c = nn._derived(h, "f", (p,), build)                     # the cached twin: a third build, then hits
    assert c.grad_fn is None and nn._derived(h, "f", (p,), build) is c and build.calls == 3


def test_a_stored_value_never_requires_grad(nn):
    p, h = torch.nn.Parameter(torch.ones(3)), Holder()
    a = nn._derived(h, "same", (p,), lambda: p)              # (``_sum_of`` of one bias returns the parameter itself)
    assert not a.requires_grad and not isinstance(a, torch.nn.Parameter) and a.data_ptr() == p.data_ptr()
    b = nn._derived(h, "nested", (p,), lambda: (p * 2.0, [p, None], "layout", 3))
    assert isinstance(b, tuple) and isinstance(b[1], list) and b[1][1] is None and b[2:] == ("layout", 3)
    assert not b[0].requires_grad and b[0].grad_fn is None and not b[1][0].requires_grad


# ---- through the layers -----------------------------------------------------------------------------------------------------
def _tconv(nn):
    return nn.TransformerConv(16, 8, heads=2)


def _hetero(nn, kind):
    if kind == "sage":
        convs = {et: nn.SAGEConv((8, 8), 4) for et in ETS}
    elif kind == "gat":
        convs = {et: nn.GATConv(8, 4, heads=2) for et in ETS}
    else:
        convs = {et: nn.TransformerConv((8, 8), 4, heads=2) for et in ETS}
    return nn.HeteroConv(convs)


# name -> (module factory, form(module, grad), the parameter that changes, whether the form has a differentiable twin)
CASES = {
    "tconv_folds": (_tconv, lambda m, grad: m._folds(), lambda m: m.lin_query.weight, True),
    "hetero_sage_weights": (lambda nn: _hetero(nn, "sage"), lambda m, grad: m._sage_weights("a", grad=grad),
                            lambda m: m.conv(ETS[1]).lin_l.weight, True),
    "hetero_sage_bias": (lambda nn: _hetero(nn, "sage"), lambda m, grad: m._bias("a"), lambda m: m.conv(ETS[0]).lin_l.bias, False),
    "hetero_gat_rel": (lambda nn: _hetero(nn, "gat"), lambda m, grad: m._rel(ETS[1]), lambda m: m.conv(ETS[1]).att_src, False),
    "hetero_gat_terms": (lambda nn: _hetero(nn, "gat"), lambda m, grad: m._terms_matrix("a"), lambda m: m.conv(ETS[0]).att_dst, False),
    "hetero_gat_bias": (lambda nn: _hetero(nn, "gat"), lambda m, grad: m._bias("a"), lambda m: m.conv(ETS[1]).bias, False),
    "hetero_tconv_weights": (lambda nn: _hetero(nn, "tconv"), lambda m, grad: m._tconv_weights(ETS, grad=grad),
                             lambda m: m.conv(ETS[0]).lin_value.weight, True),
}


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


def _tensors(v):
    if torch.is_tensor(v):
        return [v]
    return [t for u in v for t in _tensors(u)] if isinstance(v, (tuple, list)) else []


def _fresh(nn, make, form, module):
    """The form of a newly made module that carries ``module``'s parameters: nothing kept from before."""
    other = make(nn)
    other.load_state_dict(module.state_dict())
    return form(other, False)


@pytest.mark.parametrize("case", sorted(CASES))
def test_layer_form_hits_and_follows_its_parameters(nn, case):
    make, form, param, _ = CASES[case]
    torch.manual_seed(3)
    m = make(nn)
    with torch.no_grad():
        a = form(m, False)
        assert form(m, False) is a                                           # a hit is the stored object
        assert all(not t.requires_grad and not isinstance(t, torch.nn.Parameter) for t in _tensors(a))
        param(m).add_(0.5)                                                   # an optimizer's in-place step: the version moves
        b = form(m, False)
        assert b is not a and not _same(a, b) and _same(b, _fresh(nn, make, form, m))
        assert form(m, False) is b
        param(m).data.add_(0.25)                                             # behind the counter (a graph replay): stale ...
        assert form(m, False) is b and not _same(b, _fresh(nn, make, form, m))
        nn.bump_weight_generation()                                          # ... until the generation moves
        c = form(m, False)
        assert c is not b and _same(c, _fresh(nn, make, form, m))


@pytest.mark.parametrize("case", sorted(k for k, v in CASES.items() if v[3]))
def test_layer_form_under_autograd_reaches_the_parameter(nn, case):
    make, form, param, _ = CASES[case]
    torch.manual_seed(4)
    m = make(nn)
    assert all(p.requires_grad for p in m.parameters())
    a = form(m, True)                                                        # (``_folds``: grad mode on a requires_grad parameter)
    assert form(m, True) is not a                                            # nothing kept
    ts = [t for t in _tensors(a) if t.is_floating_point()]
    assert ts and all(t.requires_grad for t in ts) and any(t.grad_fn is not None for t in ts)   # (a lone bias is the leaf itself)
    sum((t * t).sum() for t in ts).backward()
    g = param(m).grad
    assert g is not None and bool((g != 0).any())
    with torch.no_grad():                                                    # the cached twin: same values, no history
        b = form(m, False)
    assert all(t.grad_fn is None and not t.requires_grad for t in _tensors(b))
    assert all(torch.equal(u, v) for u, v in zip(_tensors(a), _tensors(b)))
