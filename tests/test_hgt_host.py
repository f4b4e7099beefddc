"""Host-side checks of wholegraph_amd.nn.HGTConv (no GPU, the torch route): forward against the float64 restatement
(tests/hgt_ref.py) on a three-relation graph, the state-dict names and shapes, a type without incoming relation, the domain."""
import torch

from hgt_ref import hgt_forward, layer_graph, params_of
from wholegraph_amd import nn

ETS = [("a", "r1", "a"), ("b", "r2", "a"), ("a", "r3", "b")]
META = (["a", "b", "c"], ETS + [("c", "r4", "c")])


def test_torch_route_equals_restatement():
    torch.manual_seed(3)
    conv = nn.HGTConv({"a": 8, "b": 12, "c": 8}, 8, META, heads=2).double()
    with torch.no_grad():
        for p in conv.p_rel.values():
            p.uniform_(0.5, 2.0)
        conv.skip["a"].fill_(0.3)
    x = {"a": torch.rand(5, 8, dtype=torch.float64) * 2 - 1, "b": torch.rand(4, 12, dtype=torch.float64) * 2 - 1}
    ei = {ETS[0]: torch.tensor([[1, 2, 2, 4], [0, 0, 3, 3]]), ETS[1]: torch.tensor([[3, 0, 1], [3, 0, 4]]),      # none into a[1], a[2]
          ETS[2]: torch.tensor([[0, 4, 4], [2, 2, 0]])}
    with torch.no_grad():
        out = conv(x, ei, act="relu")
    assert conv.route == "torch" and sorted(out) == ["a", "b"]          # c: no rows, no relation of the graph ends in it
    graph = layer_graph({et: (e[0], e[1]) for et, e in ei.items()}, {"a": torch.arange(5), "b": torch.arange(4)}, META[0])
    ref = hgt_forward(x, graph, params_of(conv), META[1], 2, relu=True)
    with torch.no_grad():
        again = conv(x, graph, act="relu")
    for t in ref:
        assert float((out[t] - ref[t]).abs().max()) <= 1e-12 * float(ref[t].abs().max()), t
        assert torch.equal(out[t], again[t])
    assert float(out["a"][1].abs().sum()) > 0                            # a row without edges: out_lin's bias, gated


def test_state_dict_names_and_shapes():
    sd = nn.HGTConv({"a": 8, "b": 12, "c": 8}, 8, META, heads=2).state_dict()
    want = {"k_rel.weight": (8, 4, 4), "v_rel.weight": (8, 4, 4)}
    for t, f in (("a", 8), ("b", 12), ("c", 8)):
        want.update({"kqv_lin.lins.%s.weight" % t: (24, f), "kqv_lin.lins.%s.bias" % t: (24,), "out_lin.lins.%s.weight" % t: (8, 8),
                     "out_lin.lins.%s.bias" % t: (8,), "skip.%s" % t: (1,)})
    want.update({"p_rel." + "__".join(et): (1, 2) for et in META[1]})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(float(sd[k].min()) == 1.0 == float(sd[k].max()) for k in sd if k.startswith(("skip.", "p_rel.")))


def test_shape_domain(hiplib):
    assert nn.hgt_layer_supported(1, 4, 1) and not nn.hgt_layer_supported(1, 6, 1)                # D = 4, D = 6
    assert nn.hgt_layer_supported(8, 256, 3) and not nn.hgt_layer_supported(5, 260, 3)            # C = 256, C = 260
    assert nn.hgt_layer_supported(4, 64, 8) and not nn.hgt_layer_supported(4, 64, 9)              # 8 and 9 relations
