"""tests/hetero_launch_ref.py, the parts that need no GPU: the launch-level float64 restatements against the layer-level ones
(tests/hetero_sage_ref.py, tests/hetero_transformer_ref.py) on one small case each, and the case table of
tests/test_gpu_hetero_sage_launch.py — every case builds, holds the piece-straddling and late-slot facts it is there for, lists every
value the launch-level tests are to cover, and keeps the integer-valued block sums below 2^24 (so that a float32 sum is exact in
any order and the GPU test can ask for equality)."""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_launch_ref as lref  # noqa: E402
import hetero_sage_ref as sref  # noqa: E402
import hetero_transformer_ref as href  # noqa: E402
import test_gpu_hetero_sage_launch as cases  # noqa: E402
from test_hetero_transformer_host import ETS, edge_attrs, hand_built, make_layer  # noqa: E402

# ---- one small SAGE group: two relations into type "a" over 20 frontier entries, output rows a permutation into 25 ----
_g = torch.Generator().manual_seed(21)
N_ROWS, N_OUT, N_W = 20, 25, 6
EA, EB = ("a", "to", "a"), ("b", "to", "a")
X = {"a": torch.randn((30, 8), generator=_g), "b": torch.randn((17, 12), generator=_g)}
DST_ROWS = torch.randperm(30, generator=_g)[:N_ROWS].contiguous()
OUT_ROWS = torch.randperm(N_OUT, generator=_g)[:N_ROWS].contiguous()
HOP_A = lref.edge_case_hop(N_ROWS, 30, [0, 1, 3, 4, 5, 0, 2, 9, 0, 2] * 2, seed=1)
HOP_B = lref.edge_case_hop(N_ROWS, 17, [2, 0, 0, 1, 0, 17, 1, 0, 3, 1] * 2, seed=2)


def _sage_params(both):
    g = torch.Generator().manual_seed(22)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    return {EA: dict(Wl=r(N_W, 8), bl=r(N_W), Wr=r(N_W, 8), mean=True),
            EB: dict(Wl=r(N_W, 12), bl=r(N_W) if both else None, Wr=r(N_W, 8) if both else None, mean=False)}


def _sage_graph():
    rel = lambda et, hop: types.SimpleNamespace(hop=0, edge_type=et, n_rows=N_ROWS, row_ptr=hop[0], col=hop[1],  # noqa: E731
                                                n_edges=int(hop[1].shape[0]), dst_rows=DST_ROWS, out_rows=OUT_ROWS)
    return types.SimpleNamespace(relations=[rel(EA, HOP_A), rel(EB, HOP_B)], n_out={"a": N_OUT})


def test_edge_case_hop_follows_the_degree_list():
    deg = [0, 3, 0, 0, 7, 1]
    row_ptr, col = lref.edge_case_hop(6, 5, deg, seed=3)
    assert row_ptr.dtype == torch.int32 and col.dtype == torch.int32
    assert (row_ptr[1:] - row_ptr[:-1]).tolist() == deg and col.shape[0] == 11 and int(col.min()) >= 0 and int(col.max()) < 5
    assert torch.equal(col, lref.edge_case_hop(6, 5, deg, seed=3)[1])


def test_sage_launch_restatement_matches_the_layer_restatement():
    graph = _sage_graph()
    for both in (True, False):
        p = _sage_params(both)
        wr = p[EA]["Wr"].double() + (p[EB]["Wr"].double() if both else 0)          # (summed in float64, as the restatement adds them)
        wt = torch.cat([p[EA]["Wl"].double(), p[EB]["Wl"].double(), wr], 1)
        bias = p[EA]["bl"].double() + (p[EB]["bl"].double() if both else 0)
        rels = [HOP_A + (X["a"], None, None, True), HOP_B + (X["b"], None, None, False)]
        for relu in (False, True):
            out, C, mag = lref.hetero_sage_launch_ref(rels, N_ROWS, wt, N_W, root=(X["a"], DST_ROWS, None), bias=bias, relu=relu,
                                                      out_rows=OUT_ROWS, n_out=N_OUT)
            want = sref.hetero_sage_forward(X, graph, p, relu=relu)["a"]
            assert C.shape == (N_ROWS, 28) and out.shape == (N_OUT, N_W)
            assert float((out[OUT_ROWS] - want[OUT_ROWS]).abs().max()) <= 1e-12 * float(want.abs().max())
            named = torch.zeros(N_OUT, dtype=torch.bool)
            named[OUT_ROWS] = True
            assert bool(torch.isnan(out[~named]).all()) and float(mag[~named].abs().max()) == 0.0
        # the magnitude sum: the layer restatement's where one relation alone has a root weight and a bias; with two, the launch
        # sees their sums (|W_a + W_b| <= |W_a| + |W_b|): never larger
        want_mag = sref.hetero_sage_forward(X, graph, p, abs_terms=True)["a"]
        if both:
            assert bool((mag <= want_mag * (1 + 1e-12)).all())
        else:
            assert float((mag - want_mag).abs().max()) <= 1e-12 * float(want_mag.max())
        out_abs, C_abs, mag_abs = lref.hetero_sage_launch_ref(rels, N_ROWS, wt, N_W, root=(X["a"], DST_ROWS, None), bias=bias,
                                                              out_rows=OUT_ROWS, n_out=N_OUT, abs_terms=True)
        assert torch.equal(out_abs[OUT_ROWS], mag_abs[OUT_ROWS]) and torch.equal(mag_abs, mag) and bool((C_abs >= C.abs() - 1e-12).all())


def test_sage_launch_restatement_reads_node_lists_scales_and_the_running_sum():
    """ids, scale, acc_in and a root through dst_ids against the same launch over gathered, pre-scaled rows."""
    g = torch.Generator().manual_seed(23)
    ids = torch.randperm(60, generator=g)[:17].to(torch.int32)
    table = torch.full((60, 12), float("nan"))
    table[ids.long()] = X["b"]
    scale = torch.rand(17, generator=g) + 0.5
    dst_ids = torch.randperm(90, generator=g)[:30]
    table_a = torch.full((90, 8), float("nan"))
    table_a[dst_ids] = X["a"]
    wt = torch.randn((N_W, 20), generator=g)
    acc = torch.randn((N_ROWS, N_W), generator=g)
    got = lref.hetero_sage_launch_ref([HOP_B + (table, ids, scale, True)], N_ROWS, wt, N_W, root=(table_a, DST_ROWS, dst_ids), acc_in=acc)
    want = lref.hetero_sage_launch_ref([HOP_B + (X["b"].double() * scale.double().unsqueeze(1), None, None, True)], N_ROWS, wt, N_W,
                                       root=(X["a"], DST_ROWS, None))
    assert float((got[0] - (want[0] + acc)).abs().max()) <= 1e-12 and float((got[1] - want[1]).abs().max()) <= 1e-14
    assert float((got[2] - (want[2] + acc.abs())).abs().max()) <= 1e-12


def test_transformer_launch_restatement_matches_the_layer_restatement():
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(7)
    graph, n_in = hand_built(g)
    widths = {"a": 8, "b": 12}
    torch.manual_seed(4)
    for concat, C in ((True, [4, 4, 8]), (False, [6, 6, 6])):
        layer = make_layer(widths, [2, 2, 1], C, concat, [True, True, True], [3, None, 1]).double()
        xs = {t: torch.randn((n_in[t], widths[t]), generator=g, dtype=torch.float64) for t in n_in}
        ea = {et: v.double() for et, v in edge_attrs(graph, layer, g).items()}
        r0 = graph.relations[0]
        with torch.no_grad():
            wt, bias, fold, fold_b, layout = nn.hetero_transformer_stack([layer.conv(et) for et in ETS])
        uw = xs["a"][r0.dst_rows] @ fold + fold_b
        rels = []
        for r, lay in zip(graph.relations, layout):
            u = uw[:, lay["u0"]:lay["u0"] + lay["H"] * lay["F"]]
            w = uw[:, lay["w0"]:lay["w0"] + lay["H"] * lay["D"]] if lay["D"] else None
            rels.append((r.row_ptr, r.col, xs[r.edge_type[0]], None, ea.get(r.edge_type), u, w, lay["H"], None))
        p = href.params_of(layer)
        for relu in (False, True):
            out, A, mag, alphas = lref.hetero_transformer_launch_ref(rels, 10, wt, wt.shape[0], root=(xs["a"], r0.dst_rows, None),
                                                                     bias=bias, relu=relu, out_rows=r0.out_rows, n_out=10)
            want = href.hetero_transformer_forward(xs, graph, p, ea, relu=relu)["a"]
            assert float((out - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
        assert A.shape == (10, wt.shape[1]) and mag.shape == out.shape
        for r, lay, al in zip(graph.relations, layout, alphas):
            c = layer.conv(r.edge_type)
            _, ra = href.tref.transformer_forward(xs[r.edge_type[0]], xs["a"][r0.dst_rows], href.relation_coo(r), href.tref.params_of(c),
                                                  c.heads, concat=concat, edge_attr=ea.get(r.edge_type), return_alpha=True)
            assert al.shape == (r.n_edges, lay["H"]) and float((al - ra).abs().max()) <= 1e-12
            deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
            blk = A[:, lay["col0"]:lay["col0"] + lay["width"]]
            assert float(blk[deg == 0].abs().max()) == 0.0
            assert float((blk[deg > 0][:, lay["F"] + lay["D"]] - 1).abs().max()) <= 1e-12      # the "1" column: sum alpha


def test_case_table_builds_and_lists_every_value():
    """Every case builds on the CPU (``build_case`` asserts the piece count, a straddling row, a late-starting slot and, for P = 2,
    more than ``cap`` edges in rows 0..7 of a tile) and the table holds every value the launch-level test is to cover: every K of
    the width sweep with one and with several pieces."""
    built = [cases.build_case(c) for c in cases.CASES]
    assert len({b["name"] for b in built}) == len(built)
    sweep = {8: 16, 64: 16, 68: 8, 128: 8, 132: 4, 256: 4, 260: 2, 512: 2, 516: 1, 1024: 1}
    for K, P in sweep.items():
        assert cases.row_slots(K) == P
        assert {b["pieces"] for b in built if b["K"] == K and b["widths"]} == {"one", "many"}, K
    for pieces in ("one", "many"):
        assert any(b["widths"] == [112] * 8 and b["K"] == 1024 and b["pieces"] == pieces for b in built)
        assert any(b["widths"] == [1020] and b["K"] == 1024 and b["pieces"] == pieces for b in built)
        assert any(b["widths"] == [512] and b["root_form"] is None and b["pieces"] == pieces for b in built)
    assert {len(b["widths"]) for b in built} >= {0, 1, 3, 5, 8}
    assert {cases.stage_cap(n) for n in (1, 3, 5, 8)} == {768, 256, 144, 96}
    assert {b["n_rows"] for b in built} == {1, 15, 16, 17, 37}
    assert {b["N"] for b in built} == {1, 15, 16, 17, 47, 255, 256}
    assert {b["root_form"] for b in built} == {None, "direct", "rows", "ids32", "ids64"}
    flags = {f for b in built for f in b["flags"]}
    assert {"acc", "bias", "perm", "ldw", "ldc"} <= flags and any(f.startswith("empty") for f in flags)
    combos = {(o["ids"], o["mean"], o["scale"]) for b in built for o in b["opts"]}
    assert len(combos) == 12, combos
    # the options also rotate WITHIN one launch, and meet several pieces
    multi = [b for b in built if b["pieces"] == "many" and len(b["widths"]) >= 3]
    assert all(len({o["ids"] for o in b["opts"]}) == 3 and len({o["mean"] for o in b["opts"]}) == 2 for b in multi)
    assert {b["P"] for b in built if b["pieces"] == "many"} == {16, 8, 4, 2, 1}
    assert all(b["facts"]["pieces"] >= 4 for b in built if b["pieces"] == "many")       # (a 3000-edge row at cap <= 768)
    assert any(b["ldc"] > b["K"] for b in built) and any(b["wt"].stride(0) > b["K"] for b in built)


def test_integer_block_sums_stay_below_2_to_24():
    """A sum relation's x is integer-valued in [-8, 8] and its scale None or from {0.5, 1, 2}: every term is a multiple of 0.5, and
    with sum_e |term| < 2^23 every partial sum in any order is a multiple of 0.5 below 2^23 in magnitude — a float32.  (The bound
    is on the sum of magnitudes, in units of 0.5: below 2^24 halves.)"""
    seen = 0
    for c in cases.CASES:
        b = cases.build_case(c)
        _, C_abs, _ = lref.hetero_sage_launch_ref(b["rels"], b["n_rows"], b["wt"], b["N"], abs_terms=True, **b["kw"])
        at = 0
        for (row_ptr, col, x, ids, scale, mean), F in zip(b["rels"], b["widths"]):
            if not mean:
                live = x if ids is None else x[ids.long()]
                assert bool((live == live.round()).all()) and float(live.abs().max()) <= 8
                assert scale is None or set(scale.tolist()) <= {0.5, 1.0, 2.0}
                assert 2 * float(C_abs[:, at:at + F].max()) < 2 ** 24
                seen += 1
            at += F
    assert seen >= 30
