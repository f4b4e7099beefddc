"""``nn.hetero_sage_launch`` (``hetero_sage_kernel``, csrc/wg_sage_hetero.hip) pinned at launch level: every thread-to-work map
(P = 16, 8, 4, 2, 1 row slots), every staging capacity (n_rel = 1, 3, 5, 8), one and several pieces, rows that straddle a piece
boundary, slots whose first edge lies in a later piece, every node-list kind, mean / sum, with and without ``src_scale``, an edgeless
relation, every root form, ``acc_in`` + ReLU, ``out_rows``, ``ldw > K``, ``ldc > K`` — against the float64 restatement of
tests/hetero_launch_ref.py.  Bars:
  (a) ``out`` within 1e-5 x the magnitude sum of its terms, element by element (``check_forward`` of test_gpu_hetero_sage.py);
  (b) the kept C block of a sum relation (integer x in [-8, 8], scale None or from {0.5, 1, 2}: every partial sum is exact in fp32
      whatever the order — tests/test_hetero_launch_ref_host.py checks the 2^24 bound) and the root block: ``torch.equal``;
  (c) the kept C block of a mean relation (arbitrary floats): within 1e-6 x the sum of |terms| (a test of its own);
  (d) the ``_train`` form gives the inference form's bits, two runs give the same bits;
  (e) output rows ``out_rows`` does not name keep a sentinel (and so do the columns of ``c_out`` past K);
  (f) every launch advances ``nn.hetero_sage_launches`` by exactly 1.
The cases are the explicit table ``CASES``; ``build_case`` works on the CPU too (the host test builds every case); every case
is launched once per session (``launched``) and shared by the tests that read it."""
import pytest

from hetero_launch_ref import edge_case_hop, hetero_sage_launch_ref

K_STAGE = 768      # kStage of csrc/wg_sage_hetero.hip: edges staged per piece, all relations together
K_UNROLL = 16      # kUnroll there: the staging capacity per relation is a multiple of it
TILE_ROWS, THREADS = 16, 256
SENTINEL = -123.0


def stage_cap(n_rel):
    """``cap`` of hetero_sage_kernel: the edges of ONE relation staged per piece — (kStage / n_rel) & ~15."""
    return (K_STAGE // n_rel) & ~(K_UNROLL - 1) if n_rel > 0 else K_STAGE


def row_slots(K):
    """``P`` of the launch: the largest power of two <= 16 with P (K / 4) <= 256 threads."""
    P = 1
    while P < TILE_ROWS and 2 * P * (K // 4) <= THREADS:
        P *= 2
    return P


def degree_pattern(cap, pieces):
    """16 degrees, repeated along the rows.  ``many``: unroll remainders (15, 16, 17, 31, 32, 33), the piece capacity and its
    neighbours, a row of more than two pieces, a 3000-edge row.  ``one``: at most 72 edges per tile (one piece at any cap >= 80)."""
    if pieces == "many":
        return [0, 1, 15, 16, 17, 31, 32, 33, cap - 1, cap, cap + 1, 2 * cap + 5, 0, 0, 3000, 1]
    return [0, 1, 15, 16, 17, 0, 2, 3, 1, 0, 4, 5, 0, 0, 7, 1]


# Per-relation options rotate with k = relation index + ``rot``: ids None / int32 / int64 by k % 3, mean for odd k, src_scale for
# k // 2 odd — twelve combinations in twelve steps.  Degrees of relation r, row i: pattern[(i + deg0 + 2 r) % 16], so that heavy
# rows of one relation meet empty rows of the others.
# (name, relation widths, F_dst, root form, n_rows, N, pieces, deg0, rot, flags)
#   root form: None | "direct" (x_dst[i]) | "rows" (dst_rows) | "ids32" / "ids64" (dst_rows, then a node list)
#   flags: acc (acc_in + bias + ReLU), bias, perm (out_rows: a permutation into a larger output), ldw, ldc, empty<r> (relation r
#   has no edge in the whole launch)
CASES = [
    # K = 8, P = 16: one relation of one chunk and a root of one chunk
    ("K8-one", [4], 4, "rows", 17, 1, "one", 1, 0, "bias"),
    ("K8-many", [4], 4, "ids32", 17, 15, "many", 0, 2, "perm ldc"),
    # K = 64, P = 16
    ("K64-one", [16] * 3, 16, "ids64", 16, 16, "one", 0, 0, "acc"),
    ("K64-many", [16] * 3, 16, "rows", 37, 17, "many", 0, 1, "bias perm"),
    # K = 68, P = 8 (Q = 17: 120 idle threads)
    ("K68-one", [16] * 4, 4, "direct", 15, 47, "one", 3, 2, "ldw"),
    ("K68-many", [16] * 4, 4, "ids32", 16, 47, "many", 0, 3, "acc ldc"),
    # K = 128, P = 8
    ("K128-one", [32] * 3, 32, "rows", 37, 255, "one", 0, 4, "bias ldw ldc"),
    ("K128-many", [32] * 3, 32, "ids64", 17, 256, "many", 5, 5, "perm empty1"),
    # K = 132, P = 4 (Q = 33)
    ("K132-one", [64, 32, 32], 4, "rows", 16, 16, "one", 0, 6, "empty0"),
    ("K132-many", [128], 4, "direct", 15, 17, "many", 8, 0, "acc"),
    # K = 256, P = 4
    ("K256-one", [48] * 5, 16, "ids32", 17, 47, "one", 2, 1, "perm"),
    ("K256-many", [48] * 5, 16, "rows", 37, 15, "many", 0, 0, "bias ldw"),
    # K = 260, P = 2 (Q = 65)
    ("K260-one", [256], 4, "rows", 15, 256, "one", 0, 2, "bias"),
    ("K260-many", [48] * 5, 20, "ids64", 17, 16, "many", 0, 7, "acc perm empty4"),
    # K = 512, P = 2
    ("K512-one", [48] * 8, 128, "rows", 16, 255, "one", 0, 3, "ldc"),
    ("K512-many", [48] * 8, 128, "ids32", 37, 17, "many", 0, 0, "bias perm ldw empty6"),
    # K = 516, P = 1: a single relation wider than 256 floats
    ("K516-one", [512], 4, "direct", 1, 1, "one", 2, 0, "bias"),
    ("K516-many", [512], 4, "rows", 1, 15, "many", 14, 4, "acc"),
    # K = 1024, P = 1: eight relations
    ("K1024x8-one", [112] * 8, 128, "ids64", 15, 47, "one", 0, 5, "bias"),
    ("K1024x8-many", [112] * 8, 128, "rows", 17, 256, "many", 0, 6, "acc ldw ldc"),
    # K = 1024: one relation of 1020 floats
    ("K1024x1-one", [1020], 4, "rows", 17, 16, "one", 0, 6, "perm"),
    ("K1024x1-many", [1020], 4, "ids32", 16, 17, "many", 8, 2, "bias"),
    # K = 512 without a root, P = 2: rows 0..7 of the single relation hold more than cap = 768 edges
    ("K512noroot-one", [512], 0, None, 16, 47, "one", 0, 4, "bias"),
    ("K512noroot-many", [512], 0, None, 15, 255, "many", 8, 3, "acc"),
    # the root alone (n_rel = 0)
    ("root-only", [], 64, "ids64", 37, 17, "one", 0, 0, "bias perm ldc"),
]


def relation_options(r, rot):
    k = r + rot
    return dict(ids=[None, "int32", "int64"][k % 3], mean=k % 2 == 1, scale=(k // 2) % 2 == 1)


def piece_facts(row_ptrs, n_rows, cap, P):
    """What the kernel's walk meets in these CSRs: ``pieces`` (the largest piece count of a tile), ``straddle`` (a row whose edges
    lie on both sides of a piece boundary), ``late_slot`` (a row slot with rows whose first edge lies past the tile's first piece)
    and ``first_half`` (rows 0..7 of a tile hold more than ``cap`` edges of a relation)."""
    rps = TILE_ROWS // P
    facts = dict(pieces=0, straddle=False, late_slot=False, first_half=False)
    for rp in row_ptrs:
        rp = [int(v) for v in rp]
        for row0 in range(0, n_rows, TILE_ROWS):
            here = min(TILE_ROWS, n_rows - row0)
            base = rp[row0]
            facts["pieces"] = max(facts["pieces"], -(-(rp[row0 + here] - base) // cap))
            for lr in range(here):
                s, t = rp[row0 + lr] - base, rp[row0 + lr + 1] - base
                if any(s < b < t for b in range(cap, t, cap)):
                    facts["straddle"] = True
                slot_end = rp[row0 + min(lr + rps, here)] - base
                if lr % rps == 0 and lr > 0 and slot_end > s >= cap:
                    facts["late_slot"] = True
            if here > 8 and rp[row0 + 8] - base > cap:
                facts["first_half"] = True
    return facts


def build_case(case, dev="cpu"):
    """The tensors of one case on ``dev`` (drawn on the CPU: the same numbers everywhere) -> dict(rels, kw, exact, ...).
    Asserts the host-side facts the case is there for: the piece count, a straddling row and a late-starting slot."""
    import torch
    name, widths, F_dst, root_form, n_rows, N, pieces, deg0, rot, flags = case
    flags = flags.split()
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    n_rel = len(widths)
    K = sum(widths) + F_dst
    cap, P = stage_cap(n_rel), row_slots(K)
    pattern = degree_pattern(cap, pieces)
    ints = lambda shape: torch.randint(-8, 9, shape, generator=g).float()      # noqa: E731
    rels, opts, row_ptrs = [], [], []
    for r, F in enumerate(widths):
        o = relation_options(r, rot)
        n_src = 40 + 7 * r
        deg = [0 if "empty%d" % r in flags else pattern[(i + deg0 + 2 * r) % 16] for i in range(n_rows)]
        row_ptr, col = edge_case_hop(n_rows, n_src, deg, seed=100 * r + n_rows)
        x = torch.randn((n_src, F), generator=g) if o["mean"] else ints((n_src, F))
        ids = None
        if o["ids"] is not None:      # x is a table of 3 n_src rows read through a node list
            ids = torch.randperm(3 * n_src, generator=g)[:n_src].to(getattr(torch, o["ids"]))
            table = torch.full((3 * n_src, F), float("nan"))
            table[ids.long()] = x
            x = table
        scale = None
        if o["scale"]:
            scale = (torch.rand(n_src, generator=g) + 0.5) if o["mean"] else \
                torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n_src,), generator=g)]
        rels.append(tuple(None if t is None else t.to(dev) for t in (row_ptr, col, x, ids, scale)) + (o["mean"],))
        opts.append(o)
        row_ptrs.append(row_ptr.tolist())
    facts = piece_facts(row_ptrs, n_rows, cap, P)
    if pieces == "one":
        assert facts["pieces"] <= 1, (name, facts)
    elif n_rel > 0:
        assert facts["pieces"] > 1 and facts["straddle"], (name, facts)
        assert P == 1 or facts["late_slot"], (name, P, facts)
        assert P != 2 or facts["first_half"], (name, facts)
    root = None
    if root_form is not None:
        n_dst = n_rows + 9
        x_dst = ints((n_dst, F_dst))
        dst_rows = dst_ids = None
        if root_form != "direct":
            dst_rows = torch.randperm(n_dst, generator=g)[:n_rows].contiguous()
        if root_form in ("ids32", "ids64"):
            dst_ids = torch.randperm(2 * n_dst, generator=g)[:n_dst].to(torch.int32 if root_form == "ids32" else torch.int64)
            table = torch.full((2 * n_dst, F_dst), float("nan"))
            table[dst_ids.long()] = x_dst
            x_dst = table
        root = tuple(None if t is None else t.to(dev) for t in (x_dst, dst_rows, dst_ids))
    ldw = K + 12 if "ldw" in flags else K
    wt = (torch.randn((N, ldw), generator=g) * 0.2).to(dev)[:, ldw - K:]          # (a column slice: 12 floats = 48 B in)
    acc = "acc" in flags
    kw = dict(root=root, relu=acc)
    kw["bias"] = torch.randn(N, generator=g).to(dev) if acc or "bias" in flags else None
    kw["acc_in"] = torch.randn((n_rows, N), generator=g).to(dev) if acc else None
    n_out = n_rows
    kw["out_rows"] = None
    if "perm" in flags:
        n_out = n_rows + 11
        kw["out_rows"] = torch.randperm(n_out, generator=g)[:n_rows].contiguous().to(dev)
    return dict(name=name, rels=rels, n_rows=n_rows, wt=wt, N=N, kw=kw, n_out=n_out, K=K, P=P, cap=cap, widths=widths, opts=opts,
                facts=facts, ldc=K + 8 if "ldc" in flags else K, flags=flags, root_form=root_form, pieces=pieces)


def run_launch(b, train, dev):
    """One launch of case ``b`` -> (out [n_out, N] pre-filled with the sentinel, c_out buffer or None)."""
    import torch
    from wholegraph_amd import nn
    out = torch.full((b["n_out"], b["N"]), SENTINEL, device=dev)
    c = torch.full((b["n_rows"], b["ldc"]), SENTINEL, device=dev) if train else None
    before = nn.hetero_sage_launches
    got = nn.hetero_sage_launch(b["rels"], b["n_rows"], b["wt"], b["N"], out=out, c_out=c, **b["kw"])
    assert nn.hetero_sage_launches - before == 1, "(f) one launch"
    assert got is out
    return out, c


_RESULTS = {}


def launched(case):
    """Case ``case`` built, launched (inference form, ``_train`` form twice: (d), (f)) and restated in float64, once per session."""
    import torch
    name = case[0]
    if name not in _RESULTS:
        dev = torch.device("cuda", 0)
        b = build_case(case, dev)
        out, _ = run_launch(b, False, dev)
        out_t, c = run_launch(b, True, dev)
        out_2, c_2 = run_launch(b, True, dev)
        assert torch.equal(out, out_t), name + ": (d) the _train form's out differs from the inference form's"
        assert torch.equal(out_t, out_2) and torch.equal(c, c_2), name + ": (d) two runs differ"
        ref, C, mag = hetero_sage_launch_ref(b["rels"], b["n_rows"], b["wt"], b["N"], n_out=b["n_out"], **b["kw"])
        _, C_abs, _ = hetero_sage_launch_ref(b["rels"], b["n_rows"], b["wt"], b["N"], n_out=b["n_out"], abs_terms=True, **b["kw"])
        _RESULTS[name] = dict(b, out=out, c=c, ref=ref, C=C, mag=mag, C_abs=C_abs)
    return _RESULTS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launch_matches_float64_and_exact_integer_sums(hiplib, case):
    """(a), (b), (d), (e), (f) of the module docstring."""
    import torch
    b = launched(case)
    name, kw, K, out, c = b["name"], b["kw"], b["K"], b["out"], b["c"]
    named = torch.zeros(b["n_out"], dtype=torch.bool, device=out.device)
    named[kw["out_rows"] if kw["out_rows"] is not None else slice(None)] = True
    # (e) rows out_rows does not name, and c_out's columns past K
    assert bool((out[~named] == SENTINEL).all()), name + ": (e) a row out_rows does not name was written"
    assert int((~named).sum()) == b["n_out"] - b["n_rows"]
    assert bool((c[:, K:] == SENTINEL).all()), name + ": (e) c_out was written past K"
    # (a) out
    err = (out[named].double() - b["ref"][named]).abs()
    mag = b["mag"][named]
    worst = float((err / mag.clamp(min=1e-30)).max())
    print("%s (K %d, P %d, cap %d, %d pieces): out max |err| %.3e, worst err / magnitude sum %.3e"
          % (name, K, b["P"], b["cap"], b["facts"]["pieces"], float(err.max()), worst))
    assert bool(torch.isfinite(out[named]).all()) and bool((err <= 1e-5 * mag).all()), (name, "(a)", worst)
    # (b) the kept C blocks of the sum relations and the root block: equal
    at = 0
    for r, (F, o) in enumerate(zip(b["widths"], b["opts"])):
        if not o["mean"]:
            bad = (c[:, at:at + F] != b["C"][:, at:at + F].float()).nonzero()
            assert bad.numel() == 0, "%s: (b) relation %d (ids %s, scale %s): %d elements of C differ, the first at row %d, chunk %d" % (
                name, r, o["ids"], o["scale"], bad.shape[0], int(bad[0, 0]), int(bad[0, 1]) // 4)
        at += F
    if kw["root"] is not None:
        assert torch.equal(c[:, at:K], b["C"][:, at:].float()), name + ": (b) the root block of C"


MEAN_CASES = [c for c in CASES if any(relation_options(r, c[8])["mean"] for r in range(len(c[1])))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MEAN_CASES, ids=[c[0] for c in MEAN_CASES])
def test_mean_blocks_of_kept_rows_within_1e_6_of_float64(hiplib, case):
    """(c): the kept C block of every mean relation (arbitrary floats) within 1e-6 x the sum of |terms| of float64, rows of 3000
    edges included: the walk's sums are compensated (Kahan).  A plain float32 sum in CSR order misses the bar from some 700
    edges on (3.5e-6 at 3000 edges drawn from 40 source rows)."""
    b = launched(case)
    at, worst_of = 0, []
    for r, (F, o) in enumerate(zip(b["widths"], b["opts"])):
        if o["mean"]:
            e = (b["c"][:, at:at + F].double() - b["C"][:, at:at + F]).abs()
            scale = b["C_abs"][:, at:at + F]
            w = float((e / scale.clamp(min=1e-30)).max())
            print("%s relation %d (mean, ids %s, scale %s): C worst err / sum |terms| %.3e" % (b["name"], r, o["ids"], o["scale"], w))
            worst_of.append((r, w, bool((e <= 1e-6 * scale).all())))
        at += F
    assert worst_of and all(ok for _, _, ok in worst_of), (b["name"], "(c)", worst_of)


@pytest.mark.gpu
def test_gradient_form_two_launches_with_running_sum(hiplib):
    """The launches of ``_HeteroSageGroup.backward`` for one source type: no root, x = dZ (arbitrary floats, F = 256), a sum
    relation with scale = 1 / deg of the transposed entry (floats that are no powers of two), N = 256, rows of 3000 edges; the
    second launch adds the first one's ``gx`` through ``acc_in``.  Bar (a)."""
    import torch
    from wholegraph_amd import nn
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(77)
    n_src, n_dst, F, N = 17, 90, 256, 256
    gz = torch.randn((n_dst, F), generator=g).to(dev)
    rels = []
    for r in range(3):
        cap = stage_cap(2 if r < 2 else 1)
        pattern = degree_pattern(cap, "many")
        row_ptr, col = edge_case_hop(n_src, n_dst, [pattern[(i + 14 + 2 * r) % 16] for i in range(n_src)], seed=r)
        scale = 1.0 / torch.randint(1, 41, (n_dst,), generator=g).float()
        rels.append((row_ptr.to(dev), col.to(dev), gz, None, scale.to(dev) if r != 1 else None, False))
    wt = (torch.randn((N, 3 * F), generator=g) * 0.1).to(dev)
    gx = None
    for lo, hi in ((0, 2), (2, 3)):
        w = wt[:, lo * F:hi * F].contiguous()
        before = nn.hetero_sage_launches
        got = nn.hetero_sage_launch(rels[lo:hi], n_src, w, N, acc_in=gx)
        again = nn.hetero_sage_launch(rels[lo:hi], n_src, w, N, acc_in=gx)
        assert nn.hetero_sage_launches - before == 2 and torch.equal(got, again)
        ref, _, mag = hetero_sage_launch_ref(rels[lo:hi], n_src, w, N, acc_in=gx)
        err = (got.double() - ref).abs()
        worst = float((err / mag.clamp(min=1e-30)).max())
        print("gradient form, relations [%d, %d): max |err| %.3e, worst err / magnitude sum %.3e" % (lo, hi, float(err.max()), worst))
        assert bool(torch.isfinite(got).all()) and bool((err <= 1e-5 * mag).all()), worst
        gx = got


def _supported(widths, F_dst, N):
    import ctypes
    from wholegraph_amd import _lib as L
    return bool(L.lib().wgamd_hetero_sage_layer_supported((ctypes.c_int * max(len(widths), 1))(*widths), len(widths), F_dst, N))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["K=1028", "nine relations", "F=30", "N=257", "col0", "row stride"])
def test_refusals_launch_nothing(hiplib, monkeypatch, what):
    """Host checks only: each returns an error through ``L.check`` before any launch, the pre-filled ``out`` keeps its sentinel,
    and ``wgamd_hetero_sage_layer_supported`` — a predicate of the widths alone — says no to the four shapes and yes to the
    shapes of the two launches that are refused for their operands' layout (``col0``, the row stride)."""
    import torch
    from wholegraph_amd import _lib as L, nn
    dev = torch.device("cuda", 0)
    n_rows, n_src, N = 5, 12, 16
    widths, F_dst = {"K=1028": ([512, 512], 4), "nine relations": ([8] * 9, 8), "F=30": ([30], 0), "N=257": ([8], 8),
                     "col0": ([8, 8], 8), "row stride": ([8], 8)}[what]
    if what == "N=257":
        N = 257
    assert _supported(widths, F_dst, N) == (what in ("col0", "row stride"))
    row_ptr, col = edge_case_hop(n_rows, n_src, [2, 0, 3, 1, 4], seed=1)
    row_ptr, col = row_ptr.to(dev), col.to(dev)
    rels = []
    for F in widths:
        x = torch.ones((n_src, F + 2), device=dev)[:, :F] if what == "row stride" else torch.ones((n_src, F), device=dev)
        rels.append((row_ptr, col, x, None, None, False))
    if what == "col0":
        tail = nn._hetero_launch_tail

        def shifted(name, relu_flag, arr, *rest):
            arr[1].col0 += 4          # a gap between the two relation blocks
            return tail(name, relu_flag, arr, *rest)
        monkeypatch.setattr(nn, "_hetero_launch_tail", shifted)
    root = (torch.ones((n_rows, F_dst), device=dev), None, None) if F_dst else None
    wt = torch.ones((N, sum(widths) + F_dst + 4), device=dev)
    out = torch.full((n_rows, N), SENTINEL, device=dev)
    before = nn.hetero_sage_launches
    with pytest.raises(L.WholeMemoryError):
        nn.hetero_sage_launch(rels, n_rows, wt, N, root=root, out=out)
    torch.cuda.synchronize()
    assert nn.hetero_sage_launches == before and bool((out == SENTINEL).all())
