"""GPU: ``graph_ops.rows_first_unique`` (csrc/wg_rows_unique.hip) — the row-wise first-appearance de-duplication of a link call
group's seed-edge endpoints — against the torch formulation it replaces (``_batched_first_unique_torch``): all four outputs with
``torch.equal``, dtypes and zero tails included; the torch formulation itself against a plain Python first-appearance loop on
the small shapes; the dispatch of ``_batched_first_unique``; run-to-run equality; the domain's edge."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_S = 8192          # WGAMD_ROWS_FIRST_UNIQUE_MAX_S: one workgroup's LDS table (2 S slots of 8 bytes = 128 KiB)


def _python_first_unique(ends):
    G, S = ends.shape
    uniq, seg, batch, local = [], [0], [], []
    for g in range(G):
        seen, row = {}, []
        for v in ends[g].tolist():
            if v not in seen:
                seen[v] = len(seen)
                uniq.append(v)
                batch.append(g)
            row.append(seen[v])
        local.append(row)
        seg.append(len(uniq))
    pad = G * S - len(uniq)
    return uniq + [0] * pad, seg, batch + [0] * pad, local


def _rows(G, S, n_ids, seed):
    """[G, S] with the contents the kernel can get wrong: a row of one repeated id, an all-distinct row, id 0 first / last, a row
    whose second half repeats its first half (the src / dst halves of a joint list), ids that are multiples of 8192 and of the
    table's slot count (long probe chains), the value n_ids - 1; random draws from a small and from the whole range elsewhere."""
    rng = np.random.default_rng(seed)
    slots = max(64, 1 << int(np.ceil(np.log2(2 * S))))
    out = np.empty((G, S), dtype=np.int64)
    for g in range(G):
        kind = g % 8
        if kind == 0:
            row = np.full(S, min(7, n_ids - 1))
        elif kind == 1:
            row = (np.arange(S, dtype=np.int64) * 3 + 1) % n_ids if n_ids >= 3 * S + 1 else np.arange(S) % n_ids
        elif kind == 2:
            row = rng.integers(0, min(n_ids, max(2, S // 3)), S)
            row[0] = 0
        elif kind == 3:
            row = rng.integers(1, max(2, min(n_ids, S)), S)
            row[-1] = 0
        elif kind == 4:
            half = rng.integers(0, min(n_ids, 4 * S + 1), (S + 1) // 2)
            row = np.concatenate([half, half])[:S]
        elif kind == 5:
            row = (rng.integers(0, max(1, S // 2), S) * 8192) % n_ids
        elif kind == 6:
            row = (rng.integers(0, max(1, S // 2), S) * slots) % n_ids
        else:
            row = rng.integers(0, n_ids, S)
        row = np.asarray(row, dtype=np.int64)
        row[rng.integers(0, S)] = n_ids - 1
        out[g] = row
    return out


def _check(ends_np, n_ids, expect_kernel=True, python_loop=False):
    import torch
    from wholegraph_amd import graph_ops
    from cugraph_pyg_amd.loader.link_loader import _batched_first_unique, _batched_first_unique_torch
    ends = torch.from_numpy(ends_np).cuda()
    G, S = ends.shape
    assert graph_ops.rows_first_unique_supported(G, S, n_ids) == expect_kernel
    want = _batched_first_unique_torch(ends, n_ids)
    got = _batched_first_unique(ends, n_ids)
    again = graph_ops.rows_first_unique(ends, n_ids) if expect_kernel else got
    for name, w, g, a in zip(("uniq", "seg", "batch", "local"), want, got, again):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g, w), name
        assert torch.equal(a, g), name + " (second run)"
    assert want[0].dtype == torch.int64 and want[1].dtype == torch.int32 and want[2].dtype == torch.int32 and want[3].dtype == torch.int64
    live = int(want[1][-1])
    assert not got[0][live:].any() and not got[2][live:].any()
    if python_loop:
        uniq, seg, batch, local = _python_first_unique(ends_np)
        assert want[0].tolist() == uniq and want[1].tolist() == seg and want[2].tolist() == batch and want[3].tolist() == local


@pytest.mark.parametrize("G,S", [(1, 1), (9, 63), (9, 64), (9, 65), (9, 257), (3, 512), (3, 513), (3, 4096), (8, 4096), (2, MAX_S),
                                 (4097, 4)])
def test_rows_first_unique_equals_the_torch_formulation(hiplib, G, S):
    _check(_rows(G, S, 100003, 11 * G + S), 100003, python_loop=G * S <= 9 * 257)


@pytest.mark.parametrize("n_ids", [5, 2 ** 31, 2 ** 32 + 5, 2 ** 40])
def test_rows_first_unique_id_ranges(hiplib, n_ids):
    _check(_rows(8, 130, n_ids, 3), n_ids, python_loop=True)
    _check(_rows(8, 1500, n_ids, 4), n_ids)


def test_rows_first_unique_outside_the_domain_takes_the_torch_route(hiplib):
    import torch
    from wholegraph_amd import graph_ops
    _check(_rows(2, MAX_S + 1, 100003, 5), 100003, expect_kernel=False)
    _check(_rows(3, 40, 2 ** 40 + 1, 6), 2 ** 40 + 1, expect_kernel=False)
    assert not graph_ops.rows_first_unique_supported(2 ** 20, 2 ** 11, 10)          # G S = 2^31
    assert graph_ops.rows_first_unique_supported(2 ** 20 - 1, 2 ** 11, 10)
    with pytest.raises(ValueError, match="domain"):
        graph_ops.rows_first_unique(torch.zeros((2, MAX_S + 1), dtype=torch.int64, device="cuda"), 10)
