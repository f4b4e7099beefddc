"""GPU: ``wgamd_unique_bounded`` / ``wgamd_unique_bounded_live`` on the path that keeps its marks as bits in LDS
(csrc/wg_unique.hip: one workgroup per (range of 2^20 ids, slice of the list), slabs OR-ed word by word, scan and compaction
in one launch) — at the smallest shapes where that path can go wrong: bounds around a range edge, lists shorter and longer
than one slice, hubs, ids at a range's first and last bit, negative and out-of-bound ids, a live count below the capacity,
replay on one workspace block.  Every output is an integer array compared for equality with ``numpy.unique``.

Which path a shape takes is a rule over (n, bound) alone (header of wg_unique.hip).  Its observable is the workspace plan: a
bound the LDS path takes plans the slabs (up to 256 x 128 KB) on top of the byte path's ~1.4 bytes per possible id."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANGE = 1 << 20
LDS_BOUNDS = [37, RANGE - 1, RANGE, RANGE + 1, 3 * RANGE - 31, 3 * RANGE + 5]
DTYPES = ["int64", "int32"]


def plans_slabs(lib, bound):
    """The byte path needs bound (marks) + bound / 4 ({bits, prefix}) + bound / 8 (counts) bytes and some KB of padding."""
    return lib.wgamd_unique_bounded_workspace_bytes(bound) > 2 * bound + (64 << 10)


def reference(ids, bound):
    """(distinct ascending, inverse with -1 for ids outside [0, bound), any id >= bound)"""
    ok = (ids >= 0) & (ids < bound)
    distinct, inv = np.unique(ids[ok], return_inverse=True)
    inverse = np.full(ids.shape[0], -1, np.int32)
    inverse[ok] = inv.astype(np.int32)
    return distinct.astype(np.int64), inverse, bool((ids >= bound).any())


def check(ids, bound, dtype):
    import torch
    from wholegraph_amd.tensor import unique_bounded
    want_d, want_i, want_bad = reference(ids, bound)
    d, inv, bad = unique_bounded(torch.from_numpy(ids.astype(dtype)).cuda(), bound, report_out_of_bound=True)
    assert bad == want_bad
    assert np.array_equal(d.cpu().numpy(), want_d)
    assert np.array_equal(inv.cpu().numpy(), want_i)


def edge_ids(bound):
    """first and last id, and the first and last bit of every range and of a word inside it"""
    e = [0, bound - 1]
    for r in range((bound + RANGE - 1) // RANGE):
        e += [r * RANGE, r * RANGE + 31, r * RANGE + 32, (r + 1) * RANGE - 1]
    return np.array([v for v in e if 0 <= v < bound], np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bound", LDS_BOUNDS)
def test_bounds_around_a_range_edge_short_lists(hiplib, bound, dtype):
    assert plans_slabs(hiplib, bound)
    rng = np.random.default_rng(bound)
    for n in (0, 1, 255, 257):
        ids = rng.integers(0, bound, n)
        ids[:min(n, 16)] = rng.choice(edge_ids(bound), min(n, 16))
        ids[3::50] = -1
        check(ids, bound, dtype)
    check(np.array([bound - 1]), bound, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bound", LDS_BOUNDS)
def test_bounds_around_a_range_edge_two_million_ids(hiplib, bound, dtype):
    """every slice of a full launch holds ids of every range; the edge ids sit in the first and in the last slice"""
    rng = np.random.default_rng(bound + 1)
    n = 2_000_003
    ids = np.minimum(rng.integers(0, bound, n), rng.integers(0, bound, n))      # skewed: repeats, and gaps near the top
    e = edge_ids(bound)
    ids[:e.size] = e
    ids[n - e.size:] = e[::-1]
    ids[7::1001] = -1
    check(ids, bound, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_hub_in_every_position_of_every_slice(hiplib, dtype):
    """one id in every position: every lane of every wave of every slice ORs one bit, every slab carries it"""
    bound, hub = 3 * RANGE + 5, 2 * RANGE + 77
    ids = np.full(300_000, hub, np.int64)
    check(ids, bound, dtype)
    ids[::8192] = np.arange(ids[::8192].size) * 3      # and one other id per slice-sized stretch
    ids[-1] = bound - 1
    check(ids, bound, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_only_in_the_last_range_and_only_at_range_edges(hiplib, dtype):
    bound = 3 * RANGE + 5                                # the last range holds five ids
    rng = np.random.default_rng(5)
    check(rng.integers(3 * RANGE, bound, 100_000), bound, dtype)
    bound = 3 * RANGE - 31
    check(rng.integers(2 * RANGE, bound, 100_000), bound, dtype)
    e = np.array([r * RANGE + o for r in range(3) for o in (0, RANGE - 1) if r * RANGE + o < bound], np.int64)
    check(rng.choice(e, 50_000), bound, dtype)
    check(e, bound, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [300, 400_000])
def test_negative_and_out_of_bound_ids(hiplib, n, dtype):
    import torch
    from wholegraph_amd.tensor import unique_bounded
    bound = RANGE + 1
    rng = np.random.default_rng(n)
    ids = rng.integers(0, bound, n)
    ids[1::7] = -rng.integers(1, 1 << 30, ids[1::7].size)
    check(ids, bound, dtype)                             # negatives alone: no flag
    ids[n // 2] = bound                                  # one id just out of bound, in one slice only
    ids[5] = (1 << 31) - 1
    check(ids, bound, dtype)
    with pytest.raises(IndexError):
        unique_bounded(torch.from_numpy(ids.astype(dtype)).cuda(), bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cap,live", [(40_000, 23_456), (40_000, 0), (1_000_000, 333_333), (1_000_000, 1)])
def test_live_count_below_the_capacity(hiplib, cap, live, dtype):
    """garbage past the live count — ids >= bound among it — is never looked at and does not set the flag"""
    import torch
    from wholegraph_amd.tensor import unique_bounded_nosync
    bound = 3 * RANGE - 31
    rng = np.random.default_rng(cap + live)
    ids = rng.integers(0, bound, cap)
    ids[:live:97] = -1
    ids[live:] = rng.integers(bound, (1 << 31) - 1, cap - live)
    ids[live::3] = rng.integers(0, bound, ids[live::3].size)
    want_d, want_i, want_bad = reference(ids[:live], bound)
    assert not want_bad
    n_live = torch.tensor([live], dtype=torch.int32, device="cuda")
    distinct, inverse, info = unique_bounded_nosync(torch.from_numpy(ids.astype(dtype)).cuda(), n_live, bound)
    n_d, bad = info.tolist()
    assert bad == 0 and n_d == want_d.shape[0]
    assert np.array_equal(distinct[:n_d].cpu().numpy(), want_d)
    assert np.array_equal(inverse[:live].cpu().numpy(), want_i)


def run_on_workspace(lib, ids, bound, ws, nbytes):
    """one direct call on the caller's workspace block, on torch's current stream -> (distinct, inverse, bad), device side"""
    import torch
    from wholegraph_amd import _lib as L
    from wholegraph_amd.env import get_stream, torch_dtype_to_wm
    n = ids.shape[0]
    distinct = torch.empty(min(n, bound), dtype=torch.int64, device="cuda")
    inverse = torch.empty(n, dtype=torch.int32, device="cuda")
    info = torch.empty(2, dtype=torch.int32, device="cuda")
    L.check(lib.wgamd_unique_bounded(ids.data_ptr(), torch_dtype_to_wm(ids.dtype), n, bound, distinct.data_ptr(), inverse.data_ptr(),
                                     info.data_ptr(), info.data_ptr() + 4, ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes, get_stream()),
            "wgamd_unique_bounded")
    return distinct, inverse, info


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_on_one_workspace_block_and_on_two_streams(hiplib, dtype):
    """a dense list with an out-of-bound id, then a sparse one, back to back on ONE workspace: no mark, slab word, count or
    flag of the first call may show in the second; then the same pair on two other streams"""
    import torch
    bound = 3 * RANGE + 5
    nbytes = hiplib.wgamd_unique_bounded_workspace_bytes(bound)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(11)
    dense = rng.integers(0, bound, 1_500_000)
    dense[12345] = bound + 3
    sparse = rng.integers(0, bound, 3000)
    sparse[::11] = -1
    lists = [dense, sparse, dense]
    dev = [torch.from_numpy(a.astype(dtype)).cuda() for a in lists]
    want = [reference(a, bound) for a in lists]

    def verify(got):
        for (d, inv, info), (want_d, want_i, want_bad) in zip(got, want):
            n_d, bad = info.tolist()
            assert bool(bad) == want_bad and n_d == want_d.shape[0]
            assert np.array_equal(d[:n_d].cpu().numpy(), want_d)
            assert np.array_equal(inv.cpu().numpy(), want_i)

    verify([run_on_workspace(hiplib, a, bound, ws, nbytes) for a in dev])
    torch.cuda.synchronize()
    got = []
    for k, a in enumerate(dev):                          # one workspace block per stream: the calls may overlap
        s = torch.cuda.Stream()
        block = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(s):
            got.append(run_on_workspace(hiplib, a, bound, block, nbytes) + (block, s))
    torch.cuda.synchronize()
    verify([g[:3] for g in got])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_large_bound_stays_on_byte_marks_and_still_matches(hiplib, dtype):
    bound = 1 << 26
    assert not plans_slabs(hiplib, bound)
    rng = np.random.default_rng(26)
    ids = rng.integers(0, bound, 100_000)
    ids[::13] = -1
    ids[:4] = [0, bound - 1, RANGE, RANGE - 1]
    check(ids, bound, dtype)
