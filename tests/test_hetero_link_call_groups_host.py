"""Host: ``hetero_link_group_index`` (cugraph_pyg_amd/loader/link_call_group.py) — the ``edge_label_index`` / ``label_ptr`` of a
heterogeneous link call group from the per-batch local positions and the per-type batch offsets — against a per-batch loop."""
import pytest
import torch

from cugraph_pyg_amd.loader.link_call_group import hetero_link_group_index, link_group_index


def _case(G, n_pos, n_neg, one_type, seed):
    """Per batch: unique-list sizes per type, local positions of the sources / destinations inside them."""
    g = torch.Generator().manual_seed(seed)
    half = n_pos + n_neg
    if one_type:
        sizes = torch.randint(1, 2 * half + 1, (G,), generator=g)
        size_src = size_dst = sizes
    else:
        size_src = torch.randint(1, half + 1, (G,), generator=g)
        size_dst = torch.randint(1, half + 1, (G,), generator=g)
    local_src = torch.stack([torch.randint(0, int(size_src[b]), (half,), generator=g) for b in range(G)])
    local_dst = torch.stack([torch.randint(0, int(size_dst[b]), (half,), generator=g) for b in range(G)])
    ptr_src = torch.zeros(G + 1, dtype=torch.int32)
    ptr_src[1:] = torch.cumsum(size_src, 0)
    ptr_dst = ptr_src if one_type else torch.zeros(G + 1, dtype=torch.int32)
    if not one_type:
        ptr_dst[1:] = torch.cumsum(size_dst, 0)
    return local_src, local_dst, ptr_src, ptr_dst


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("one_type", [False, True], ids=["two-types", "one-type"])
@pytest.mark.parametrize("n_pos,n_neg", [(5, 0), (5, 5), (7, 2), (4, 8)])
def test_hetero_link_group_index_equals_the_per_batch_loop(G, one_type, n_pos, n_neg):
    local_src, local_dst, ptr_src, ptr_dst = _case(G, n_pos, n_neg, one_type, 10 * G + n_neg)
    index, label_ptr = hetero_link_group_index(local_src, local_dst, ptr_src, ptr_dst, n_pos, n_neg)
    half = n_pos + n_neg
    rows = [[], []]
    for b in range(G):
        for p in range(half):          # positives first inside a batch, batch-major
            rows[0].append(int(local_src[b, p]) + int(ptr_src[b]))
            rows[1].append(int(local_dst[b, p]) + int(ptr_dst[b]))
    assert index.dtype == torch.int64 and index.shape == (2, G * half) and index.tolist() == rows
    assert label_ptr.dtype == torch.int64 and label_ptr.tolist() == [b * half for b in range(G + 1)]
    assert int(index[0].max()) < int(ptr_src[-1]) and int(index[1].max()) < int(ptr_dst[-1])
    if one_type:        # one joint list: the homogeneous helper over [sources | destinations]
        both, ptr = link_group_index(torch.cat([local_src, local_dst], 1), ptr_src, n_pos, n_neg)
        assert torch.equal(both, index) and torch.equal(ptr, label_ptr)


def test_hetero_link_group_index_takes_views_and_int32_positions():
    """The halves of one [G, 2 half] tensor (non-contiguous views) and int32 positions give the same index."""
    local_src, local_dst, ptr, _ = _case(3, 6, 3, True, 4)
    joint = torch.cat([local_src, local_dst], 1)
    a, _ = hetero_link_group_index(joint[:, :9], joint[:, 9:], ptr, ptr, 6, 3)
    b, _ = hetero_link_group_index(local_src.int(), local_dst.int(), ptr.long(), ptr.long(), 6, 3)
    c, _ = hetero_link_group_index(local_src, local_dst, ptr, ptr, 6, 3)
    assert torch.equal(a, c) and torch.equal(b, c) and b.dtype == torch.int64
    with pytest.raises(AssertionError):
        hetero_link_group_index(local_src, local_dst[:, :-1], ptr, ptr, 6, 3)
