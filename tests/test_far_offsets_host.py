"""Host-side checks of tests/far_offsets.py: the rows ``band_rows`` picks straddle every threshold the way the GPU cases rely
on, and what a wrapped read of each of them lands on is what the module's docstring says.  No GPU, no torch."""
import numpy as np
import pytest

import far_offsets as fo

CASES = [(100, 4), (128, 4), (256, 4), (128, 2)]     # (F, element bytes): fp32 at F = 100 / 128 / 256, fp16 at F = 128


@pytest.mark.parametrize("F,elem", CASES)
@pytest.mark.parametrize("per_band", [1, 3])
def test_band_rows_straddle_every_threshold(F, elem, per_band):
    L = F * elem
    n_rows = fo.n_rows_of(F, elem)
    rows = fo.band_rows(F, elem, per_band)
    assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0)
    assert rows[0] == 0 and rows[-1] == n_rows - 1 and (n_rows - 1) * L + L <= fo.N_BYTES
    live = set(rows.tolist())
    ths = fo.thresholds(elem)
    assert {1 << 31, 1 << 32, (1 << 31) * elem, (1 << 32) * elem} == set(ths) and all(T + per_band * L <= fo.N_BYTES for T in ths)
    for T in ths:
        below = [r for r in live if (r + 1) * L <= T]
        above = [r for r in live if r * L >= T]
        across = [r for r in live if r * L < T < (r + 1) * L]
        if T % L == 0:
            # the row whose last byte is the last byte below the threshold, and the row that starts exactly on it
            assert T // L - 1 in live and (T // L - 1) * L + L - 1 == T - 1
            assert T // L in live and not across
            want_below, want_above = per_band, per_band
        else:
            assert across == [T // L]
            want_below, want_above = per_band, per_band - 1
        # per_band consecutive rows on each side, touching the threshold
        assert all(T // L - 1 - k in live for k in range(want_below)) and len(below) >= want_below
        assert all(T // L + (T % L != 0) + k in live for k in range(want_above)) and len(above) >= want_above
    # element-index thresholds, stated in elements: a row holds element 2^31 - 1 or 2^31, and 2^32 - 1 or 2^32
    for e in (1 << 31, 1 << 32):
        assert any(r * F <= e - 1 < (r + 1) * F for r in live) and any(r * F <= e < (r + 1) * F for r in live)


@pytest.mark.parametrize("F,elem", CASES)
def test_a_wrapped_read_lands_on_the_fill_or_on_a_different_threshold_row(F, elem):
    """Position modulo 2^31 and 2^32, in bytes and in elements, against every other chosen row's position.  The threshold rows
    alias one another (the thresholds are multiples of one another): every collision stays among them and row 0, whose values
    differ row from row.  The last row of the view and any extra row collide with nothing: their wrapped reads land on NaN."""
    L = F * elem
    n_rows = fo.n_rows_of(F, elem)
    extra = [n_rows // 3 + 17, n_rows - 12345]
    rows = fo.band_rows(F, elem, 3, more=extra)
    band = set(fo.band_rows(F, elem, 3).tolist()) - {n_rows - 1}
    hits = fo.wrap_collisions(rows, F, elem)
    assert hits, "2^32 bytes wraps onto 2^31 bytes and both onto row 0: the bands must collide"
    for r, m, s in hits:
        assert r in band and s in band, (r, m, s)
        assert (r * L) % m != r * L and abs((r * L) % m - s * L) < L
    for r in extra + [n_rows - 1]:
        assert all(r not in (a, b) for a, _, b in hits)
    # the check is not vacuous: it refuses an extra row that a threshold row wraps onto
    with pytest.raises(AssertionError):
        fo.band_rows(F, elem, 3, more=[n_rows // 3 + 17, 1])
    # wrap_collisions itself, on a hand-made pair: row a = row b + 2^32 bytes exactly when L divides 2^32
    if (1 << 32) % L == 0:
        a, b = 40 + (1 << 32) // L, 40
        assert (a, 1 << 32, b) in fo.wrap_collisions([a, b], F, elem)
        assert not fo.wrap_collisions([a, b + 2], F, elem)


@pytest.mark.parametrize("F,elem", CASES + [(64, 4), (4, 4), (32, 4), (128, 8)])
def test_live_rows_of_the_gpu_cases_pass_the_collision_check(F, elem):
    """The exact row sets tests/test_gpu_far_offsets.py places: ``band_rows`` accepts them (its assertion runs here, without a
    GPU), they are a few hundred at most, and a dozen of them lie below 2^31 bytes."""
    rows = fo.live_rows(F, elem)
    wide = fo.live_rows(F, elem, per_band=44)            # (the cases that need more input rows than destinations)
    assert set(rows.tolist()) <= set(wide.tolist()) and (elem != 4 or 333 <= len(wide) <= 400)
    assert 30 <= len(rows) <= 300 and len(set(rows.tolist())) == len(rows)
    assert int((rows * F * elem < (1 << 31) - F * elem).sum()) >= 12
    assert rows[-1] == fo.n_rows_of(F, elem) - 1


def test_sage_extents_sit_on_either_side_of_two_gib():
    for F in (100, 128, 256):
        below, first64, full = fo.sage_extents(F)
        assert below * F * 4 < (1 << 31) <= (below + 1) * F * 4
        assert (first64 - 1) * F * 4 < (1 << 31) <= first64 * F * 4
        assert full == fo.N_BYTES // (F * 4) and full * F * 4 > (1 << 34)
        if (1 << 31) % (F * 4) == 0:
            assert below * F * 4 == (1 << 31) - F * 4 and first64 * F * 4 == 1 << 31


def test_spanning_stride_crosses_all_thresholds():
    for n, w in ((300, 128), (317, 64), (333, 256)):
        ld = fo.spanning_ld(n, w)
        starts = np.arange(n, dtype=np.int64) * ld * 4
        assert ld % 4 == 0 and starts[-1] + w * 4 <= fo.N_BYTES
        for T in fo.thresholds(4):
            assert (starts < T).any() and (starts >= T).any()


def test_sage_wgrad_refuses_a_row_stride_its_tile_offsets_cannot_hold(hiplib):
    """wgamd_sage_wgrad_bf16x3 reads agg, grad_out and act_out per tile of up to 64 rows with 32-bit byte offsets from the tile's
    first row: a row stride of 2^24 floats or more is refused on the host (nothing is launched, no pointer is followed).  Strides of
    12.9 M floats are accepted and checked in tests/test_gpu_far_offsets.py (test_sage_wgrad_band_rows_and_strided_operands)."""
    import ctypes
    from wholegraph_amd import _lib as L
    buf = np.zeros(1024, np.float32)
    rows = np.zeros(8, np.int64)
    at = buf.ctypes.data + (-buf.ctypes.data) % 16
    F, N, n = 64, 32, 8
    need = hiplib.wgamd_sage_wgrad_workspace_bytes(n, F, N)
    assert need > 0

    def call(ld_agg, ldg, ld_act, ws_bytes):      # (host memory stands in for the operands: the refusal comes first)
        return hiplib.wgamd_sage_wgrad_bf16x3(at, ld_agg, at, F, F, None, 0, rows.ctypes.data, n, at, ldg, at if ld_act else None, ld_act,
                                              N, at, at, None, 0, ctypes.c_void_p(at), ws_bytes, None)
    for lds in ((1 << 24, N, 0), (F, 1 << 24, 0), (F, N, 1 << 24), (1 << 40, N, 0)):
        assert call(*lds, need) == L.WHOLEMEMORY_INVALID_INPUT, lds
