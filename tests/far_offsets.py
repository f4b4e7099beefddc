"""Rows, edges and output elements more than 2 GiB and more than 4 GiB from their base pointer.

One device allocation of 2^32 + 2^16 four-byte elements (16 GiB + 256 KiB), filled ONCE with float32 NaN (bits 0x7FC00000),
serves every table, ``col`` array and far output of tests/test_gpu_far_offsets.py as a view.  Only a few hundred rows of it are
ever live: a kernel that truncates an offset (an ``int`` product, a 32-bit byte offset, a lost high word) reads the fill —
NaN as float32, every other element NaN as fp16 / bf16, 2143289344 as an int32 id — or another live row's different numbers.

``band_rows`` picks the live rows: ``per_band`` rows on either side of each threshold — byte offset 2^31, byte offset 2^32,
element index 2^31, element index 2^32 — plus row 0 and the last row of the view.  Where the row length divides a threshold the
band holds the row whose last byte is the last byte below it and the row that starts exactly on it; otherwise it holds the row
that straddles it.

What a wrapped read lands on.  The thresholds are multiples of one another (2^32 = 2 * 2^31, and an element threshold is a
byte threshold times the element size), so the row that starts on byte 2^32 wraps, modulo 2^31, onto the row that starts on
byte 2^31, and both wrap onto row 0: the rows the bands must hold alias one another by construction and no choice of rows can
avoid it.  ``wrap_collisions`` lists, for a set of rows, every (row, modulus, other row) where the row's position taken modulo
2^31 or 2^32 (in bytes and in elements) comes within one row length of another chosen row's true position.  ``band_rows``
asserts the part that can hold: every such collision is between two rows of the threshold bands or row 0 (whose values
``place`` requires to be pairwise different, so the wrapped read returns another row's numbers and an exact comparison fails),
and the extra rows (``more``, the last row of the view) collide with nothing: their wrapped reads land on the NaN fill.
"""
import numpy as np

N_ELEMS = (1 << 32) + (1 << 16)          # four-byte elements of the far buffer
N_BYTES = 4 * N_ELEMS
NAN_BITS = 0x7FC00000                    # float32 NaN as torch.fill_ writes it
MIN_FREE_BYTES = 32 << 30                # the module is skipped on a device with less free memory than this
_MODULI = (1 << 31, 1 << 32)


def n_rows_of(F, elem_bytes, n_bytes=N_BYTES):
    """Rows of the [rows, F] view of ``n_bytes`` bytes."""
    return n_bytes // (F * elem_bytes)


def thresholds(elem_bytes):
    """The four thresholds as byte offsets (duplicates merged), ascending."""
    return sorted({1 << 31, 1 << 32, (1 << 31) * elem_bytes, (1 << 32) * elem_bytes})


def wrap_collisions(rows, F, elem_bytes):
    """[(row, modulus in bytes, other row)]: ``row``'s byte position modulo ``modulus`` differs from its position and lies within
    one row length of ``other``'s.  Moduli: 2^31 and 2^32 bytes, 2^31 and 2^32 elements."""
    L = F * elem_bytes
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    pos = rows * L
    out = []
    for m in sorted({M * s for M in _MODULI for s in (1, elem_bytes)}):
        wrapped = pos % m
        for i in np.nonzero(wrapped != pos)[0]:
            near = np.nonzero(np.abs(pos - wrapped[i]) < L)[0]
            out += [(int(rows[i]), m, int(rows[j])) for j in near if j != i]
    return out


def band_rows(F, elem_bytes, per_band, n_bytes=N_BYTES, more=()):
    """Row ids of the [rows, F] view (elements of ``elem_bytes`` bytes) that straddle every threshold inside the view, ``per_band``
    rows on each side, plus row 0, the last row and ``more``; ascending, int64.  See the module docstring for what it asserts."""
    L = F * elem_bytes
    n_rows = n_rows_of(F, elem_bytes, n_bytes)
    band = {0}
    for T in thresholds(elem_bytes):
        r0 = T // L                      # the row that starts on the threshold, or the one that straddles it
        if r0 - per_band < 0 or r0 + per_band > n_rows:
            continue                     # a threshold outside this view (element index 2^32 of an int64 view)
        band.update(range(r0 - per_band, r0 + per_band))
        if T % L == 0:
            assert (r0 - 1) * L + L - 1 == T - 1 and r0 * L == T
    extra = {n_rows - 1} | {int(r) for r in more}
    assert all(0 <= r < n_rows for r in extra)
    rows = np.array(sorted(band | extra), dtype=np.int64)
    only_extra = extra - band
    for r, m, s in wrap_collisions(rows, F, elem_bytes):
        assert r not in only_extra and s not in only_extra, \
            "row %d wraps (mod %d bytes) onto row %d: one of them is not a threshold row" % (r, m, s)
    # within one band nothing but the neighbouring rows themselves: the bands are far apart
    assert len(rows) == len(band | extra)
    return rows


def spread_rows(F, elem_bytes, low=12, high=12, n_bytes=N_BYTES):
    """Extra live rows between the bands: ``low`` rows spread over the first 2^31 bytes (a table kept below 2 GiB still has a
    dozen rows to read) and ``high`` over the rest of the view; odd steps, so that none sits at a round position."""
    L = F * elem_bytes
    n_rows = n_rows_of(F, elem_bytes, n_bytes)
    first = ((1 << 31) - 1) // L
    lo = [first * k // (low + 1) + 3 * k + 11 for k in range(1, low + 1)]
    hi = [first + (n_rows - first) * k // (high + 1) + 5 * k + 17 for k in range(1, high + 1)]
    return lo + hi


def live_rows(F, elem_bytes, per_band=4, n_bytes=N_BYTES):
    """The live rows of a GPU case: the bands, row 0, the last row and ``spread_rows`` (checked by ``band_rows``)."""
    return band_rows(F, elem_bytes, per_band, n_bytes, more=spread_rows(F, elem_bytes, n_bytes=n_bytes))


def sage_extents(F):
    """The three extents (in rows) of a float32 [rows, F] table the one-kernel SAGE layer is run at: the largest table below
    2^31 bytes (32-bit offsets), the first one of at least 2^31 bytes (64-bit offsets), the full view."""
    L = F * 4
    below = ((1 << 31) - 1) // L
    return below, -(-(1 << 31) // L), n_rows_of(F, 4)


# ---------------------------------------------------------------------------------------------------------------------
# device side (torch imported on use: the host-side test of band_rows needs none of it)
# ---------------------------------------------------------------------------------------------------------------------
def enough_memory():
    """(ok, reason) from one ``torch.cuda.mem_get_info()`` query."""
    import torch
    free, total = torch.cuda.mem_get_info()
    return free >= MIN_FREE_BYTES, "far-offset tests need %d GiB of free device memory, %.1f GiB free of %.1f" % (
        MIN_FREE_BYTES >> 30, free / 2**30, total / 2**30)


def far_buffer(n_elems=N_ELEMS):
    """The far buffer: ``n_elems`` float32 on the current device, every one NaN."""
    import torch
    buf = torch.empty(n_elems, dtype=torch.float32, device="cuda")
    buf.fill_(float("nan"))
    return buf


def view(buf, F, dtype, rows=None):
    """The [rows, F] view of ``buf`` as ``dtype`` from its first byte (``rows``: fewer than the whole buffer holds)."""
    flat = buf.view(dtype)
    n = flat.numel() // F if rows is None else int(rows)
    assert n * F <= flat.numel()
    return flat[:n * F].view(n, F)


def flat_view(buf, dtype, n=None):
    """``buf`` as a 1-D array of ``dtype`` (a CSR's ``col``, a weights array)."""
    flat = buf.view(dtype)
    return flat if n is None else flat[:n]


def strided_view(buf, n_rows, width, ld):
    """float32 [n_rows, width] with row stride ``ld`` elements from the first byte of ``buf``."""
    assert (n_rows - 1) * ld + width <= buf.numel() and ld >= width
    return buf.as_strided((n_rows, width), (ld, 1))


def spanning_ld(n_rows, width, align=4):
    """A row stride (in float32 elements, a multiple of ``align``) at which ``n_rows`` rows of ``width`` span the whole far buffer:
    the last row ends within one stride of its end, so the rows cross all four thresholds."""
    ld = ((N_ELEMS - width) // (n_rows - 1)) // align * align
    assert (n_rows - 1) * ld + width <= N_ELEMS and (n_rows - 1) * ld > (1 << 32) - ld
    return ld


def place(v, rows, values):
    """Write the live rows: ``v[rows[i]] = values[i]``.  The values must differ row from row (a wrapped read that lands on another
    live row must not return the right numbers by accident)."""
    import torch
    rows = torch.as_tensor(np.asarray(rows), device=v.device).long()
    values = torch.as_tensor(values, device=v.device).to(v.dtype)
    assert values.shape == (rows.numel(),) + tuple(v.shape[1:])
    if values.dim() == 2 and values.shape[0] > 1:
        assert torch.unique(values, dim=0).shape[0] == values.shape[0], "live rows must be pairwise different"
    v[rows] = values


def clear(v, rows):
    """Set the rows of ``v`` back to the fill (whatever the view's dtype)."""
    import torch
    rows = torch.as_tensor(np.asarray(rows), device=v.device).long()
    row_bytes = v[0].numel() * v.element_size()
    assert v.dim() == 2 and row_bytes % 4 == 0 and v.stride(1) == 1
    words = torch.full((rows.numel(), row_bytes // 4), NAN_BITS, dtype=torch.int32, device=v.device)
    v[rows] = words.view(v.dtype).view((rows.numel(),) + tuple(v.shape[1:]))


def clear_span(flat, lo, hi):
    """Set elements [lo, hi) of a 1-D view (4- or 8-byte elements) back to the fill."""
    import torch
    flat[lo:hi].view(torch.int32).fill_(NAN_BITS)


def is_fill(v, rows):
    """True when every byte of the rows of ``v`` still holds the fill."""
    import torch
    rows = torch.as_tensor(np.asarray(rows), device=v.device).long()
    got = v[rows].contiguous().view(torch.int32)
    return bool((got == NAN_BITS).all())


def neighbours(rows, n_rows):
    """The rows next to ``rows`` that are not in ``rows`` themselves (they must stay untouched)."""
    rows = np.asarray(rows, dtype=np.int64)
    near = np.unique(np.concatenate([rows - 1, rows + 1]))
    near = near[(near >= 0) & (near < n_rows)]
    return np.setdiff1d(near, rows)
