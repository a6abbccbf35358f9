"""Dispatch order of the sweep step kernels (csrc/amvs_strip_order.h), checked on the HOST copy of the very
function the kernels call (amvs_sweep_order; no GPU needed).

For every launch shape of the grid below the edge-first decode must
  * enumerate every (job, strip row, strip column) of the launch exactly once;
  * give every XCD (block b runs on XCD b % 8) exactly the strips the top-to-bottom order gives it -- its L2
    footprint is unchanged, only the start order inside its range differs;
  * start, inside every XCD's range, the bands of a view (band-major: of the launch) that lie in the upper half
    of the image top to bottom and, after them, those in the lower half bottom to top.
"""
import numpy as np
import pytest

JOBS = list(range(1, 34))
BANDS = [1, 2, 3, 4, 5, 7, 8, 19, 54, 55]         # 1, 2, odd and even strip-row counts
COLS = [1, 2, 3, 34]                               # strip columns (34: 1920 pixels wide, 58-column strips)


def _order(n_jobs, tx, ty, band_major, paired, edge_first):
    from amvs import _lib
    o = _lib.sweep_order(n_jobs, tx, ty, band_major=band_major, paired=paired, edge_first=edge_first)
    assert not (o == -2).any(), "a record was not written"
    return o


def _strips(o):
    live = o[..., 0] >= 0
    return o[live][:, :3]


def _check_shape(n_jobs, tx, ty, band_major, paired):
    new = _order(n_jobs, tx, ty, band_major, paired, True)
    old = _order(n_jobs, tx, ty, band_major, paired, False)
    assert new.shape == old.shape
    tag = f"jobs={n_jobs} tiles={ty}x{tx} band_major={band_major} paired={paired}"
    # every strip exactly once
    s = _strips(new)
    want = n_jobs * tx * ty
    assert len(s) == want, tag
    key = (s[:, 0].astype(np.int64) * ty + s[:, 1]) * tx + s[:, 2]
    assert len(np.unique(key)) == want and key.min() == 0 and key.max() == want - 1, tag
    # dead waves carry -1 everywhere, live waves of a pair have consistent flags
    dead = new[..., 0] < 0
    assert (new[dead] == -1).all(), tag
    if paired:
        live = ~dead
        assert (new[live][:, 3] == new[live][:, 1] % 2).all(), tag
        partner = (new[live][:, 1] // 2) * 2 + 1 < ty
        assert (new[live][:, 4] == partner).all(), tag
    else:
        assert (new[~dead][:, 3:] == 0).all(), tag
    half = (ty + 1) // 2 if not paired else 2 * (((ty + 1) // 2 + 1) // 2)   # first strip row of the lower half
    for xcd in range(min(8, new.shape[0])):
        a, b = new[xcd::8], old[xcd::8]
        ka = {tuple(r) for r in _strips(a)}
        kb = {tuple(r) for r in _strips(b)}
        assert ka == kb, f"{tag}: XCD {xcd} owns other strips than before"
        # start order: the first live wave of each block names the block's (job, row)
        first = np.array([blk[blk[:, 0] >= 0][0, :2] for blk in a if (blk[:, 0] >= 0).any()])
        if band_major:
            groups = [first]
        else:
            groups = [first[first[:, 0] == j] for j in np.unique(first[:, 0])]
            # the views themselves stay in ascending order
            assert (np.diff(first[:, 0]) >= 0).all(), tag
        for g in groups:
            rows = g[:, 1]
            upper = rows < half
            n_up = int(upper.sum())
            assert upper[:n_up].all() and not upper[n_up:].any(), f"{tag}: XCD {xcd} upper part must come first"
            assert (np.diff(rows[:n_up]) >= 0).all(), f"{tag}: XCD {xcd} upper part walks down"
            assert (np.diff(rows[n_up:]) <= 0).all(), f"{tag}: XCD {xcd} lower part walks up"


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n_jobs", JOBS)
def test_edge_first_order_view_major(n_jobs, paired):
    for ty in BANDS:
        for tx in COLS:
            _check_shape(n_jobs, tx, ty, False, paired)


@pytest.mark.parametrize("n_jobs", JOBS)
def test_edge_first_order_band_major(n_jobs):
    for ty in BANDS:
        for tx in COLS:
            _check_shape(n_jobs, tx, ty, True, False)


def test_grids_smaller_than_eight_workgroups():
    seen = 0
    for n_jobs in (1, 2, 3):
        for ty in (1, 2, 3):
            for tx in (1, 2, 3, 5):
                for paired in (False, True):
                    o = _order(n_jobs, tx, ty, False, paired, True)
                    if o.shape[0] < 8:
                        seen += 1
                        _check_shape(n_jobs, tx, ty, False, paired)
    assert seen > 20


def test_top_to_bottom_order_is_the_previous_decode():
    """edge_first = 0 is the order the kernels used before: strip t = 4 * remapped block + wave, view-major."""
    n_jobs, tx, ty = 4, 34, 55
    o = _order(n_jobs, tx, ty, False, False, False)
    nblk = o.shape[0]
    q, r = divmod(nblk, 8)
    for bid in (0, 1, 7, 8, 9, nblk - 1):
        xcd = bid % 8
        base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        for wv in range(4):
            t = (base + bid // 8) * 4 + wv
            if t >= n_jobs * tx * ty:
                assert o[bid, wv, 0] == -1
                continue
            job, rem = divmod(t, tx * ty)
            assert tuple(o[bid, wv, :3]) == (job, rem // tx, rem % tx)

