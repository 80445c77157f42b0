"""CPU: the generator of filter_edge_cases.py puts non-finite rows on the edges it names (so
test_gpu_filter_edges.py means what it says)."""
import numpy as np
import pytest

import filter_edge_cases as fc


def _base(m=1000):
    return np.random.default_rng(0).normal(0.0, 10.0, (m, 6)).astype(np.float32)


@pytest.mark.parametrize("n", fc.SIZES + (fc.SIZE_SECOND_CHUNK,))
def test_rows_are_on_the_edges(n):
    a = fc.edge_cloud(_base(), n)
    assert a.shape == (n, 6) and a.dtype == np.float32
    finite = np.isfinite(a[:, :3]).all(axis=1)
    bad = np.nonzero(~finite)[0]
    assert np.array_equal(bad, fc.bad_rows(n))
    assert not finite[0] and not finite[n - 1]                       # first and last row
    if n > fc.BLOCK:                                                 # both sides of a block boundary
        assert not finite[fc.BLOCK - 1] and not finite[fc.BLOCK]
    elif n == fc.BLOCK:                                              # the block's last row is the cloud's last
        assert not finite[fc.BLOCK - 1]
    if n > 2:
        assert finite[1:n - 1].any()                                 # … and the filter has rows to keep
    if n > fc.SCAN_CHUNK * fc.BLOCK:
        blk = finite[: n - n % fc.BLOCK].reshape(-1, fc.BLOCK)
        assert not blk[fc.DEAD_BLOCK].any()                          # one whole block dropped
        assert blk[fc.DEAD_BLOCK - 1].any() and blk[fc.DEAD_BLOCK + 1].any()
        assert not finite[fc.SCAN_CHUNK * fc.BLOCK - 1] and not finite[fc.SCAN_CHUNK * fc.BLOCK]   # chunk two opens
    kinds = a[bad, :3][~np.isfinite(a[bad, :3])]
    if len(bad) >= 3:
        assert np.isnan(kinds).any() and (kinds == np.inf).any() and (kinds == -np.inf).any()
        assert all((~np.isfinite(a[bad, d])).any() for d in range(3))  # in x, in y, in z
    assert np.array_equal(fc.kept_rows(a), np.nonzero(finite)[0])


def test_sizes_are_the_block_edges():
    assert fc.SIZES == (1, 255, 256, 257, 262145)
    assert fc.SIZE_SECOND_CHUNK // fc.BLOCK > fc.SCAN_CHUNK           # a full block of kept rows in chunk two
    a = fc.edge_cloud(_base(), fc.SIZE_SECOND_CHUNK)
    assert np.isfinite(a[fc.SCAN_CHUNK * fc.BLOCK + 1:fc.SCAN_CHUNK * fc.BLOCK + fc.BLOCK, :3]).all()


@pytest.mark.parametrize("n", fc.SIZES[1:])
def test_nan_normal_on_a_kept_row(n):
    a = fc.edge_cloud(_base(), n)
    r = fc.nan_normal_row(n)
    assert r >= 0 and np.isfinite(a[r, :3]).all() and np.isnan(a[r, 3:]).all()
    assert r in fc.kept_rows(a)
    assert fc.nan_normal_row(1) == -1 and len(fc.kept_rows(fc.edge_cloud(_base(), 1))) == 0


def test_passes_over_the_base_do_not_coincide():
    a = fc.edge_cloud(_base(100), 257)
    ok = np.isfinite(a[:, :3]).all(axis=1)
    assert len(np.unique(a[ok, :3], axis=0)) == ok.sum()
