"""Edge cases of the NaN filter (csrc/filter.hip), shared by test_filter_edge_cases.py — which proves on
numpy alone that the generator puts rows on the edges it names — and test_gpu_filter_edges.py, which
runs them on the device.  No GPU imports.

The filter keeps a row when its x, y, z are finite (RemoveNANandINFData), in input order.  The lone
path (k_flag_finite → device scan → k_compact / k_compact_posed) and the batched path
(k_filter_count_b → k_filter_scan_b → k_filter_scatter_b) work in blocks of 256 rows; the batched
scan takes a job's block counts 1,024 at a time, so row 262,144 opens its second chunk.

Clouds are (n, 6) float32 rows x y z nx ny nz.
"""
import numpy as np

BLOCK = 256                          # internal.h kBlock: rows per filter block
SCAN_CHUNK = 1024                    # filter.hip k_filter_scan_b: block counts per chunk
SIZES = (1, 255, 256, 257, SCAN_CHUNK * BLOCK + 1)
# past the sizes the lone path needs: the batched scan's second chunk holding kept rows too
SIZE_SECOND_CHUNK = SCAN_CHUNK * BLOCK + BLOCK + 100
DEAD_BLOCK = 2                       # the block whose rows are all non-finite (where the cloud has it)


def bad_rows(n):
    """The rows edge_cloud(…, n) makes non-finite: 0 and n−1, both sides of the first 256 boundary,
    one whole block, both sides of the batched scan's chunk boundary."""
    rows = {0, n - 1, BLOCK - 1, BLOCK, SCAN_CHUNK * BLOCK - 1, SCAN_CHUNK * BLOCK}
    rows |= set(range(DEAD_BLOCK * BLOCK, (DEAD_BLOCK + 1) * BLOCK)) if n > (DEAD_BLOCK + 2) * BLOCK else set()
    return np.array(sorted(r for r in rows if 0 <= r < n), np.int64)


def nan_normal_row(n):
    """A kept row whose normal is NaN (the filter tests xyz alone); −1: the cloud has no kept row."""
    keep = np.setdiff1d(np.arange(n), bad_rows(n))
    return int(keep[len(keep) // 2]) if len(keep) else -1


def edge_cloud(base, n):
    """n rows cycled from the finite (m, 6) rows `base` (each pass over them shifted by 1 mm in x, so
    passes do not coincide), the rows of bad_rows(n) made non-finite — NaN, +inf, −inf in x, y, z by
    turns — and one kept row given a NaN normal."""
    base = np.asarray(base, np.float32).reshape(-1, 6)
    i = np.arange(n)
    a = base[i % len(base)].copy()
    a[:, 0] += (i // len(base)).astype(np.float32) * np.float32(1e-3)
    for k, r in enumerate(bad_rows(n)):
        a[r, k % 3] = (np.nan, np.inf, -np.inf)[(k + k // 3) % 3]
    if nan_normal_row(n) >= 0:
        a[nan_normal_row(n), 3:] = np.nan
    return a


def kept_rows(a6):
    """The reference: the input index of every row with finite x, y, z, in order."""
    return np.nonzero(np.isfinite(np.asarray(a6)[:, :3]).all(axis=1))[0].astype(np.uint32)
