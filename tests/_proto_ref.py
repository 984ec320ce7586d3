"""numpy float64 mirrors of the prototype kernels for the tests: ``update_mirror`` / ``rectify_mirror`` are the package's own
host statements of ``udaseg_proto_update`` / ``udaseg_proto_rectify``; the accumulate mirror and the derived bars live here."""
import numpy as np

from uda_aerial_semantic_segmentation_research_amd.proto import rectify_mirror, update_mirror  # noqa: F401


def accumulate_mirror(features, labels, classes):
    """``features [P, D]`` fp32, ``labels [P]`` uint8 -> ``(sums [C, D], sq [C], counts [C + 2], abs_sums [C, D], abs_sq [C])`` in
    float64 / int64 under ``udaseg_proto_accumulate``'s rules; ``abs_sums`` / ``abs_sq`` are the sums of the magnitudes the
    error bar of a cell is derived from."""
    f = np.asarray(features, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    D = f.shape[1]
    finite = np.isfinite(f).all(axis=1)
    sums, sq = np.zeros((classes, D)), np.zeros(classes)
    abs_sums, abs_sq = np.zeros((classes, D)), np.zeros(classes)
    counts = np.zeros(classes + 2, dtype=np.int64)
    counts[classes + 1] = int((~finite).sum())
    counts[classes] = int((finite & (lab >= classes)).sum())
    for c in range(classes):
        rows = f[finite & (lab == c)]
        counts[c] = len(rows)
        sums[c] = rows.sum(axis=0)
        abs_sums[c] = np.abs(rows).sum(axis=0)
        norm2 = np.zeros(len(rows))
        for j in range(D):                                           # a pixel's squared norm: ascending j, as the kernel forms it
            norm2 = norm2 + rows[:, j] * rows[:, j]
        sq[c] = abs_sq[c] = norm2.sum()
    return sums, sq, counts, abs_sums, abs_sq


def sum_bars(counts, abs_sums, abs_sq):
    """Two float64 summations of the same n numbers in any two orders differ by at most ``2 (n - 1) 2^-53 sum|x|``: the bar per
    cell is ``n_c 2^-52 sum|x|``."""
    n = np.asarray(counts[:len(abs_sq)], dtype=np.float64)
    return n[:, None] * 2.0 ** -52 * abs_sums, n * 2.0 ** -52 * abs_sq
