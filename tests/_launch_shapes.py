"""Launch shapes of the capped-grid pixel kernels outside the convolutions, restated for the tests: every launcher below caps its
grid and lets the kernel walk the rest of its input in a grid-stride loop, and a case "past the grid" has to be chosen from
these figures (tests/_loss_cases.py::grid_pix / passes and tests/_pool_ref.py::grid_for do the same for their families).

One function per launcher -> ``Launch(blocks, threads, trips, per_trip)``: the grid's x extent, the block size, the trips the
busiest thread (or wave) makes round the loop and the items all blocks cover in one trip -- pixels, except for the nearest
resize, where an item is a group of four destination pixels of one row.  ``first_trip_*`` give the items of trip one as a mask
(what a kernel that never came round again would have touched); tests/test_launch_shapes_host.py reads every cap out of the
``.hip`` text and holds it against the constants here, so a cap changed in csrc/ fails there and does not silently move a case
back to one trip."""
from collections import namedtuple

import numpy as np

Launch = namedtuple("Launch", "blocks threads trips per_trip")

# the caps, by launcher (csrc/<file>: what the host test reads them from)
PREPARE_BATCH_CAP = 1024        # data_prep.hip      gx = ... > 1024 ? 1024 : ...
AUG_OUTPUT_CAP = 1024           # augment.hip        gx = ... > 1024 ? 1024 : ...
PREDICT_GATHER_CAP = 256        # predict.hip        capped_grid(tp, 256, 256)
PREDICT_FINISH_CAP = 8192       # predict.hip        capped_grid(pixels, 256, 8192)
PREDICT_THRESHOLD_CAP = 1024    # predict.hip        capped_grid(hw, 256, 1024)
ARGMAX_CONFUSION_CAP = 1024     # losses.hip         capped_grid(pixels, 256, 1024) of udaseg_argmax_confusion
CH_CELLS = 32768                # pseudo.hip         table cells of one class group
CH_THREADS = 1024
CH_BLOCKS = 256                 # pseudo.hip         blocks of ALL class groups together
PL_THREADS = 256
PL_MAX_BLOCKS = 2048            # pseudo.hip         a wave takes a chunk of 256 pixels
PA_CU = 256                     # proto.hip          PaShape<DV>::max_blocks = PA_CU * (1024 / threads)
PR_THREADS = 256
PR_MAX_BLOCKS = 4096            # proto.hip
PC_THREADS = 256
PC_MAX_BLOCKS = 4096            # proto_contrast.hip
RESIZE_NEAREST_CAP = 1024       # resize.hip         cdiv64(groups, 256) > 1024 ? 1024 : ...
PL_CHUNK = 256                  # pixels a wave of pseudo_labels_kernel takes at a time
PA_CHUNK = 64                   # pixels a wave of proto_accumulate_kernel takes at a time


def _cdiv(a, b):
    return -(-a // b)


def _flat(items, threads, cap):
    """capped_grid(items, threads, cap) with one item per thread and trip."""
    blocks = max(min(_cdiv(items, threads), cap), 1)
    return Launch(blocks, threads, _cdiv(items, blocks * threads), blocks * threads)


def _waves(items, chunk, threads, cap):
    """One chunk of ``chunk`` items per wave and trip: capped_grid(chunks, threads / 64, cap)."""
    waves = threads // 64
    chunks = _cdiv(items, chunk)
    blocks = max(min(_cdiv(chunks, waves), cap), 1)
    return Launch(blocks, threads, _cdiv(chunks, blocks * waves), blocks * waves * chunk)


def prepare_batch(h, w):
    """prepare_batch_kernel: per image (blockIdx.y)."""
    return _flat(h * w, 256, PREPARE_BATCH_CAP)


def aug_output(h, w):
    """aug_output_kernel, all eight instantiations: per image and view."""
    return _flat(h * w, 256, AUG_OUTPUT_CAP)


def predict_gather(th, tw):
    """predict_gather_kernel: per tile and view."""
    return _flat(th * tw, 256, PREDICT_GATHER_CAP)


def predict_finish(pixels):
    return _flat(pixels, 256, PREDICT_FINISH_CAP)


def predict_threshold(hw):
    """predict_threshold_kernel: per image."""
    return _flat(hw, 256, PREDICT_THRESHOLD_CAP)


def argmax_confusion(pixels):
    return _flat(pixels, 256, ARGMAX_CONFUSION_CAP)


def conf_hist_groups(classes, bins):
    """Class groups of conf_hist_kernel (blockIdx.y): each group re-reads the scores."""
    return _cdiv(classes, min(classes, CH_CELLS // bins))


def conf_hist(pixels, classes, bins):
    blocks = max(min(CH_BLOCKS // conf_hist_groups(classes, bins), _cdiv(pixels, CH_THREADS)), 1)
    return Launch(blocks, CH_THREADS, _cdiv(pixels, blocks * CH_THREADS), blocks * CH_THREADS)


def pseudo_labels(pixels):
    return _waves(pixels, PL_CHUNK, PL_THREADS, PL_MAX_BLOCKS)


def proto_accumulate_threads(dim):
    dv = dim // 4
    return 1024 if dv <= 4 else 512 if dv <= 8 else 256


def proto_accumulate(pixels, dim):
    threads = proto_accumulate_threads(dim)
    return _waves(pixels, PA_CHUNK, threads, PA_CU * (1024 // threads))


def proto_rectify(pixels):
    return _flat(pixels, PR_THREADS, PR_MAX_BLOCKS)


def proto_assign(pixels):
    return _flat(pixels, PC_THREADS, PC_MAX_BLOCKS)


def resize_nearest(h, w):
    """resize_nearest_kernel: per image; an item is a group of four destination pixels of one row (the last may be short)."""
    return _flat(h * _cdiv(w, 4), 256, RESIZE_NEAREST_CAP)


def first_trip(launch, items):
    """bool [items]: the items trip one covers (the kernels walk their items in ascending order, blocks side by side)."""
    return np.arange(items) < launch.per_trip


def first_trip_nearest(h, w):
    """bool [h, w]: the destination pixels whose four-pixel group falls into trip one."""
    w4 = _cdiv(w, 4)
    group = np.arange(h)[:, None] * w4 + np.arange(w)[None, :] // 4
    return group < resize_nearest(h, w).per_trip
