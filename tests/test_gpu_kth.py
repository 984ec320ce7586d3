"""kernels.kth_smallest (csrc/ohem.hip: udaseg_kth_hist + udaseg_kth_select, the three-level radix select) alone, on crafted buffers,
with EXACT equality against np.sort (tests/_ohem_ref.kth_smallest): the bits of the result, -inf for k == 0, +inf for k > n."""
import numpy as np
import pytest
import torch

import _ohem_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 1000, 70001)
KINDS = ("all_equal", "low_bits_only", "mid_bits_only", "zero_denormal_one", "half_void", "random")
HIST_TRIP = 256 * 256 * 4                # values one full grid of udaseg_kth_hist takes in one trip


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    return kernels


def ranks(n):
    return sorted({0, 1, n // 2, max(n - 1, 0), n, n + 5})


def crafted(kind, n):
    rng = np.random.default_rng(100 * KINDS.index(kind) + n % 97)
    base = np.float32(0.7).view(np.uint32)
    if kind == "all_equal":
        return np.full(n, 0.625, dtype=np.float32)
    if kind == "low_bits_only":          # bits 29..10 agree: levels 0 and 1 see ONE bin, level 2 decides
        return ((base & ~np.uint32(1023)) | rng.integers(0, 1024, n).astype(np.uint32)).view(np.float32)
    if kind == "mid_bits_only":          # only bits 19..10 differ: level 1 decides, level 2 sees one bin
        return ((base & ~np.uint32(0xFFC00)) | (rng.integers(0, 1024, n).astype(np.uint32) << 10)).view(np.float32)
    v = rng.random(n).astype(np.float32)
    if kind == "zero_denormal_one":
        v[rng.integers(0, n, max(n // 10, 1))] = 0.0
        v[rng.integers(0, n, max(n // 10, 1))] = 1.0
        v[rng.integers(0, n, max(n // 10, 1))] = np.uint32(1).view(np.float32)
        if n >= 3:
            v[:3] = [1.0, np.uint32(1).view(np.float32), 0.0]
    if kind == "half_void":
        v[rng.permutation(n)[: n // 2]] = -1.0
    return v


def bits(x):
    return np.asarray(x, dtype=np.float32).reshape(1).view(np.uint32)[0]


def check(K, v, tag):
    dev = torch.from_numpy(v).cuda()
    n_live = int((v.view(np.uint32) < (1 << 30)).sum())
    ks = ranks(n_live)
    got = torch.stack([K.kth_smallest(dev, k) for k in ks]).cpu().numpy()
    for k, g in zip(ks, got):
        want, n2 = R.kth_smallest(v, k)
        assert n2 == n_live
        assert bits(g) == bits(want), f"{tag} k={k} of n={n_live}: got {g!r} ({bits(g):#x}), np.sort says {want!r} ({bits(want):#x})"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_kth_smallest_equals_np_sort(K, kind, n):
    check(K, crafted(kind, n), f"{kind} n={n}")


def test_second_trip_of_the_capped_histogram_grid(K):
    """One value more than a full grid takes in one trip, and the smallest values placed in that tail."""
    v = crafted("random", HIST_TRIP + 1000)
    v[HIST_TRIP:] *= np.float32(1e-3)
    check(K, v, "second trip")


def test_buffer_that_is_not_16_byte_aligned(K):
    """A view one float into an allocation takes the scalar-load kernel."""
    v = crafted("random", 1001)
    dev = torch.from_numpy(v).cuda()[1:]
    assert dev.data_ptr() % 16 != 0
    for k in ranks(1000):
        assert bits(K.kth_smallest(dev, k).cpu().numpy()) == bits(R.kth_smallest(v[1:], k)[0]), k


def test_the_same_call_twice_gives_the_same_bits(K):
    dev = torch.from_numpy(crafted("random", 70001)).cuda()
    a, b = K.kth_smallest(dev, 35000), K.kth_smallest(dev, 35000)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_arguments_raise(K):
    with pytest.raises(ValueError):
        K.kth_smallest(torch.zeros(4, device="cuda", dtype=torch.float64), 1)
    with pytest.raises(ValueError):
        K.kth_smallest(torch.zeros(4, device="cuda"), -1)
    with pytest.raises(ValueError):
        K.kth_smallest(torch.zeros(0, device="cuda"), 1)
