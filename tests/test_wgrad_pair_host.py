"""The block algebra of the pair-packed weight gradient (csrc/conv_wgrad_halo2.hip, H2P) in numpy float64, no GPU.

A 16-channel NHWC row of W pixels is a 32-channel row of W / 2 pixel pairs.  With k indexing the 16 pairs of a K step,

    A[m][k] = dy[2k + (m >= 16)][m % 16]          B[k][n] = x[2k + s + (n >= 16)][n % 16]

the 32 x 32 product holds four 16 x 16 blocks: (m<16, n<16) tap s over the even pixels, (m>=16, n>=16) tap s over the odd pixels,
(m<16, n>=16) tap s + 1 over the even pixels, (m>=16, n<16) tap s - 1 over the odd pixels.  Shift groups s = -1 and s = +1 give the
three kernel columns; two blocks are the offsets -2 / +2 and must be dropped.  The emulation walks the kernel's tiles (4 rows x 64
pixels, halo of one pixel, zero fill outside the image and behind a ragged edge) and reassembles dW exactly as the epilogue does;
the direct weight gradient is the yardstick, to 1e-12.  The up-sampled form (32 gathered channels, one pixel per k,
B[k][n] = a[y >> 1][j + floor(s / 2)][n], four shift groups) is covered by the same walk.
"""
import numpy as np
import pytest

TR, TW = 4, 64          # H2P<4, 2>


def direct_wgrad(x, dy):
    """dW[co][ky][kx][ci] = sum_p dy[p][co] * xpad[p + (ky - 1, kx - 1)][ci]; x [n][h][w][ci], dy [n][h][w][co], float64."""
    n, h, w, ci = x.shape
    xp = np.zeros((n, h + 2, w + 2, ci))
    xp[:, 1:-1, 1:-1] = x
    dw = np.zeros((dy.shape[-1], 3, 3, ci))
    for ky in range(3):
        for kx in range(3):
            dw[:, ky, kx, :] = np.einsum("nhwo,nhwi->oi", dy, xp[:, ky:ky + h, kx:kx + w])
    return dw


def offset_corr(x, dy, ky, off, parity):
    """sum over the pixels of column parity `parity` of dy[p] * x[p + (ky - 1, off)] (zero outside the image)."""
    n, h, w, ci = x.shape
    xp = np.zeros((n, h + 2, w + 6, ci))
    xp[:, 1:-1, 3:-3] = x
    sh = xp[:, ky:ky + h, 3 + off:3 + off + w]
    return np.einsum("nhwo,nhwi->oi", dy[:, :, parity::2], sh[:, :, parity::2])


def tiles(n, h, w):
    for img in range(n):
        for y0 in range(0, h, TR):
            for x0 in range(0, w, TW):
                yield img, y0, x0


def staged(t, img, y0, x0, rows, cols, c0, nc):
    """rows x cols pixels from (y0, x0), channels [c0, c0 + nc): what the range-checked loads leave in LDS (zero outside)."""
    n, h, w, c = t.shape
    out = np.zeros((rows, cols, nc))
    for r in range(rows):
        for q in range(cols):
            y, xx = y0 + r, x0 + q
            if 0 <= y < h and 0 <= xx < w:
                cc = min(nc, max(0, c - c0))
                out[r, q, :cc] = t[img, y, xx, c0:c0 + cc]
    return out


def pair_blocks(x, dy, cob):
    """acc[sg][ky]: the 32 x 32 accumulators of shift groups s = -1 (sg 0) and s = +1 (sg 1) for produced-channel block cob."""
    n, h, w, _ = x.shape
    acc = np.zeros((2, 3, 32, 32))
    for img, y0, x0 in tiles(n, h, w):
        X = staged(x, img, y0 - 1, x0 - 1, TR + 2, TW + 2, 0, 16)           # halo pixel hx = image column x0 + hx - 1
        D = staged(dy, img, y0, x0, TR, TW, 16 * cob, 16)
        Dp = D.reshape(TR, TW // 2, 32)                                      # the same bytes as pair rows: A[m][k] = Dp[r][k][m]
        for sg in range(2):
            Xp = X[:, 2 * sg:2 * sg + TW].reshape(TR + 2, TW // 2, 32)       # byte offset 64 sg of the row: B[k][n] = Xp[row][k][n]
            for ky in range(3):
                for r in range(TR):
                    acc[sg, ky] += Dp[r].T @ Xp[r + ky]
    return acc


def reassemble(acc, co, cob, dw):
    """The epilogue: the listed blocks -> the three kernel columns; rows >= co are never written."""
    rows = min(16, co - 16 * cob)
    for ky in range(3):
        c0 = acc[0, ky, :16, :16] + acc[0, ky, 16:, 16:]
        c1 = acc[0, ky, :16, 16:] + acc[1, ky, 16:, :16]
        c2 = acc[1, ky, :16, :16] + acc[1, ky, 16:, 16:]
        for kx, c in enumerate((c0, c1, c2)):
            dw[16 * cob:16 * cob + rows, ky, kx, :] += c[:rows]


@pytest.mark.parametrize("n,h,w,co", [(2, 6, 32, 16), (1, 5, 34, 16), (1, 9, 130, 16), (1, 6, 66, 24), (2, 4, 32, 24)],
                         ids=["16to16", "16to16_ragged", "16to16_two_tiles_wide", "16to24_ragged", "16to24"])
def test_paired_operands_reassemble_to_the_direct_gradient(n, h, w, co):
    rng = np.random.default_rng(n * 1000 + h * 100 + w + co)
    x = rng.standard_normal((n, h, w, 16))
    dy = rng.standard_normal((n, h, w, co))
    if co == 24:
        dy[..., 23] = 0.0           # 23 logical classes in 24 physical channels
    ref = direct_wgrad(x, dy)
    dw = np.zeros_like(ref)
    for cob in range((co + 15) // 16):
        acc = pair_blocks(x, dy, cob)
        reassemble(acc, co, cob, dw)
        # the two blocks the epilogue drops are the column offsets -2 (odd pixels) and +2 (even pixels): no tap of a 3 x 3 kernel
        rows = min(16, co - 16 * cob)
        for ky in range(3):
            m2 = offset_corr(x, dy[..., 16 * cob:16 * cob + rows], ky, -2, 1)
            p2 = offset_corr(x, dy[..., 16 * cob:16 * cob + rows], ky, +2, 0)
            assert np.abs(acc[0, ky, 16:16 + rows, :16] - m2).max() <= 1e-12 * np.abs(m2).max()
            assert np.abs(acc[1, ky, :rows, 16:] - p2).max() <= 1e-12 * np.abs(p2).max()
            assert np.abs(m2).max() > 1e-3 and np.abs(p2).max() > 1e-3          # not zero: storing them would be wrong
    assert np.abs(dw - ref).max() <= 1e-12 * np.abs(ref).max()


def test_rows_behind_the_physical_channels_stay_zero():
    rng = np.random.default_rng(5)
    x, dy = rng.standard_normal((1, 4, 32, 16)), rng.standard_normal((1, 4, 32, 24))
    acc = pair_blocks(x, dy, 1)
    assert not acc[:, :, 8:16].any() and not acc[:, :, 24:].any()          # channels 24 .. 31 of the second block were staged as zero


def up_blocks(a, dy):
    """The up-sampled form: dy paired (16 channels), x = nearest_x2(a) with 32 channels, one pixel per k:
    B[k][n] = x_up[2k + s][n] = a[y >> 1][j + floor(s / 2)][n], s in {-1, 0, 1, 2}.  acc[s + 1][ky] is 32 (m) x 32 (ci)."""
    n, ha, wa, ci = a.shape
    h, w = 2 * ha, 2 * wa
    acc = np.zeros((4, 3, 32, ci))
    for img, y0, x0 in tiles(n, h, w):
        D = staged(dy, img, y0, x0, TR, TW, 0, 16).reshape(TR, TW // 2, 32)
        j0 = x0 // 2
        for si, s in enumerate((-1, 0, 1, 2)):
            for ky in range(3):
                for r in range(TR):
                    y = y0 + r + ky - 1                       # row of the up-sampled image; outside: zero padding
                    B = np.zeros((TW // 2, ci))
                    if 0 <= y < h:
                        for k in range(TW // 2):
                            j = j0 + k + (s // 2)             # python's // is floor
                            if 0 <= j < wa:
                                B[k] = a[img, y >> 1, j]
                    acc[si, ky] += D[r].T @ B
    return acc


@pytest.mark.parametrize("n,ha,wa", [(2, 4, 16), (1, 3, 17), (1, 5, 40)], ids=["a_2x4x16", "ragged", "two_tiles_wide"])
def test_upsampled_form_reassembles_to_the_direct_gradient(n, ha, wa):
    rng = np.random.default_rng(n + ha + wa)
    a = rng.standard_normal((n, ha, wa, 32))
    dy = rng.standard_normal((n, 2 * ha, 2 * wa, 16))
    x_up = a.repeat(2, axis=1).repeat(2, axis=2)
    ref = direct_wgrad(x_up, dy)
    acc = up_blocks(a, dy)
    dw = np.zeros_like(ref)
    for ky in range(3):
        for si, s in enumerate((-1, 0, 1, 2)):
            if 0 <= s + 1 <= 2:
                dw[:, ky, s + 1, :] += acc[si, ky, :16]            # m < 16: tap s over the even pixels
            if 0 <= s <= 2:
                dw[:, ky, s, :] += acc[si, ky, 16:]                # m >= 16: tap s - 1 over the odd pixels
        m2 = offset_corr(x_up, dy, ky, -2, 1)
        p2 = offset_corr(x_up, dy, ky, +2, 0)
        assert np.abs(acc[0, ky, 16:] - m2).max() <= 1e-12 * np.abs(m2).max()          # odd half of s = -1: offset -2, dropped
        assert np.abs(acc[3, ky, :16] - p2).max() <= 1e-12 * np.abs(p2).max()          # even half of s = 2: offset +2, dropped
        # s = 0 and s = 1 read the same rows of a: one fragment serves both
    assert np.abs(dw - ref).max() <= 1e-12 * np.abs(ref).max()


def up_blocks_kernel(a, dy):
    """The up-sampled form as the kernel runs it: s = 0 and s = 1 are ONE product, so three products e = floor(s / 2) in {-1, 0, 1};
    an output row y reads only the rows (y >> 1) + py - 1 + u of a (py = y & 1, u in {0, 1}).  acc[py][u][e + 1] is 32 x 32."""
    n, ha, wa, ci = a.shape
    h, w = 2 * ha, 2 * wa
    AR, AW = TR // 2 + 2, TW // 2 + 2
    acc = np.zeros((2, 2, 3, 32, ci))
    for img, y0, x0 in tiles(n, h, w):
        D = staged(dy, img, y0, x0, TR, TW, 0, 16).reshape(TR, TW // 2, 32)
        X = staged(a, img, y0 // 2 - 1, x0 // 2 - 1, AR, AW, 0, ci)          # halo of a: row 0 = y0 / 2 - 1, pixel 0 = x0 / 2 - 1
        for r in range(TR):
            py, rsel = r & 1, r >> 1
            for u in range(2):
                for e in range(3):
                    acc[py, u, e] += D[r].T @ X[rsel + py + u, e:e + TW // 2]
    return acc


@pytest.mark.parametrize("n,ha,wa", [(2, 4, 16), (1, 3, 17), (1, 5, 40)], ids=["a_2x4x16", "ragged", "two_tiles_wide"])
def test_upsampled_form_as_the_kernel_runs_it(n, ha, wa):
    rng = np.random.default_rng(7 * n + ha + wa)
    a = rng.standard_normal((n, ha, wa, 32))
    dy = rng.standard_normal((n, 2 * ha, 2 * wa, 16))
    ref = direct_wgrad(a.repeat(2, axis=1).repeat(2, axis=2), dy)
    acc = up_blocks_kernel(a, dy)
    four = up_blocks(a, dy)
    dw = np.zeros_like(ref)
    rows = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}        # kernel rows a (py, u) accumulator stands for
    for (py, u), kys in rows.items():
        P = acc[py, u]
        for ky in kys:
            dw[:, ky, 0, :] += P[0, :16] + P[1, 16:]
            dw[:, ky, 1, :] += P[1, :16] + P[1, 16:]
            dw[:, ky, 2, :] += P[1, :16] + P[2, 16:]
    assert np.abs(dw - ref).max() <= 1e-12 * np.abs(ref).max()
    # the two shift groups that read the same rows of a hold the same sums
    assert np.abs(four[1] - four[2]).max() <= 1e-12 * np.abs(four[1]).max()
