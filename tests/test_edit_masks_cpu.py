"""CPU: the numpy restatement of the foreground-edit mask refinement (tests/edit_mask_restatement.py) that the GPU tests compare
flexam_amd.edit_masks with: its blur against scipy.ndimage.gaussian_filter, its element against the row formula, its hull fill against
a brute-force hull; and the host tables flexam_amd.edit_masks hands to the kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_mask_restatement as R  # noqa: E402


def test_blur_is_bit_exact_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for i in range(120):
        h, w = rng.integers(5, 91, 2)
        b = (rng.random((h, w)) < rng.uniform(0.05, 0.95)).astype(np.float32)
        sigma = [15 / 6.0, 7 / 6.0, 40 / 6.0][i % 3]
        want = ndimage.gaussian_filter(b, sigma=sigma)
        got = R.gaussian_blur(b, sigma)
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, h, w, sigma)


def test_library_weights_are_the_restatements():
    from flexam_amd import edit_masks as E
    for br in (1, 7, 15, 40):
        w = R.gaussian_weights(br / 6.0)
        r = (len(w) - 1) // 2
        assert np.array_equal(E.gaussian_weights(br), w[r:])
    for r in (1, 2, 7, 30, 200):
        assert np.array_equal(E.ellipse_half_widths(r), R.ellipse_half_widths(r))


@pytest.mark.parametrize("r", [1, 2, 3, 7, 30, 200])
def test_element_matches_the_row_formula_and_is_symmetric(r):
    el = R.ellipse_element(r)
    assert el.shape == (2 * r + 1, 2 * r + 1)
    assert np.array_equal(el, el[::-1]) and np.array_equal(el, el[:, ::-1])
    for dy in range(-r, r + 1):
        half = int(np.rint(r * np.sqrt((r * r - dy * dy) / (r * r))))
        assert np.array_equal(np.flatnonzero(el[dy + r]) - r, np.arange(-half, half + 1))
    assert el[r].all() and el[:, r].all()


def _brute_hull_fill(b):
    """Every pixel in the closed convex hull of a component's centres (tested against every pair of centres: a point is outside
    exactly when some line through two centres has it strictly on one side and every centre on the other or on it), plus the
    8-connected lines between consecutive hull vertices."""
    out = np.zeros(b.shape, bool)
    H, W = b.shape
    gy, gx = np.mgrid[0:H, 0:W]
    for ys, xs in R.components(b):
        pts = np.stack([xs, ys], 1)
        if len(pts) < 3:
            continue
        inside = np.ones(b.shape, bool)
        for i in range(len(pts)):
            for j in range(len(pts)):
                if i == j or (pts[i] == pts[j]).all():
                    continue
                a, c = pts[i], pts[j]
                side = (c[0] - a[0]) * (pts[:, 1] - a[1]) - (c[1] - a[1]) * (pts[:, 0] - a[0])
                if (side >= 0).all():
                    inside &= (c[0] - a[0]) * (gy - a[1]) - (c[1] - a[1]) * (gx - a[0]) >= 0
        if inside.sum() == 0 or np.linalg.matrix_rank(pts[1:] - pts[0]) < 2:
            continue                                   # collinear centres: nothing
        out |= inside
        hull = R.convex_hull(pts)
        for i in range(len(hull)):
            lx, ly = R.line_pixels(hull[i], hull[(i + 1) % len(hull)])
            out[ly, lx] = True
    return out


def test_hull_fill_matches_brute_force_and_is_one_interval_per_row():
    rng = np.random.default_rng(1)
    for i in range(60):
        h, w = rng.integers(4, 14, 2)
        b = rng.random((h, w)) < rng.uniform(0.1, 0.5)
        got = R.hull_fill(b)
        assert np.array_equal(got, _brute_hull_fill(b)), i
        # what csrc/edit_mask.hip relies on: one component's filled hull is a single interval per row
        for ys, xs in R.components(b):
            one = np.zeros(b.shape, bool)
            R.fill_component(b.shape, ys, xs, one)
            for row in one:
                nz = np.flatnonzero(row)
                assert len(nz) == 0 or nz[-1] - nz[0] + 1 == len(nz), i


def test_collinear_components_and_line_tie_rule():
    b = np.zeros((9, 12), bool)
    b[1, 1:6] = True                    # one row
    b[3:8, 10] = True                   # one column
    b[4, 2], b[5, 3], b[6, 4] = True, True, True     # a 45-degree diagonal
    assert not R.hull_fill(b).any()
    xs, ys = R.line_pixels((0, 0), (2, 1))            # y(1) = 1/2 exactly: the half goes to the larger y
    assert list(zip(xs, ys)) == [(0, 0), (1, 1), (2, 1)]
    xs2, ys2 = R.line_pixels((2, 1), (0, 0))
    assert sorted(zip(xs2, ys2)) == sorted(zip(xs, ys))


def test_dilation_matches_direct_element_sweep():
    rng = np.random.default_rng(2)
    for r in (1, 2, 7):
        b = rng.random((23, 31)) < 0.03
        el = R.ellipse_element(r)
        want = np.zeros_like(b)
        for y, x in zip(*np.nonzero(b)):
            for dy, dx in zip(*np.nonzero(el)):
                yy, xx = y + dy - r, x + dx - r
                if 0 <= yy < b.shape[0] and 0 <= xx < b.shape[1]:
                    want[yy, xx] = True
        assert np.array_equal(R.dilate(b, r), want), r
