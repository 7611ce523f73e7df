"""A numpy restatement of demo.py's foreground-edit mask refinement (demo.py:33-96), the yardstick of tests/test_edit_masks_*.py.

It restates the reference's scipy / OpenCV call sequence from their documented behaviour, independently of csrc/edit_mask.hip:
  blur      scipy.ndimage.gaussian_filter (truncate 4, mode 'reflect'): fp64 sums in correlate1d's order, float32 after each axis;
  hull      8-connected components; per component the convex hull of its pixel centres (Andrew's monotone chain); the pixels whose
            centres lie in the closed hull, plus the hull's edges drawn as 8-connected lines (along the major axis, the minor
            coordinate is floor(exact + 1/2)); components with collinear centres give nothing;
  dilate    cv2.dilate with MORPH_ELLIPSE of size (2r+1)^2, pixels outside the frame contributing nothing: per row the distance to the
            nearest set pixel, then one compare per element row.
No SciPy or OpenCV here (tests/test_edit_masks_cpu.py holds the blur to SciPy where SciPy is installed)."""
import numpy as np


def gaussian_weights(sigma):
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def _reflect(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gaussian_blur(img, sigma):
    """float32 [H, W] -> float32 [H, W], as scipy.ndimage.gaussian_filter(img, sigma)."""
    w = gaussian_weights(sigma)
    r = (len(w) - 1) // 2
    out = np.asarray(img, np.float32)
    for axis in (0, 1):
        a = np.moveaxis(out, axis, -1).astype(np.float64)
        n = a.shape[-1]
        ext = a[..., _reflect(np.arange(-r, n + r), n)]
        acc = ext[..., r:r + n] * w[r]
        for j in range(r, 0, -1):
            acc = acc + (ext[..., r - j:r - j + n] + ext[..., r + j:r + j + n]) * w[r + j]
        out = np.moveaxis(acc.astype(np.float32), -1, axis)
    return np.ascontiguousarray(out)


def components(b):
    """8-connected components of a bool [H, W] image: list of (ys, xs) index arrays."""
    H, W = b.shape
    runs = []                                   # (y, s, e)
    row_runs = []
    for y in range(H):
        d = np.diff(np.concatenate([[0], b[y].astype(np.int8), [0]]))
        s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1
        row_runs.append(list(range(len(runs), len(runs) + len(s))))
        runs += [(y, int(a), int(c)) for a, c in zip(s, e)]
    par = list(range(len(runs)))

    def find(i):
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i

    for y in range(1, H):
        for i in row_runs[y]:
            _, s, e = runs[i]
            for j in row_runs[y - 1]:
                _, s2, e2 = runs[j]
                if s2 <= e + 1 and e2 >= s - 1:
                    a, c = find(i), find(j)
                    if a != c:
                        par[max(a, c)] = min(a, c)
    groups = {}
    for i, (y, s, e) in enumerate(runs):
        groups.setdefault(find(i), []).append((y, s, e))
    out = []
    for g in groups.values():
        ys = np.concatenate([np.full(e - s + 1, y) for y, s, e in g])
        xs = np.concatenate([np.arange(s, e + 1) for y, s, e in g])
        out.append((ys, xs))
    return out


def convex_hull(points):
    """Andrew's monotone chain on integer (x, y) points: counter-clockwise vertices (y down), collinear points dropped."""
    pts = sorted(set(map(tuple, points)))
    if len(pts) < 3:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def line_pixels(p, q):
    """8-connected pixels of the segment p -> q ((x, y) integers): one per step of the major axis, the minor coordinate
    floor(exact + 1/2) (a half goes to the larger coordinate, whichever way the segment runs)."""
    (x0, y0), (x1, y1) = p, q
    dx, dy = x1 - x0, y1 - y0
    if abs(dx) >= abs(dy):
        if dx < 0:
            x0, y0, dx, dy = x1, y1, -dx, -dy
        if dx == 0:
            return np.array([x0]), np.array([y0])
        xs = np.arange(x0, x0 + dx + 1)
        ys = y0 + np.floor_divide(2 * (xs - x0) * dy + dx, 2 * dx)
        return xs, ys
    if dy < 0:
        x0, y0, dx, dy = x1, y1, -dx, -dy
    ys = np.arange(y0, y0 + dy + 1)
    xs = x0 + np.floor_divide(2 * (ys - y0) * dx + dy, 2 * dy)
    return xs, ys


def fill_component(shape, ys, xs, out):
    """ORs into `out` the closed convex hull of the pixel centres plus the hull's edges as 8-connected lines; nothing when the
    centres are collinear."""
    hull = convex_hull(np.stack([xs, ys], 1))
    if len(hull) < 3:
        return
    h = np.array(hull)
    x0, x1, y0, y1 = h[:, 0].min(), h[:, 0].max(), h[:, 1].min(), h[:, 1].max()
    gy, gx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    inside = np.ones(gx.shape, bool)
    for i in range(len(h)):
        a, b = h[i], h[(i + 1) % len(h)]
        inside &= (b[0] - a[0]) * (gy - a[1]) - (b[1] - a[1]) * (gx - a[0]) >= 0
    out[y0:y1 + 1, x0:x1 + 1] |= inside
    for i in range(len(h)):
        lx, ly = line_pixels(tuple(h[i]), tuple(h[(i + 1) % len(h)]))
        out[ly, lx] = True


def hull_fill(b):
    out = np.zeros(b.shape, bool)
    for ys, xs in components(b):
        fill_component(b.shape, ys, xs, out)
    return out


def ellipse_half_widths(r):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (2r+1, 2r+1)) row half widths for |dy| = 0 .. r (cvRound = half to even)."""
    dy = np.arange(r + 1)
    return np.rint(r * np.sqrt((r * r - dy * dy) * (1.0 / (r * r)))).astype(np.int64)


def ellipse_element(r):
    hw = ellipse_half_widths(r)
    dx = np.abs(np.arange(-r, r + 1))
    return np.stack([dx <= hw[abs(dy)] for dy in range(-r, r + 1)])


def row_distances(b):
    """Per pixel, the horizontal distance to the nearest set pixel of its row (a large number when the row is empty)."""
    H, W = b.shape
    big = 1 << 20
    idx = np.arange(W)
    last = np.where(b, idx, -big)
    last = np.maximum.accumulate(last, axis=1)
    nxt = np.where(b, idx, big + W)
    nxt = np.minimum.accumulate(nxt[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(idx - last, nxt - idx)


def dilate(b, r):
    if r <= 0:
        return b.copy()
    hw = ellipse_half_widths(r)
    d = row_distances(b)
    H = b.shape[0]
    out = np.zeros(b.shape, bool)
    for dy in range(-r, r + 1):
        lo, hi = max(0, -dy), min(H, H - dy)
        if lo < hi:
            out[lo:hi] |= d[lo + dy:hi + dy] <= hw[abs(dy)]
    return out


def refine_frame(grey, blur_radius=15, dilation_pixels=200):
    """One frame after frame 0: grey [H, W] (channel mean) -> uint8 {0, 1} [H, W]."""
    b = grey > 0.5
    if blur_radius > 0:
        b = gaussian_blur(b.astype(np.float32), blur_radius / 6.0) > 0.5
    return dilate(hull_fill(b), dilation_pixels).astype(np.uint8)


def blob_video(frames, height, width, seed=0, blobs=3):
    """Seeded moving-blob mask video [F, 3, H, W] in 0-255 (ellipses drifting across the frame, one of them with a hole)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    c0 = rng.uniform([0.2 * height, 0.2 * width], [0.8 * height, 0.8 * width], (blobs, 2))
    v = rng.uniform(-2.0, 2.0, (blobs, 2))
    ax = rng.uniform(0.05, 0.15, (blobs, 2)) * np.array([height, width])
    out = np.zeros((frames, 3, height, width), np.float32)
    for f in range(frames):
        m = np.zeros((height, width), bool)
        for k in range(blobs):
            cy, cx = c0[k] + v[k] * f
            d = ((yy - cy) / ax[k, 0]) ** 2 + ((xx - cx) / ax[k, 1]) ** 2
            m |= (d < 1.0) & ~((k == 0) & (d < 0.3))
        out[f, :, m] = 255.0
    return out
