"""GPU: the device-resident colour tables (csrc/raster_colors.hip behind flexam_amd/conditioning_raster.py).

Float32 tracks that live on the GPU never come back to the host and np.percentile is never called; the six videos are the bytes of
the host path.  Checked from the bottom up: the radix selection against np.sort, the percentiles against numpy's arithmetic restated
(tests/percentile_restatement.py), the three tables against the host functions on the downloaded tracks, the videos against the host
path and the reference's fixtures, and the property itself -- with np.percentile disabled and every device-to-host copy measured."""
import numpy as np
import pytest
import torch

import percentile_restatement as R
from oracle import make_golden_raster as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sorted_valid(values, mask):
    v = values if mask is None else values[mask]
    return np.sort(v)                                             # NaN last


def _select_case(values, segments, seg_len, ranks, mask=None, comp=0, inverse=False):
    """values: numpy [rows, C]; runs the selection and checks it against np.sort per segment."""
    from flexam_amd import hip as H
    src = torch.from_numpy(values).to(DEV)
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    r = torch.from_numpy(np.asarray(ranks, dtype=np.int64)).to(DEV)
    got, info = H.select_ranks(src, comp, segments, seg_len, r, m, inverse)
    again, info2 = H.select_ranks(src, comp, segments, seg_len, r, m, inverse)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(info, info2)          # repeatable
    _, counted = H.select_ranks(src, comp, segments, seg_len, None, m, inverse)
    assert torch.equal(counted, info)
    got, info = got.cpu().numpy(), info.cpu().numpy()
    col = values[:, comp]
    with np.errstate(divide="ignore"):
        x = (1 / (col + 1e-10)).astype(np.float32) if inverse else col
    for s in range(segments):
        sl = slice(s * seg_len, (s + 1) * seg_len)
        want = _sorted_valid(x[sl], None if mask is None else mask.reshape(-1)[sl])
        raw = col[sl] if mask is None else col[sl][mask.reshape(-1)[sl]]
        assert info[s, 0] == want.size and info[s, 1] == int(np.isnan(want).any()) and info[s, 2] == int((raw != 0).any()) and info[s, 3] == 0
        for k, rank in enumerate(np.asarray(ranks)[s]):
            if want.size == 0:
                assert np.isnan(got[s, k])
                continue
            w = want[min(max(int(rank), 0), want.size - 1)]
            assert got[s, k] == w or (np.isnan(w) and np.isnan(got[s, k])), (s, k, rank, got[s, k], w)


def test_selection_equals_sort():
    rng = np.random.default_rng(0)
    # one segment, a length that is no multiple of the workgroup's span, every kind of value
    n = 100_003
    a = rng.normal(0, 5, (n, 1)).astype(np.float32)
    a[rng.integers(0, n, 50), 0] = np.inf
    a[rng.integers(0, n, 50), 0] = -np.inf
    a[rng.integers(0, n, 50), 0] = 0.0
    a[rng.integers(0, n, 50), 0] = -0.0
    _select_case(a, 1, n, [[0, 2000, 2001, n - 1]])
    _select_case(a, 1, n, [[n // 2, n + 5, -3, 17]])                              # past the end: the last element; below 0: the first
    a[rng.integers(0, n, 3), 0] = np.nan
    _select_case(a, 1, n, [[0, n - 4, n - 3, n - 1]])
    # 97 masked segments of the z component of [.., 3] points (the per-frame depth percentiles' shape), depths of one exponent
    seg, t_n = 4099, 97
    p = rng.uniform(2.0, 4.0, (t_n * seg, 3)).astype(np.float32)
    mask = rng.random((t_n, seg)) > 0.3
    mask[5] = False                                                               # an empty segment
    mask[6] = False
    mask[6, 77] = True                                                            # a segment of one
    p[7 * seg:8 * seg, 2] = 2.5                                                   # all equal
    p[8 * seg + 3, 2] = np.nan
    ranks = np.stack([[int(0.02 * (c - 1)), int(0.02 * (c - 1)) + 1, int(0.98 * (c - 1)), min(int(0.98 * (c - 1)) + 1, max(c - 1, 0))]
                      for c in mask.sum(1)])
    _select_case(p, t_n, seg, ranks, mask, comp=2)
    _select_case(p, t_n, seg, ranks, None, comp=2, inverse=True)
    _select_case(p[:, :2].copy(), 3, 1000, [[1, 2], [3, 4], [998, 999]], None, comp=1)      # another stride
    # all zero: the flag the tracking colours branch on
    z = np.zeros((5000, 3), np.float32)
    z[::2, 2] = -0.0
    z[:, 0] = 1.0
    _select_case(z, 1, 5000, [[0, 4999]], None, comp=2, inverse=True)


def test_selection_over_forty_million_values():
    from flexam_amd import hip as H
    n = 97 * 413124
    g = torch.Generator(device=DEV).manual_seed(1)
    src = (torch.rand(n, 1, device=DEV, generator=g) * 6 + 2).contiguous()        # most of them share one exponent
    ranks = torch.tensor([[int(0.02 * (n - 1)), int(0.02 * (n - 1)) + 1, int(0.98 * (n - 1)), n - 1]], device=DEV)
    got, info = H.select_ranks(src, 0, 1, n, ranks, None, True)
    with np.errstate(divide="ignore"):
        want = np.sort((1 / (src.cpu().numpy()[:, 0] + 1e-10)).astype(np.float32))
    assert info.cpu().tolist() == [[n, 0, 1, 0]]
    assert got.cpu().numpy()[0].tolist() == want[ranks.cpu().numpy()[0]].tolist()


def test_selection_argument_errors():
    from flexam_amd import hip as H
    src = torch.zeros(100, 3, device=DEV)
    ranks = torch.zeros(1, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="segments"):
        H.select_ranks(src, 2, 2, 100, None)                                       # more rows than the tensor has
    with pytest.raises(RuntimeError, match="comp"):
        H.select_ranks(src, 3, 1, 100, ranks)                                      # the C ABI's own checks: code + message
    with pytest.raises(RuntimeError, match="K=9"):
        H.select_ranks(src, 2, 1, 100, torch.zeros(1, 9, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="ranks"):
        H.select_ranks(src, 2, 1, 100, ranks.to(torch.int32))
    with pytest.raises(RuntimeError, match="mask"):
        H.select_ranks(src, 2, 1, 100, ranks, torch.ones(50, dtype=torch.bool, device=DEV))
    lib = H.lib()
    assert lib.flexam_select_f32(src.data_ptr(), 3, 2, 0, None, 1, 100, None, 0, None, torch.zeros(4, dtype=torch.int64, device=DEV).data_ptr(),
                                 torch.zeros(4, dtype=torch.int32, device=DEV).data_ptr(), 16, None) == -1
    assert b"workspace" in lib.flexam_last_error()
    with pytest.raises(RuntimeError):
        H.raster_colors_tracking(src, 8, 8)
    with pytest.raises(RuntimeError, match="lut"):
        H.raster_colors_depth(src.view(1, 100, 3), None, torch.zeros(1, 2, dtype=torch.float64, device=DEV), torch.zeros(256, 3, dtype=torch.uint8, device=DEV))


def _clips():
    """name -> (points [T, N, 3] float32, visibility [T, N] bool)."""
    out = {}
    for name in ("plain", "edges", "foreground", "wide"):
        pts, vis, _, _, _ = G.case(name)
        out[name] = (np.ascontiguousarray(pts, dtype=np.float32), np.asarray(vis).reshape(pts.shape[:2]).astype(bool))
    rng = np.random.default_rng(21)
    t_n, n, h, w = 9, 20011, 96, 160
    pts = np.stack([rng.uniform(-8, w + 8, (t_n, n)), rng.uniform(-8, h + 8, (t_n, n)), rng.uniform(0.4, 7.0, (t_n, n))], -1).astype(np.float32)
    vis = rng.random((t_n, n)) > 0.2
    vis[2] = False                                                 # a frame with no visible point
    vis[3] = False
    vis[3, 123] = True                                             # ... with one
    vis[4, 50] = True
    pts[5, :, 2] = 1.75                                            # p98 == p2
    pts[6, :40, 2] = 0.0
    pts[6, 40:80, 0] = np.nan
    pts[6, 80:90, 1] = np.inf
    out["dense"] = (pts, vis)
    with_nan = pts.copy()
    with_nan[4, 50, 2] = np.nan                                    # a NaN among the visible depths of frame 4 (and so of the whole clip)
    out["dense_nan"] = (with_nan, vis)
    return out


@pytest.mark.parametrize("name", ("plain", "edges", "foreground", "wide", "dense", "dense_nan"))
def test_percentiles_and_tables_equal_the_host_functions(name):
    from flexam_amd import conditioning_raster as P
    from flexam_amd import hip as H
    pts, vis = _clips()[name]
    h, w = (96, 160) if name.startswith("dense") else (G.H, G.W)
    d_pts, d_vis = torch.from_numpy(pts).to(DEV), torch.from_numpy(vis).to(DEV).view(torch.uint8)
    t_n, n, _ = pts.shape
    # percentiles, both forms, against the restatement
    with np.errstate(divide="ignore"):
        inv0, inv_all = (1 / (pts[0, :, 2] + 1e-10)).astype(np.float32), (1 / (pts[:, :, 2] + 1e-10)).astype(np.float32)
    for src, segs, seg_len in ((inv0, 1, n), (inv_all, 1, t_n * n)):
        got, _ = P._device_percentiles(d_pts, segs, seg_len, None, True, True)
        assert got.dtype == torch.float32
        want = np.array([R.percentile(src, q, True) for q in (2, 98)], dtype=np.float32)
        assert np.array_equal(got.cpu().numpy()[0], want, equal_nan=True), (got, want)
    got, info = P._device_percentiles(d_pts, t_n, n, d_vis, False, False)
    assert got.dtype == torch.float64
    for t in range(t_n):
        d = pts[t, vis[t], 2]
        assert info[t, 0] == d.size
        if d.size:
            want = np.array([R.percentile(d, q, False) for q in (2, 98)])
            assert np.array_equal(got[t].cpu().numpy(), want, equal_nan=True), (t, got[t], want)
    # tables
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        assert np.array_equal(P._tracking_colors_device(d_pts, h, w).cpu().numpy(), P._tracking_colors(pts[0], h, w))
        assert np.array_equal(P._depth_colors_device(d_pts, d_vis).cpu().numpy(), P._depth_colors(pts, vis))
        assert np.array_equal(P._depth_colors_device(d_pts, None).cpu().numpy(), P._depth_colors(pts, np.ones_like(vis)))
        codes = P.apply_cosine_positional_encoding(d_pts, h, w, 4)
        assert len(codes) == 4 and codes[0].shape == d_pts.shape
        first = P._cosine_codes(d_pts, h, w, 4, None, frames=1)
        for i in range(4):
            want = P._generate_colors_from_points(codes[i][0].cpu().numpy(), n)
            assert np.array_equal(H.raster_colors_cosine(codes[i][0].contiguous()).cpu().numpy(), want)
            assert torch.equal(first[i][0].view(torch.int32), codes[i][0].contiguous().view(torch.int32))      # frame 0 of the full code, NaN included


def _parent_cosine_codes(pts, height, width, L):
    """apply_cosine_positional_encoding as it stood before the device path, for a tensor on the GPU: torch's device kernels for the
    code, np.percentile on a host copy of the inverse depths."""
    x_n = torch.clamp((pts[:, :, 0] - 0) / (width - 0), 0, 1)
    y_n = torch.clamp((pts[:, :, 1] - 0) / (height - 0), 0, 1)
    inv_z = 1 / (pts[:, :, 2] + 1e-10)
    inv_np = inv_z.detach().cpu().numpy()
    p2, p98 = np.percentile(inv_np, 2), np.percentile(inv_np, 98)
    p2_t, p98_t = torch.tensor(p2, device=inv_z.device, dtype=inv_z.dtype), torch.tensor(p98, device=inv_z.device, dtype=inv_z.dtype)
    z_n = torch.clamp((inv_z - p2_t) / (p98_t - p2_t + 1e-10), 0, 1)
    norm = torch.zeros_like(pts)
    norm[:, :, 0], norm[:, :, 1], norm[:, :, 2] = x_n, y_n, z_n
    return [torch.cos(((2 ** i) * np.pi) * norm) for i in range(L)]


def test_all_zero_depths_take_the_generators():
    from flexam_amd import conditioning_raster as P
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(0, 64, (3, 700)), rng.uniform(0, 64, (3, 700)), np.zeros((3, 700))], -1).astype(np.float32)
    pts[1, ::2, 2] = -0.0
    d_pts = torch.from_numpy(pts).to(DEV)
    assert np.array_equal(P._tracking_colors_device(d_pts, 64, 64, np.random.default_rng(4)).cpu().numpy(),
                          P._tracking_colors(pts[0], 64, 64, np.random.default_rng(4)))
    assert np.array_equal(P._tracking_colors_device(d_pts, 64, 64, np.random.RandomState(4)).cpu().numpy(),
                          P._tracking_colors(pts[0], 64, 64, np.random.RandomState(4)))
    a = P.visualize_tracking_DELTA(d_pts, None, False, 4, 64, 64, 2, generator=np.random.default_rng(4), torch_generator=torch.Generator().manual_seed(9))
    b = P.visualize_tracking_DELTA(pts, None, False, 4, 64, 64, 2, generator=np.random.default_rng(4), torch_generator=torch.Generator().manual_seed(9), device=DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    full = P.apply_cosine_positional_encoding(d_pts, 64, 64, 2, generator=torch.Generator().manual_seed(9))
    want = P._visualize_cosine_encoded_tracking(full, d_pts, None, 64, 64)
    assert all(torch.equal(a[1][i], want[i]) for i in range(2))


@pytest.mark.parametrize("name", ("plain", "edges", "foreground", "wide", "dense", "dense_nan"))
def test_videos_from_device_tracks_equal_the_host_path(golden, name):
    from flexam_amd import conditioning_raster as P
    if name.startswith("dense"):
        (pts, vis), mask, gen, pw, h, w = _clips()[name], None, "full_edit", 4, 96, 160
    else:
        pts, vis, mask, gen, pw = G.case(name)
        pts, h, w = np.ascontiguousarray(pts, dtype=np.float32), G.H, G.W
    d_pts = torch.from_numpy(pts).to(DEV)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tr, cos, dep = P.visualize_tracking_DELTA(d_pts, torch.from_numpy(np.asarray(vis)), False, pw, h, w, 4, gen, mask_video=mask)
        h_tr, _, h_dep = P.visualize_tracking_DELTA(pts, np.asarray(vis), False, pw, h, w, 4, gen, mask_video=mask, device=DEV)
        assert tr.is_cuda and torch.equal(tr, h_tr) and torch.equal(dep, h_dep)
        # the cosine videos: today's pieces on the same device tensor -- the parent's code for a GPU tensor, its host colour function
        parent = _parent_cosine_codes(d_pts, h, w, 4)
        colours = [P._generate_colors_from_points(e[0].cpu().numpy(), pts.shape[1]) for e in parent]
    fr = P._Frames(pts, P._prepare_vis_mask(np.asarray(vis), pts.shape), h, w, P._mask_for(mask, gen, pts.shape[0], h, w, torch.device(DEV)), torch.device(DEV))
    for i in range(4):
        assert torch.equal(cos[i], fr.video(colours[i], 2, 0)), i
    by = lambda v: (v[0].permute(1, 2, 3, 0).cpu() * 255).round().to(torch.uint8).numpy()
    if not name.startswith("dense"):
        g = golden(f"g13_raster_{name}")
        assert np.array_equal(by(tr), g["tracking"].numpy()) and np.array_equal(by(dep), g["depth"].numpy())
        assert all(np.array_equal(by(cos[i]), g[f"cos{i}"].numpy()) for i in range(4))
    # the single-video functions take the same path
    vis_t = torch.from_numpy(np.asarray(vis)).to(DEV)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u8 = P.fun_visualize_tracking_with_depth(d_pts, vis_t, h, w, pw, mask, gen)
        assert np.array_equal(u8.cpu().numpy(), by(tr))
        assert torch.equal(P._visualize_depth_tracking(d_pts, vis_t, h, w, pw, mask_video=mask, generate_type=gen), dep)
        one = P._visualize_cosine_encoded_tracking(P.apply_cosine_positional_encoding(d_pts, h, w, 2), d_pts, vis_t, h, w, mask_video=mask, generate_type=gen)
    assert torch.equal(one[1], cos[1])


def test_device_tracks_never_reach_the_host(monkeypatch):
    """The property: with np.percentile disabled a call with CUDA float32 tracks succeeds where the same call with the numpy copy
    raises, and nothing larger than the selection's counts and flags is copied to the host."""
    from flexam_amd import conditioning_raster as P
    rng = np.random.default_rng(8)
    t_n, n, h, w = 97, 6000, 96, 160
    pts = np.stack([rng.uniform(0, w, (t_n, n)), rng.uniform(0, h, (t_n, n)), rng.uniform(0.5, 6, (t_n, n))], -1).astype(np.float32)
    vis = rng.random((t_n, n)) > 0.1
    d_pts, d_vis = torch.from_numpy(pts).to(DEV), torch.from_numpy(vis).to(DEV)
    want = P.visualize_tracking_DELTA(pts, vis, False, 4, h, w, 4, device=DEV)
    copies = []

    def wrap(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            to_host = name != "to" or any(torch.device(x).type == "cpu" for x in list(a) + list(k.values()) if isinstance(x, (str, torch.device)))
            if self.is_cuda and to_host:
                copies.append((name, self.numel() * self.element_size()))
            return real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, f)
    for name in ("cpu", "numpy", "tolist", "item", "to"):
        wrap(name)

    def no_percentile(*a, **k):
        raise AssertionError("np.percentile called")
    monkeypatch.setattr(np, "percentile", no_percentile)
    got = P.visualize_tracking_DELTA(d_pts, d_vis, False, 4, h, w, 4)
    codes = P.apply_cosine_positional_encoding(d_pts, h, w, 2)
    assert codes[1].shape == d_pts.shape
    biggest = max(size for _, size in copies)
    print(f"device-to-host copies: {len(copies)}, the largest {biggest} bytes")
    assert copies and biggest <= 4096, copies                    # 97 segments x (count, 3 flags) x 8 bytes = 3104
    with pytest.raises(AssertionError, match="np.percentile called"):
        P.visualize_tracking_DELTA(pts, vis, False, 4, h, w, 4, device=DEV)
    with pytest.raises(AssertionError, match="np.percentile called"):
        P.visualize_tracking_DELTA(d_pts.double(), d_vis, False, 4, h, w, 4)          # float64 on the device keeps the host path
    monkeypatch.undo()
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and len(got[1]) == 4
