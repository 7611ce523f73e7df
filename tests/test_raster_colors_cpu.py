"""CPU: the arithmetic the device-resident colour tables rest on (flexam_amd/conditioning_raster.py, csrc/raster_colors.hip).

The device path selects order statistics exactly and then interpolates as numpy does, so numpy's roundings are restated
(tests/percentile_restatement.py, and `_percentile_index` in the package, which the device path calls) and pinned here against the
installed numpy bit for bit: a numpy that changes `_lerp` or its index arithmetic shows up here and not as a colour."""
import numpy as np
import pytest

import percentile_restatement as R

SIZES = (1, 2, 3, 50, 51, 1000, 28672, 413124)


def _contents(kind, n, rng):
    if kind == "uniform":
        return rng.uniform(0.5, 9.5, n).astype(np.float32)
    if kind == "ties":
        return rng.integers(1, 6, n).astype(np.float32)
    if kind == "one_exponent":
        return rng.uniform(2.0, 4.0, n).astype(np.float32)[::-1].copy()
    if kind == "inverse_depth":
        return (1 / (rng.uniform(0.5, 9.5, n).astype(np.float32) + 1e-10)).astype(np.float32)
    if kind == "inf":
        a = rng.normal(0, 3, n).astype(np.float32)
        a[rng.integers(0, n, max(1, n // 20))] = np.inf
        a[rng.integers(0, n, max(1, n // 20))] = -np.inf
        return a
    if kind == "nan":
        a = rng.uniform(0.5, 9.5, n).astype(np.float32)
        a[rng.integers(0, n)] = np.nan
        return a
    raise KeyError(kind)


def _same(x, y):
    return x.dtype == y.dtype and (x == y or (np.isnan(x) and np.isnan(y)))       # zeros compare with ==: numpy leaves their sign open


def _check(a):
    from flexam_amd import conditioning_raster as P
    for q in (2, 98):
        want_s, want_a = np.percentile(a, q), np.percentile(a, [2, 98])[(2, 98).index(q)]
        assert want_s.dtype == np.float32 and want_a.dtype == np.float64
        for index in (R.ranks, P._percentile_index):
            got_s, got_a = R.percentile(a, q, True, index), R.percentile(a, q, False, index)
            assert _same(got_s, want_s), (a.shape, q, got_s, want_s)
            assert _same(got_a, want_a), (a.shape, q, got_a, want_a)


@pytest.mark.parametrize("kind", ("uniform", "ties", "one_exponent", "inverse_depth", "inf", "nan"))
def test_restatement_equals_numpy_percentile_bit_for_bit(kind):
    rng = np.random.default_rng(SIZES.index(1000) + len(kind))
    for n in SIZES:
        _check(_contents(kind, n, rng))


def test_restatement_on_a_whole_clip_and_on_2d_input():
    rng = np.random.default_rng(3)
    from flexam_amd import conditioning_raster as P
    _check(_contents("inverse_depth", 97 * 28672, rng).reshape(97, 28672))          # float32 rounds the index (n - 1) q here ...
    _check(_contents("ties", 51 * 7, rng).reshape(51, 7))
    big = _contents("uniform", 97 * 413124, rng)                                    # ... and n - 1 itself at the dense clip's size
    assert float(np.float32(big.size - 1)) != big.size - 1
    assert P._percentile_index(big.size, 98, True) == R.ranks(big.size, 98, True) != R.ranks(big.size, 98, False)
    assert _same(R.percentile(big, 98, True, P._percentile_index), np.percentile(big, 98))


def test_the_two_forms_differ():
    """What makes two arithmetics necessary: the scalar and the array form of one percentile are different numbers."""
    rng = np.random.default_rng(5)
    differ = 0
    for n in (50, 51, 1000, 28672, 413124, 97 * 28672):
        a = _contents("inverse_depth", n, rng)
        differ += sum(float(np.percentile(a, q)) != float(np.percentile(a, [q])[0]) for q in (2, 98))
    assert differ >= 6


def test_host_path_turns_nan_into_byte_zero():
    """NaN through the byte casts of the host colour tables gives 0 here; the device kernels write 0 by definition."""
    from flexam_amd import conditioning_raster as P
    nan = np.array([np.nan, 0.25, np.nan], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        assert (np.clip(nan, 0, 1) * 255).astype(np.uint8).tolist() == [0, 63, 0]
        code = np.stack([nan, nan, nan], -1)
        assert P._generate_colors_from_points(code, 3).tolist() == [[0, 0, 0], [159, 159, 159], [0, 0, 0]]
        pts = np.array([[np.nan, 4.0, 1.0], [4.0, np.nan, 2.0], [2.0, 2.0, 3.0]], dtype=np.float32)
        c = P._tracking_colors(pts, 8, 8)
        assert c[0, 0] == 0 and c[1, 1] == 0 and c[2, 0] == 63
        pts[1, 2] = np.nan                                                           # a NaN depth: both percentiles are NaN, every blue byte 0
        assert P._tracking_colors(pts, 8, 8)[:, 2].tolist() == [0, 0, 0]
        assert P._spectral_bytes(np.array([np.nan, 0.0])).tolist()[0] == [0, 0, 0]
