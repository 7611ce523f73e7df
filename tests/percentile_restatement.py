"""np.percentile(a, q) of float32 data restated as sort + index + interpolation, with the roundings numpy 2.x applies (method 'linear':
`_QuantileMethods['linear']`, `_get_indexes`, `_get_gamma`, `_lerp` in numpy/lib/_function_base_impl.py; the linear method's virtual
index is `(n - 1) * quantiles`, not `_compute_virtual_index`, which only the other methods go through).  numpy evaluates the two call
forms the colour tables use in DIFFERENT precisions:

  scalar q   np.percentile(a, 2)          quantile = 2 / float32(100); the virtual index (n - 1) q, the weight and the
                                          interpolation are float32 (n - 1 itself is rounded to float32 above 2^24); result float32
  array q    np.percentile(a, [2, 98])    quantile = 2 / 100 in float64; index and weight float64; the difference of the two
                                          neighbours is float32, the interpolation float64; result float64

Any NaN gives NaN; an index at or past n - 1 takes the last element for both neighbours (weight = index + 1, which then multiplies
a zero difference -- or inf - inf = NaN, as numpy)."""
import numpy as np


def ranks(n: int, q, scalar_form: bool):
    """(lower rank, upper rank, weight) for n values."""
    F = np.float32 if scalar_form else np.float64
    quantile = F(q) / F(100)
    virtual = F(n - 1) * quantile
    previous = np.floor(virtual)
    lo, hi = int(previous), int(previous + F(1))               # `previous_indexes + 1` in the index's precision: above 2^24 it can stay put
    if virtual >= n - 1:
        lo = hi = -1
    if virtual < 0:
        lo = hi = 0
    gamma = F(np.float64(virtual) - np.float64(lo))
    return lo % max(n, 1), hi % max(n, 1), gamma


def lerp(lower, upper, gamma, scalar_form: bool):
    lower, upper = np.float32(lower), np.float32(upper)
    with np.errstate(invalid="ignore", over="ignore"):
        d = upper - lower
        if scalar_form:
            g = np.float32(gamma)
            return upper - d * (np.float32(1) - g) if g >= np.float32(0.5) else lower + d * g
        g, d = np.float64(gamma), np.float64(d)
        return np.float64(upper) - d * (np.float64(1) - g) if g >= 0.5 else np.float64(lower) + d * g


def percentile(a, q, scalar_form: bool, index=ranks):
    """np.percentile(a, q) (scalar_form) / np.percentile(a, [q])[0] of float32 `a`, flattened."""
    s = np.sort(np.asarray(a, dtype=np.float32).ravel())
    if np.isnan(s[-1]):
        return np.float32(np.nan) if scalar_form else np.float64(np.nan)
    lo, hi, gamma = index(s.size, q, scalar_form)
    return lerp(s[lo], s[hi], gamma, scalar_form)
