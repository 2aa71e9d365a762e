"""Gradient clipping restated in numpy (tt_grad_sumsq, tt_grad_clip_apply;
contract in include/tt.h): clipvalue, then clipnorm per variable or
global_clipnorm over all, in the order of Keras' legacy _transform_gradients.

A variable is a list of fp32 arrays (its regions' valid values).  Sums of
squares are math.fsum over the exact fp64 products (the correctly rounded
sum); the norm, the factor and the clipped values use the fp32 operations the
contract names."""
import math

import numpy as np

F32 = np.float32


def clamp(g: np.ndarray, clipvalue) -> np.ndarray:
    g = np.asarray(g, F32)
    if clipvalue is None:
        return g
    v = F32(clipvalue)
    return np.clip(g, -v, v)


def sumsq(arrays, clipvalue=None) -> float:
    """fsum of the exact fp64 squares of clamp(g) over a variable's arrays."""
    sq = [np.square(clamp(a, clipvalue).astype(np.float64)).ravel() for a in arrays]
    return math.fsum(np.concatenate(sq)) if sq else 0.0


def naive_sumsq(arrays, clipvalue=None) -> float:
    """The same sum as a plain double loop (an fp64 running sum)."""
    s = 0.0
    for a in arrays:
        for x in np.asarray(a, F32).ravel():
            if clipvalue is not None:
                x = min(max(x, -F32(clipvalue)), F32(clipvalue))
            s += float(x) * float(x)
    return s


def norm32(ss: float) -> np.float32:
    return F32(np.sqrt(np.float64(ss)))


def factor_of_norm(n: np.float32, c) -> np.float32:
    c = F32(c)
    return c / (n if not n <= c else c)  # one fp32 division; exactly 1 for n <= c


def factor(ss: float, c) -> np.float32:
    return factor_of_norm(norm32(ss), c)


def factor_candidates(ss: float, c):
    """The factors of n and of its two fp32 neighbours (the square root's
    rounding to fp32 may move one ulp)."""
    n = norm32(ss)
    return {factor_of_norm(m, c).tobytes() for m in (n, np.nextafter(n, F32(np.inf)), np.nextafter(n, F32(-np.inf)))}


def scaled(g: np.ndarray, clipvalue, f) -> np.ndarray:
    """fp32(clamp(g) * f), one fp32 multiply."""
    return clamp(g, clipvalue) * F32(f)


def clip(variables, clipvalue=None, clipnorm=None, global_clipnorm=None):
    """variables: list of lists of fp32 arrays.  Returns (ss per variable,
    factor per variable, clipped arrays in the same nesting)."""
    ss = [sumsq(v, clipvalue) for v in variables]
    if clipnorm is not None:
        fs = [factor(s, clipnorm) for s in ss]
    elif global_clipnorm is not None:
        total = math.fsum(np.concatenate([np.square(clamp(a, clipvalue).astype(np.float64)).ravel()
                                          for v in variables for a in v] or [np.zeros(0)]))
        fs = [factor(total, global_clipnorm)] * len(variables)
    else:
        fs = [F32(1.0)] * len(variables)
    out = [[scaled(a, clipvalue, f) for a in v] for v, f in zip(variables, fs)]
    return ss, fs, out
