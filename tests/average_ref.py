"""Host reference of the weight-averaging kernels (csrc/average.hip) in numpy float64: the warm-up rule, the float64 value
of an update with its rounding bound, the per-model squared distance and the weighted mean."""
from fractions import Fraction

import numpy as np

EPS32 = 2.0 ** -24          # unit roundoff of fp32


def decay_used(decay, n, warmup=True):
    """The decay of update number n (n updates applied before it): min(decay, (1 + n) / (10 + n)) with warm-up.  The quotient is
    the correctly rounded double (Fraction -> float rounds once), as an IEEE division gives it."""
    decay = float(decay)
    return min(decay, float(Fraction(1 + n, 10 + n))) if warmup else decay


def warmup_sequence(decay, count, warmup=True):
    return [decay_used(decay, n, warmup) for n in range(count)]


def om_of(d):
    """(float)(1.0 - d) as a double."""
    return float(np.float32(1.0 - float(d)))


def ema_expected(p, e, d):
    """E = e + om (p - e) in float64 of the stored fp32 operands, and the bound of the rule's two roundings (the rounded
    difference, the fma's one rounding): 2^-24 (|om| |p - e| + |E|) (1 + 2^-20)."""
    p64, e64, om = p.astype(np.float64), e.astype(np.float64), om_of(d)
    E = e64 + om * (p64 - e64)
    bound = EPS32 * (abs(om) * np.abs(p64 - e64) + np.abs(E)) * (1.0 + 2.0 ** -20)
    return E, bound


def dist2(p, e_new, offs):
    """Per model sum ((double)p - (double)e_new)^2 (numpy's float64 sum) and the element counts."""
    d = (p.astype(np.float64) - e_new.astype(np.float64)) ** 2
    return ([float(np.sum(d[offs[m]:offs[m + 1]])) for m in range(len(offs) - 1)],
            [int(offs[m + 1] - offs[m]) for m in range(len(offs) - 1)])


def mean64(srcs, weights):
    """sum_k weights[k] (double)src_k in float64, in source order."""
    acc = np.zeros(srcs[0].shape, np.float64)
    for w, s in zip(weights, srcs):
        acc = acc + float(w) * s.astype(np.float64)
    return acc


def ulp32(x):
    """The fp32 unit in the last place at |x| (float64 array in, float64 out)."""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
