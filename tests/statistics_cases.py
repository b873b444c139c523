"""The yardstick of the running field statistics: the recurrences of csrc/stats_kernels.hip restated in NumPy, elementwise, in the
kernel's operation order, every operation rounded on its own (NumPy never fuses), the divisor np.float64(n).  Host only.

    n == 1:  mean = x;  m2 = 0;  min = x;  max = x
    n  > 1:  d = x - mean;  mean = mean + d / n;  m2 = m2 + d * (x - mean);  min = x < min ? x : min;  max = x > max ? x : max
"""
import numpy as np

QUANTITIES = ('mean', 'm2', 'min', 'max')


def welford(samples):
    """{'count', 'mean', 'm2', 'min', 'max', 'var'} of a sequence of equally shaped float64 arrays, by the device's recurrences."""
    mean = m2 = mn = mx = None
    n = 0
    for x in samples:
        x = np.asarray(x, dtype=np.float64)
        n += 1
        if n == 1:
            mean, m2, mn, mx = x.copy(), np.zeros_like(x), x.copy(), x.copy()
            continue
        d = x - mean
        mean = mean + d / np.float64(n)
        m2 = m2 + d * (x - mean)
        mn = np.where(x < mn, x, mn)
        mx = np.where(x > mx, x, mx)
    if n == 0:
        raise ValueError("welford: no samples")
    return {'count': n, 'mean': mean, 'm2': m2, 'min': mn, 'max': mx, 'var': m2 / n}


def rank(expect, every, arm_step, after):
    """Rank n (1, 2, ...) of the record of the step that takes the count to `expect` (csrc/api_stats.inc: stats_rank), or None
    where that step is not recorded: not a multiple of the stride, not above `after`, or not committed after arming."""
    a = max(arm_step, after)
    if expect % every != 0 or expect <= a:
        return None
    return expect // every - a // every


def recorded_steps(first, last, every, arm_step, after):
    """The steps of first..last that are recorded, by the three conditions themselves."""
    return [s for s in range(first, last + 1) if s % every == 0 and s > after and s > arm_step]
