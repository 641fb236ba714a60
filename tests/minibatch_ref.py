"""The reference of macm_adv_moments and of the advantage normalisation of macm_ppo_grad_rows (include/macm.h),
in numpy float64, and the bound within which the device's moments must agree with it (a helper, not a test).

    moments(x, index, eps)  -> mean, rstd, std, n over the positions whose index is inside x
    normalise(adv, mean, rstd) -> (float32)(((float64)adv - mean) * rstd): the library's expression, operation
                                  for operation, so its bits are the device's

The sums here are math.fsum's: exact sums of the float64 terms, rounded once. The reference's own error is
then a handful of roundings whatever the row count, and the bound below is the device's.

The bound (u = 2^-53, n positions that count, first order in u as grad_ref.tol is):
* mean. The device adds n float64 terms in some fixed association: n - 1 additions, each of which rounds a
  partial sum that is at most sum |x_r| in magnitude, and the division rounds once more: n roundings, each
  at most u sum |x_r| / n = u mean|x|. The reference rounds twice (fsum, the division). So
      |mean_dev - mean_ref| <= (n + 2) u mean|x|.
* std. Each term d_r^2 = (x_r - m)^2 carries the subtraction's rounding twice (it is squared) and the
  square's once: 3 u d_r^2; the n - 1 additions of nonnegative terms add (n - 1) u S2; the division by n - 1
  and the square root round once each, and the root halves the relative error that S2 brings in:
  ((n + 2) / 2 + 2) u std for the device. The device's mean is off by some delta <= n u mean|x| from the
  exact mean of the data, which changes S2 by n delta^2 exactly (the first-order term is sum (x_r - mean) = 0):
  second order, below u S2 while n^2 u (mean|x| / std)^2 < 1, which holds with room for the tests' inputs
  (std of the order of |mean|, n < 2^18); one more u covers it. The reference: fsum, the same three roundings
  per term, the division and the root: 3.5 u std. So
      |std_dev - std_ref| <= (n / 2 + 8) u std.
* rstd = 1 / (std + eps): the addition and the division round once each on either side, and std's relative
  error carries over at most in full (eps >= 0):
      |rstd_dev - rstd_ref| <= (n / 2 + 12) u rstd.
With n = 1 the std is an exact 0 on both sides and rstd is 1 / eps exactly; the tests assert that outright."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -53


def gathered(x, index):
    """The float64 values that count: x[index[r]] for the positions whose index is inside x (index None: all)."""
    x = np.asarray(x, F32).reshape(-1)
    if index is None:
        return x.astype(F64)
    index = np.asarray(index, np.int64)
    return x[index[(index >= 0) & (index < x.size)]].astype(F64)


def moments(x, index=None, eps=1e-8):
    """dict(mean, rstd, std, n, mean_abs): macm_adv_moments' definition; mean_abs = mean |x_r| for the bound."""
    v = gathered(x, index)
    n = v.size
    mean = math.fsum(v) / n if n > 0 else 0.0
    s2 = math.fsum((v - mean) ** 2)  # the second pass, with the rounded mean
    var = s2 / (n - 1) if n > 1 else 0.0
    std = math.sqrt(var)
    return dict(mean=mean, rstd=1.0 / (std + eps), std=std, n=n, mean_abs=math.fsum(np.abs(v)) / n if n else 0.0)


def bounds(ref):
    """dict(mean, std, rstd): the largest |device - reference| the definition allows (the module docstring)."""
    n = ref["n"]
    return dict(mean=(n + 2) * U * ref["mean_abs"], std=(n / 2 + 8) * U * ref["std"],
                rstd=(n / 2 + 12) * U * ref["rstd"])


def normalise(adv, mean, rstd):
    """(float32)(((float64)adv - mean) * rstd): one subtraction, one multiplication, one rounding."""
    return ((np.asarray(adv, F32).astype(F64) - F64(mean)) * F64(rstd)).astype(F32)
