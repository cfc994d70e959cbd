"""The bound shared by the probe-lookup tests (tests/test_probe_lookup_cpu.py, tests/test_gpu_probe_lookup.py); the statement itself is
api.probe_lookup (include/firework_hip.h).

lookup_bound(ref, T, wrap): per channel
    |gpu - ref| <= 2^-24 |ref| + c 2^-53 T,        T = sum over corners and k of |w B_k sh|   (api.probe_lookup(..., terms=True))
The device and numpy evaluate the same float64 expression operation for operation.  + - * / floor min max are correctly rounded on both
sides, so from equal inputs they give equal bits: the cell (i, f) and the trilinear weights are bit-equal.  The two sides can first part
at a square root — the device library's may differ from numpy's by a few float64 ulps; S = 4 is taken for "a few" — and from there
every later operation can add one more rounding's worth (2^-53 relative) of difference.  c counts them along the longest chain into one
term w B_k sh of the sum and through the sum:

  the normal     nh = n / sqrt(...):                                       S + 1
  B_k            the longest basis chain is Y6 = C (3 (z z) - 1): z z carries 2 (S + 1) + 1, then three more operations, then the
                 band factor A_k:                                          2 S + 7
  the wrap       h = 0.5 ((nh . rh) + 1) with rh = r / sqrt(...): two square roots, two divisions, one product, two additions and the
                 + 1; every value on the way is at most 1 in magnitude, so h is off by at most (2 S + 6) 2^-53 absolutely (the
                 multiplication by 0.5 is exact).  fac = h h + 0.2 moves by 2 h dh plus its own two roundings; relative to fac that is
                 dh * 2 h / (h h + 0.2) <= dh / sqrt(0.2) < 2.24 dh:           ceil(2.24 (2 S + 6)) + 2
                 w fac:                                                    + 1     (the numerator, N)
                 the sum of up to 8 non-negative numerators: a weighted mean of their errors plus 7 additions:   N + 7
                 w / sum:                                                  N + (N + 7) + 1
  the sums       B_k sh: 1;  the 8 additions of e (each at most 2^-53 of a partial sum, which T bounds): 8;  w e: 1;  the 8 additions
                 of E (the first one to 0 is exact, counted all the same): 8
  float32        the device's one rounding is 2^-24 of ITS float64 value, which is within the terms above of ref: one more count
                 covers the product of the two.

  without wrap   c = (2 S + 7) + 1 + 8 + 1 + 8 + 1 = 34
  with wrap      N = ceil(2.24 x 14) + 2 + 1 = 35;  c = (35 + 42 + 1) + 34 = 112

Nothing here is measured on the GPU: ref and T come from the test's own inputs.

What the count relies on.  Y6 = C (3 (z z) - 1) and Y8 = C (x x - y y) subtract: where they cancel, a normal nh that differed between
the two sides would move B_6 and B_8 by up to that difference times C (3 z z + 1) and C (x x + y y), which |B_k| — and so T, which is
taken with |B_k| as the header states it — does not bound.  nh differs only if the two sides' sqrt of the same float64 differ.  IEEE 754
asks a correctly rounded square root and numpy's is one.  If the device's float64 sqrt is correctly rounded as well, nh, every B_k and
the trilinear weights are bit-equal on both sides, and S only enters through the wrap's weights, where nothing cancels (fac >= 0.2):
the bound then holds as derived.  A device sqrt that was merely "a few ulps" off would keep it everywhere except within a few ulps'
relative distance of the zeros of Y6 and Y8, and there the bound relies on the correct rounding."""
import math

import numpy as np

S = 4       # "a few" float64 ulps between two square roots


def rounding_count(wrap: bool) -> int:
    sums = (2 * S + 7) + 1 + 8 + 1 + 8 + 1
    if not wrap:
        return sums
    n = math.ceil(2.24 * (2 * S + 6)) + 2 + 1
    return n + (n + 7) + 1 + sums


assert rounding_count(False) == 34 and rounding_count(True) == 112


def lookup_bound(ref, T, wrap: bool) -> np.ndarray:
    """the bound above for a float64 reference ref (N, 3) and its T (N, 3)"""
    return 2.0 ** -24 * np.abs(np.asarray(ref, np.float64)) + rounding_count(wrap) * 2.0 ** -53 * np.asarray(T, np.float64)
