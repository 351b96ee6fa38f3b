"""Float64 restatement of the spherical interpolation between behaviour codes (lib/utils.py:920-925), what
``vunet_seq_slerp`` (csrc/seq_interp.hip) is held to -- as tests/pose_angles_ref.py is for the kinematics kernels.

Everything the result is sensitive to is machine independent: the three sums are exactly rounded (``math.fsum`` of the
float64 products), the scalar functions are the C library's (``math``), and the blend is one float64 multiply-add chain per
element without fusing.  tests/golden/make_golden_behavior_interp.py wrote the fixture's float64 column with this same
arithmetic; tests/test_behavior_interp_golden.py holds this file to that column bit for bit and to the reference's own
float32-path output within the distance the fixture recorded between the two.
"""
import math

import numpy as np

DEFAULT_STEPS = np.linspace(0, 1, 6)


def slerp_coefficients(val, low, high):
    """(c_lo, c_hi) of slerp(val, low, high) in float64.  A row of zeros makes 0 / 0: NaN coefficients, as numpy gives."""
    a, b = np.asarray(low, dtype=np.float64).reshape(-1), np.asarray(high, dtype=np.float64).reshape(-1)
    aa, bb, ab = math.fsum(a * a), math.fsum(b * b), math.fsum(a * b)
    den = math.sqrt(aa) * math.sqrt(bb)
    c = ab / den if den != 0.0 else float("nan")
    c = -1.0 if c < -1.0 else (1.0 if c > 1.0 else c)        # (comparisons pass a NaN on, as np.clip does)
    omega = math.acos(c) if c == c else float("nan")
    so = math.sin(omega)
    v = float(val)
    if so == 0.0:
        return 1.0 - v, v
    return math.sin((1.0 - v) * omega) / so, math.sin(v * omega) / so


def slerp(val, low, high):
    """slerp(val, low, high) -> float64 [H]."""
    c_lo, c_hi = slerp_coefficients(val, low, high)
    return c_lo * np.asarray(low, dtype=np.float64) + c_hi * np.asarray(high, dtype=np.float64)


def slerp_codes(b1, b2, steps=None):
    """[P, H] x [P, H] -> (out float64 [2, P, S, H], bound float64 [2, P, S, H]): out[0, p, s] = slerp(steps[s], b1[p], b2[p]),
    out[1, p, s] = slerp(steps[s], b2[p], b1[p]); bound = |c_lo low| + |c_hi high|, the magnitude a rounding of the result is
    relative to."""
    steps = DEFAULT_STEPS if steps is None else np.asarray(steps, dtype=np.float64)
    b1, b2 = np.asarray(b1, dtype=np.float64), np.asarray(b2, dtype=np.float64)
    out = np.empty((2, b1.shape[0], len(steps), b1.shape[1]))
    mag = np.empty_like(out)
    for d, (lo, hi) in enumerate(((b1, b2), (b2, b1))):
        for p in range(b1.shape[0]):
            for s, v in enumerate(steps):
                c_lo, c_hi = slerp_coefficients(v, lo[p], hi[p])
                out[d, p, s] = c_lo * lo[p] + c_hi * hi[p]
                mag[d, p, s] = np.abs(c_lo * lo[p]) + np.abs(c_hi * hi[p])
    return out, mag
