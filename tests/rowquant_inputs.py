"""Float32 matrices that put a symmetric int8 quantizer (scale = amax / 127, codes = round_half_even(x / scale)) on its edges, one
case per ROW.  The row quantizers take them as they are (tests/test_gpu_parity.py), the column quantizer transposed
(tests/test_colquant_exact_gpu.py), so both see the same values."""
import numpy as np


def ties_and_near_ties() -> np.ndarray:
    """[10][1280]: rows in which MANY quotients x / scale are exact rounding ties (k + 0.5 -> half to even) or sit one ulp beside one;
    scale = amax / 127 = 1, 2, 0.5, 1.5, 3."""
    rng = np.random.default_rng(7)
    rows = []
    for amax in (127.0, 254.0, 63.5, 190.5, 381.0):
        s = amax / 127.0
        halves = (rng.integers(-126, 126, size=1280) + 0.5) * s  # exact ties in f32
        halves[0] = amax
        rows.append(halves)
        near = halves.copy().astype(np.float32)
        near[1:] = np.nextafter(near[1:], np.float32(np.inf) * np.sign(rng.standard_normal(1279)).astype(np.float32))  # one ulp off a tie
        rows.append(near)
    return np.stack(rows).astype(np.float32)


def exponent_range() -> np.ndarray:
    """[207][1536]: rows spanning the whole exponent range -- both sides of the 2^+-60 guard of RowDiv (sdnq_dev.h), subnormal-scale
    rows, scales whose significand is all ones (the one case where RN(1 / s) is too coarse), ties and near-ties at every magnitude."""
    rng = np.random.default_rng(11)
    k = 1536
    rows = []
    for e in list(range(-120, 121, 4)) + [-126, -61, -60, -59, 59, 60, 61, 120]:
        base = rng.standard_normal(k).astype(np.float32) * np.float32(0.3)
        base[0] = 1.0
        rows.append(np.ldexp(base, e).astype(np.float32))
        # scale with an all-ones significand: amax = 127 * (2 - 2^-23) * 2^e
        s = np.ldexp(np.float32(2.0) - np.float32(2.0 ** -23), e)
        r = (rng.integers(-126, 127, size=k) + rng.choice([0.0, 0.5], size=k)).astype(np.float64) * np.float64(s)
        r[0] = 127.0 * np.float64(s)
        rows.append(r.astype(np.float32))
        # ties / near ties around an ordinary scale at this magnitude
        s2 = np.ldexp(np.float32(1.25), e)
        t = ((rng.integers(-126, 126, size=k) + 0.5).astype(np.float64) * np.float64(s2)).astype(np.float32)
        t[1::2] = np.nextafter(t[1::2], np.float32(np.inf))
        t[0] = np.float32(127.0) * s2
        rows.append(t)
    return np.stack(rows)
