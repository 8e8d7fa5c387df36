"""Host (numpy) implementation of mds_spot's normative arithmetic, written from the rules in include/mds.h - blend, smoothing,
peaks, height, distance - and of the gaussian weights the Python side computes.  It is the expected value of the kernel tests
where neither the reference nor scipy exists; tests/test_spotting.py holds IT to the reference's recorded results
(tests/golden/spotting_ref.npz) and, where scipy imports, to scipy itself.

numpy evaluates `a * b`, `a + b`, `a / b` on float64 arrays element by element with one IEEE rounding each: the expressions below
are the header's, operation for operation."""
import numpy as np


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, r): 2r + 1 float64 weights, r = int(truncate * sigma + 0.5)"""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def reflect(i, n):
    """R: d c b a | a b c d | d c b a, period 2n"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def blend(tracks, firsts):
    """tracks: fp32 (n_k, C) arrays whose row 0 is frame firsts[k] -> (float64 (N, C), lo); a frame a track does not cover is
    skipped, K stays the divisor.  Raises ValueError when the union of the ranges is not contiguous."""
    lo = min(firsts)
    hi = max(f + len(t) for f, t in zip(firsts, tracks))
    covered = np.zeros(hi - lo, dtype=bool)
    x = np.zeros((hi - lo, tracks[0].shape[1]), dtype=np.float64)
    for f, t in zip(firsts, tracks):
        covered[f - lo:f - lo + len(t)] = True
        x[f - lo:f - lo + len(t)] = x[f - lo:f - lo + len(t)] + t.astype(np.float64)
    if not covered.all():
        raise ValueError("the union of the tracks' ranges is not contiguous")
    return x / float(len(tracks)), lo


def smooth(x, w, single):
    """x: float64 (N,) or (N, C); w: the 2r + 1 weights.  single: the result is rounded once to fp32 (and returned as fp32)"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, r = x.shape[0], (len(w) - 1) // 2
    l = np.arange(n)
    acc = x[l] * w[r]
    for j in range(r, 0, -1):
        acc = acc + (x[reflect(l - j, n)] + x[reflect(l + j, n)]) * w[r - j]
    return acc.astype(np.float32) if single else acc


def local_maxima(y):
    """rise, plateau, fall -> (left + right) // 2; rows 0 and N - 1 never, a plateau that touches an edge never"""
    y = np.asarray(y, dtype=np.float64)
    n, out, i = len(y), [], 1
    while i < n - 1:
        if y[i - 1] < y[i]:
            j = i + 1
            while j < n - 1 and y[j] == y[i]:
                j += 1
            if y[j] < y[i]:
                out.append((i + j - 1) // 2)
                i = j
        i += 1
    return np.array(out, dtype=np.int64)


def select_by_distance(peaks, prio, distance):
    """highest priority first, among equal values the lower row first; a visited peak that is alive is kept and removes every
    other peak closer than `distance`"""
    keep = np.ones(len(peaks), dtype=bool)
    for j in sorted(range(len(peaks)), key=lambda k: (-prio[k], peaks[k])):
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and peaks[j] - peaks[k] < distance:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < len(peaks) and peaks[k] - peaks[j] < distance:
            keep[k] = False
            k += 1
    return keep


def candidates(y, height):
    """the peaks that pass `height` (before the distance rule) and their values as float64"""
    yd = np.asarray(y, dtype=np.float64)
    p = local_maxima(yd)
    p = p[height <= yd[p]] if len(p) else p
    return p, yd[p]


def find_peaks(y, height, distance):
    """y: the smoothed series of ONE class (fp32 or float64) -> (rows int64, confidences float64)"""
    p, v = candidates(y, height)
    keep = select_by_distance(p, v, distance)
    return p[keep], v[keep]


def spot(x, w, height, distance, single):
    """one class, from the (blended) series: (smoothed, rows, confidences)"""
    y = smooth(x, w, single)
    p, v = find_peaks(y, height, distance)
    return y, p, v


def has_tie(y, height, distance):
    """two candidate peaks that pass `height`, lie closer than `distance` and have bit-equal values: the one case in which
    scipy's result depends on an unstable sort"""
    p, v = candidates(y, height)
    for i in range(len(p)):
        k = i + 1
        while k < len(p) and p[k] - p[i] < distance:
            if v[k] == v[i]:
                return True
            k += 1
    return False
