"""Generate tests/golden/spotting_ref.npz by running THE REFERENCE's own src/utils.py::post_processing (build container only;
needs scipy).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spotting.py

/root/reference/src/utils.py is loaded by path; its `import cv2` (absent here, and unused by post_processing) is satisfied by
an empty placeholder module.  What the fixture pins is the reference's own function - scipy.ndimage.gaussian_filter, then
scipy.signal.find_peaks(height, distance) - executed on the series below.  Only inputs, settings and recorded results (data) are
stored:

  series.<family>.<N>.<dtype>            the input series
  weights.<sigma>                        scipy's own kernel for that sigma, as gaussian_filter1d uses it
  smoothed.<family>.<N>.<dtype>.<sigma>  gaussian_filter's output
  peaks.<case>.idx / .conf               post_processing's two lists (frame_indexes[0] = 0), case = <family>.<N>.<dtype>.<param set>
  params                                 the parameter sets (gauss_sigma, height, distance)
  cases                                  the case names

The blend cases (3 and 14 tracks with different first frames) are recorded from a numpy restatement of
scripts/ball_action/ensemble.py::load_and_blend_predictions, lines 28-33 (np.unique of the concatenated indexes, zeros,
`blend[frame_indexes] += prediction` per track, `/= len`, cut at the first index, and the assert of line 34) - the function
itself imports the `src` package and cannot be loaded alone.  Each blended class column then goes through post_processing.

No binary box inputs: they give bit-equal peaks, whose order under scipy's unstable sort is unspecified.  The generator
refuses (asserts) a case in which two candidate peaks that pass `height`, closer than `distance`, have bit-equal values.
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spotting_host  # noqa: E402

REF_FILE = "/root/reference/src/utils.py"
SIZES = (1, 2, 3, 12, 13, 25, 26, 97, 1000, 4500)
PARAMS = np.array([[3.0, 0.2, 15], [1.0, 0.5, 1], [3.0, 0.0, 40]])
FAMILIES = ("noise", "bumps", "flat", "const", "edge_l", "edge_r")
LARGE = 4500          # first parameter set only; 1000 and 4500 rows only for noise, bumps and const (the other families' plateaus
                      # fit into 97 rows): the fixture stays a few hundred KB
BLEND_CLASSES = 2


def load_reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_utils", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def series(family, n, rng):
    i = np.arange(n)
    if family == "noise":        # sigmoid of noise on a slow wave
        return 1.0 / (1.0 + np.exp(-(3.0 * rng.standard_normal(n) + 2.5 * np.sin(i / 37.0) - 0.5)))
    if family == "bumps":        # sparse bumps, each with its own amplitude
        x = np.zeros(n)
        for c in rng.choice(n, size=max(1, n // 23), replace=False):
            a, s = rng.uniform(0.15, 1.0), rng.uniform(1.0, 4.0)
            x = np.maximum(x, a * np.exp(-0.5 * ((i - c) / s) ** 2))
        return x
    if family == "flat":         # a saturated run of exact 1.0, longer than 2r + 1
        x = 0.05 + 0.1 * rng.random(n)
        x[n // 3:n // 3 + 41] = 1.0
        return x
    if family == "const":
        return np.full(n, 0.625)
    x = 0.1 + 0.2 * rng.random(n)      # a plateau of the series' maximum that touches an edge
    if family == "edge_l":
        x[:min(n, 45)] = 0.9
    else:
        x[max(0, n - 45):] = 0.9
    return x


def blend_restated(frame_indexes_lst, prediction_lst, num_classes):
    frame_indexes = np.unique(np.concatenate(frame_indexes_lst))                    # ensemble.py:28
    blend_prediction = np.zeros((np.max(frame_indexes) + 1, num_classes))          # :29
    for fi, prediction in zip(frame_indexes_lst, prediction_lst):                   # :30-31
        blend_prediction[fi] += prediction
    blend_prediction /= len(prediction_lst)                                         # :32
    blend_prediction = blend_prediction[np.min(frame_indexes):]                     # :33
    assert blend_prediction.shape[0] == frame_indexes.shape[0]                      # :34
    return blend_prediction, frame_indexes


def main():
    from scipy.ndimage import _filters
    ref = load_reference()
    rng = np.random.default_rng(20261020)
    d, cases = dict(params=PARAMS), []
    for sigma in sorted(set(PARAMS[:, 0])):
        r = int(4.0 * sigma + 0.5)
        d[f"weights.{sigma}"] = _filters._gaussian_kernel1d(sigma, 0, r)[::-1].copy()
        assert np.array_equal(d[f"weights.{sigma}"], spotting_host.gaussian_weights(sigma))

    def record(case, x, sigma, height, distance, smoothed_key):
        y = ref.gaussian_filter(x, sigma)
        assert not spotting_host.has_tie(y, height, distance), f"{case}: bit-equal candidate peaks within distance - change the seed"
        idx, conf = ref.post_processing([0], x, sigma, height, int(distance))
        d[smoothed_key] = y
        d[f"peaks.{case}.idx"] = np.array(idx, dtype=np.int64)
        d[f"peaks.{case}.conf"] = np.array(conf, dtype=np.float64)      # .tolist() of fp32 values: exact in float64
        cases.append(case)

    for family in FAMILIES:
        for n in SIZES:
            if n >= 1000 and family not in ("noise", "bumps", "const"):
                continue
            x64 = series(family, n, rng)
            for dt in ("f32", "f64"):
                x = x64.astype(np.float32) if dt == "f32" else x64
                d[f"series.{family}.{n}.{dt}"] = x
                for pi, (sigma, height, distance) in enumerate(PARAMS):
                    if n == LARGE and pi > 0:
                        continue
                    record(f"{family}.{n}.{dt}.{pi}", x, sigma, height, distance, f"smoothed.{family}.{n}.{dt}.{sigma}")

    # blend: K tracks of (n_k, C) fp32 with different first frames whose union is contiguous
    for bi, (K, n) in enumerate(((3, 300), (14, 320))):
        firsts = [int(v) for v in rng.integers(5, 60, size=K)]
        firsts[0] = 7
        lens = [int(n - f - rng.integers(0, 40)) for f in firsts]
        lens[1] = n - firsts[1]
        tracks = [np.stack([series("noise", m, rng), series("bumps", m, rng)], 1).astype(np.float32) for m in lens]
        x, fi = blend_restated([np.arange(f, f + m) for f, m in zip(firsts, lens)], tracks, BLEND_CLASSES)
        d[f"blend.{bi}.first"], d[f"blend.{bi}.rows"] = np.array(firsts), np.array(lens)
        for k, t in enumerate(tracks):
            d[f"blend.{bi}.track.{k}"] = t
        d[f"blend.{bi}.x"], d[f"blend.{bi}.frame_indexes"] = x, fi
        sigma, height, distance = PARAMS[0]
        for c in range(BLEND_CLASSES):
            y = ref.gaussian_filter(x[:, c], sigma)
            assert not spotting_host.has_tie(y, height, distance)
            idx, conf = ref.post_processing(fi.tolist(), x[:, c], sigma, height, int(distance))
            d[f"blend.{bi}.smoothed.{c}"] = y
            d[f"blend.{bi}.idx.{c}"], d[f"blend.{bi}.conf.{c}"] = np.array(idx, dtype=np.int64), np.array(conf, dtype=np.float64)
    d["cases"] = np.array(cases)
    out = os.path.join(HERE, "spotting_ref.npz")
    np.savez_compressed(out, **d)
    print(len(cases), "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
