"""Spotting on the device: per-frame probabilities -> spotted actions (``mds_spot``, include/mds.h).

The reference does this on the host: ``scripts/ball_action/predict.py::get_raw_predictions`` copies every frame's prediction to
the CPU, ``src/utils.py::post_processing`` runs ``scipy.ndimage.gaussian_filter`` and ``scipy.signal.find_peaks(height,
distance)`` once per class (``src/{ball_action,action}/annotations.py::raw_predictions_to_actions``), and
``scripts/ball_action/ensemble.py::load_and_blend_predictions`` averages the folds' raw predictions in float64 first.  Here

* ``PredictionTrack`` is the device-resident ``raw_predictions`` of one half (``StreamPredictor.predict_track`` fills it);
* ``Spotter`` turns one track (fp32 series, as predict.py) or a list of tracks (float64 blend, as ensemble.py) into
  ``(frame indexes, confidences)`` per class with ONE launch and ONE device-to-host copy;
* ``post_processing`` / ``raw_predictions_to_actions`` / ``blend`` keep the reference's signatures for numpy callers.

The header states the arithmetic; with the weights computed below (scipy's own formula, numpy float64) the results are the
reference's bit for bit.  One rule is this library's own: where two candidate peaks closer than ``distance`` have bit-equal
values, scipy's result depends on an unstable sort - here the lower row has priority.

No scipy import and no eager fallback: CPU tensors raise unless the test-suite's kernel simulator has been injected (``_lib``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import cabi


class PredictionTrack:
    """``raw_predictions`` of consecutive frames on the device: row j of the (capacity, num_classes) fp32 buffer ``data`` is the
    prediction for frame ``first_index + j``; ``count`` rows are filled.  The capacity is fixed: the buffer never moves."""

    def __init__(self, capacity: int, num_classes: int, device):
        if capacity < 1 or num_classes < 1:
            raise ValueError(f"PredictionTrack: capacity = {capacity}, num_classes = {num_classes}")
        self.data = torch.zeros(int(capacity), int(num_classes), dtype=torch.float32, device=device)
        self.first_index = 0
        self.count = 0

    @property
    def capacity(self):
        return self.data.shape[0]

    @property
    def num_classes(self):
        return self.data.shape[1]

    def rows(self):
        """the filled rows, on the device"""
        return self.data[:self.count]

    def numpy(self) -> np.ndarray:
        """the reference's ``raw_predictions`` (one device-to-host copy)"""
        return self.rows().cpu().numpy()

    def frame_indexes(self) -> np.ndarray:
        """the reference's ``frame_indexes``"""
        return np.arange(self.first_index, self.first_index + self.count)

    @classmethod
    def from_numpy(cls, frame_indexes, raw_predictions, device):
        """a saved ``np.savez(frame_indexes=..., raw_predictions=...)`` of predict.py: consecutive indexes, (n, C) float32"""
        fi = np.asarray(frame_indexes)
        raw = np.asarray(raw_predictions)
        if raw.ndim != 2 or raw.dtype != np.float32 or len(fi) != len(raw) or len(fi) < 1:
            raise ValueError("PredictionTrack.from_numpy: (n, C) float32 raw_predictions with n >= 1 frame indexes")
        if not np.array_equal(fi, np.arange(int(fi[0]), int(fi[0]) + len(fi))):
            raise ValueError("PredictionTrack.from_numpy: the frame indexes are not consecutive")
        t = cls(len(raw), raw.shape[1], device)
        t.data.copy_(torch.from_numpy(np.ascontiguousarray(raw)))
        t.first_index, t.count = int(fi[0]), len(raw)
        return t


def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """scipy.ndimage's kernel for ``gaussian_filter(x, sigma)``, its own formula in numpy float64"""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


class Spotter:
    """``post_processing`` of every class in one launch.  ``spotter(track)``: one ``PredictionTrack``, the fp32 series of
    predict.py (MDS_SPOT_SINGLE); ``spotter([track, ...])``: up to 16 tracks blended in float64 as ensemble.py does
    (MDS_SPOT_BLEND).  Returns, per class, ``(frame_indexes: list[int], confidences: list[float])``."""

    def __init__(self, gauss_sigma: float = 3.0, height: float = 0.2, distance: float = 15, truncate: float = 4.0):
        if not gauss_sigma > 0:
            raise ValueError(f"Spotter: gauss_sigma = {gauss_sigma} (> 0)")
        if not distance >= 1:
            raise ValueError(f"Spotter: distance = {distance} (>= 1, as scipy.signal.find_peaks)")
        self._set_weights(gaussian_weights(gauss_sigma, truncate))
        self.gauss_sigma, self.height, self.truncate = float(gauss_sigma), float(height), float(truncate)
        self.distance = int(math.ceil(distance))          # find_peaks: np.ceil(distance)
        self._lib = None          # tests inject the kernel simulator here
        self._dev = {}            # device -> weights, workspace and result buffers (they only grow)

    def _set_weights(self, w):
        self.weights = np.ascontiguousarray(w, dtype=np.float64)
        self.radius = (len(self.weights) - 1) // 2
        if self.radius > cabi.MDS_SPOT_MAX_RADIUS:
            raise ValueError(f"Spotter: kernel radius {self.radius} (truncate * sigma) above {cabi.MDS_SPOT_MAX_RADIUS}")

    def _library(self, x):
        if self._lib is not None:
            return self._lib
        if not x.is_cuda:
            raise cabi.MdsError("mds.spotting runs on MI355X only: keep the tracks on cuda")
        return cabi.load()

    def _buffers(self, dev, ws_bytes, out_bytes):
        b = self._dev.setdefault(dev, dict(ws=None, out=None))
        if "w" not in b:
            b["w"] = torch.from_numpy(self.weights).to(dev)
        if b["ws"] is None or b["ws"].numel() * 8 < ws_bytes:
            b["ws"] = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
        if b["out"] is None or b["out"].numel() * 8 < out_bytes:
            b["out"] = torch.empty((out_bytes + 7) // 8, dtype=torch.float64, device=dev)
        return b

    def _launch(self, tracks, single, want_smoothed, f64=False):
        """tracks: [(device tensor (n, C), first index)] -> (lo, N, C, cap, the result buffer on the device, smoothed or None)"""
        if not 1 <= len(tracks) <= cabi.MDS_SPOT_MAX_TRACKS:
            raise ValueError(f"Spotter: {len(tracks)} tracks (1 .. {cabi.MDS_SPOT_MAX_TRACKS})")
        x0 = tracks[0][0]
        dev, C = x0.device, x0.shape[1]
        for t, _ in tracks:
            if t.device != dev or t.dim() != 2 or t.shape[1] != C or t.shape[0] < 1 or not t.is_contiguous() \
                    or t.dtype != (torch.float64 if f64 else torch.float32):
                raise ValueError("Spotter: every track is a non-empty contiguous (n, C) buffer of one dtype on one device")
        lib = self._library(x0)
        lo = min(f for _, f in tracks)
        N = max(f + t.shape[0] for t, f in tracks) - lo          # (a gap inside is the launch's refusal)
        cap = max(1, (N - 3) // self.distance + 1 if N >= 3 else 1)      # MDS_SPOT_MAX_PEAKS(N, distance)
        conf_bytes, idx_bytes = C * cap * 8, C * cap * 4
        b = self._buffers(dev, cabi.MDS_SPOT_WS_BYTES * N * C, conf_bytes + idx_bytes + C * 4)
        out = b["out"]
        ints = out.view(torch.int32)
        conf = out[:C * cap]
        index = ints[2 * C * cap:3 * C * cap]
        count = ints[3 * C * cap:3 * C * cap + C]
        smoothed = torch.empty(N, C, dtype=torch.float32 if single else torch.float64, device=dev) if want_smoothed else None
        K = len(tracks)
        pad = [0] * (cabi.MDS_SPOT_MAX_TRACKS - K)
        args = cabi.make("mds_spot_args", mode=cabi.MDS_SPOT_SINGLE if single else cabi.MDS_SPOT_BLEND, K=K, C=C,
                         track=[t.data_ptr() for t, _ in tracks] + pad, track_f64=int(f64), first=[int(f) for _, f in tracks] + pad,
                         rows=[t.shape[0] for t, _ in tracks] + pad, weights=b["w"], radius=self.radius, distance=self.distance,
                         height=self.height, cap=cap, peak_index=index, peak_conf=conf, peak_count=count, smoothed=smoothed,
                         workspace=b["ws"], workspace_bytes=b["ws"].numel() * 8)
        args._keep.extend(t for t, _ in tracks)
        with torch.cuda.device(dev) if dev.type == "cuda" else _Null():
            lib.call("spot", args, torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
        return lo, N, C, cap, out[:(conf_bytes + idx_bytes + C * 4 + 7) // 8], smoothed

    @staticmethod
    def _as_tracks(track_or_tracks):
        single = isinstance(track_or_tracks, PredictionTrack)
        ts = [track_or_tracks] if single else list(track_or_tracks)
        for t in ts:
            if not isinstance(t, PredictionTrack) or t.count < 1:
                raise ValueError("Spotter: PredictionTrack(s) with at least one row")
        return [(t.rows(), t.first_index) for t in ts], single

    def _peaks(self, tracks, single, f64=False):
        lo, N, C, cap, out, _ = self._launch(tracks, single, False, f64)
        host = out.cpu().numpy()                                   # the one device-to-host copy
        conf = host[:C * cap].reshape(C, cap)
        ints = host.view(np.int32)
        index = ints[2 * C * cap:3 * C * cap].reshape(C, cap)
        count = ints[3 * C * cap:3 * C * cap + C]
        if (count > cap).any():
            raise cabi.MdsError(f"mds_spot kept {int(count.max())} peaks of one class, room for {cap}")
        return [((index[c, :count[c]].astype(np.int64) + lo).tolist(), conf[c, :count[c]].tolist()) for c in range(C)]

    @torch.no_grad()
    def __call__(self, track_or_tracks):
        tracks, single = self._as_tracks(track_or_tracks)
        return self._peaks(tracks, single)

    @torch.no_grad()
    def smoothed(self, track_or_tracks):
        """the smoothed series the peaks are taken from, (N, C) on the device: fp32 for one track, float64 for a list"""
        tracks, single = self._as_tracks(track_or_tracks)
        return self._launch(tracks, single, True)[5]


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def _identity_spotter(lib):
    s = Spotter(1.0, 0.0, 1)
    s._set_weights(np.ones(1))          # r = 0: y == x exactly
    s._lib = lib
    return s


@torch.no_grad()
def blend(tracks, _lib=None):
    """``load_and_blend_predictions`` of a list of tracks: (float64 (N, C) numpy array, frame indexes) - what ensemble.py saves"""
    ts, _ = Spotter._as_tracks(list(tracks))
    lo, N, _, _, _, sm = _identity_spotter(_lib)._launch(ts, False, True)
    return sm.cpu().numpy(), np.arange(lo, lo + N)


def _series_tracks(frame_indexes, predictions, device):
    """a numpy array or tensor (N,) / (N, C), fp32 or float64 -> ([(device tensor (N, C), first index)], single, f64)"""
    p = predictions if torch.is_tensor(predictions) else torch.from_numpy(np.ascontiguousarray(predictions))
    if p.dtype not in (torch.float32, torch.float64) or p.dim() not in (1, 2) or p.shape[0] < 1:
        raise ValueError("mds.spotting: predictions are fp32 or float64, (N,) or (N, C), N >= 1")
    if device is None:
        device = p.device if p.is_cuda else ("cuda" if torch.cuda.is_available() else "cpu")
    p = p.reshape(p.shape[0], -1).contiguous().to(device)
    f64 = p.dtype == torch.float64
    return [(p, int(frame_indexes[0]))], not f64, f64


def post_processing(frame_indexes, predictions, gauss_sigma, height, distance, device=None, _lib=None):
    """the reference's ``src/utils.py::post_processing`` for ONE class: ``predictions`` is a 1-D numpy array or tensor; fp32 input
    is smoothed as fp32 input is by scipy (MDS_SPOT_SINGLE), float64 input in float64 (MDS_SPOT_BLEND with one float64 track).
    Returns ``(action_frame_indexes, confidences)``."""
    s = Spotter(gauss_sigma, height, distance)
    s._lib = _lib
    tracks, single, f64 = _series_tracks(frame_indexes, predictions, device)
    return s._peaks(tracks, single, f64)[0]


def raw_predictions_to_actions(frame_indexes, raw_predictions, class2target, postprocess_params, device=None, _lib=None):
    """the reference's ``raw_predictions_to_actions`` with its two constants as arguments: ``{class: (frame indexes,
    confidences)}`` for ``class2target = {class: column}`` - one launch for all columns where the reference makes one pass per class"""
    s = Spotter(**postprocess_params)
    s._lib = _lib
    tracks, single, f64 = _series_tracks(frame_indexes, raw_predictions, device)
    per_class = s._peaks(tracks, single, f64)
    return {cls: per_class[col] for cls, col in class2target.items()}
