"""Epoch metrics on the device: per-class average precision and binary accuracy (``mds_metric_push`` / ``mds_metric_eval``,
include/mds.h).

The reference's ``src/metrics.py::PerClassMetric.update`` copies every step's prediction and target to the host
(``.cpu().numpy()``, twice per metric: four blocking copies per iteration with the two metrics the train scripts install) and
``compute`` concatenates the epoch's list of arrays and calls sklearn once per metric.  Here

* ``update`` is ONE launch on the prediction's current stream that appends the step's rows to epoch buffers on the device - no
  synchronisation, no host copy; the row count is kept on the host from the tensor shapes;
* ``compute`` is ONE launch and ONE device-to-host copy;
* ``AveragePrecision`` / ``Accuracy`` keep the reference's names, constructor signatures, ``name`` / ``better`` attributes,
  ``target2class`` and ``epoch_complete(state)``, which writes ``state.metrics`` exactly as the reference does.

The header states the arithmetic: accuracy equals sklearn's ``accuracy_score`` bit for bit, average precision equals
``average_precision_score`` within 2 (N + 8) 2^-53.  ``compute`` raises ``ValueError`` where the reference does: no rows,
targets that are neither 0 nor 1 (AveragePrecision only - sklearn's "continuous format is not supported", e.g. mixup's soft
targets), scores that are not finite.  Ranks are not combined: the reference has no distributed metrics.

Base class: ``argus.metrics.Metric`` where argus imports; otherwise a local stand-in with the hooks ``epoch_start`` -> ``reset``,
``iteration_complete`` -> ``update(state.step_output)`` and ``epoch_complete``.  argus's hook names are written from memory and are
not pinned by anything in this repository.

No sklearn import and no eager fallback: CPU tensors raise unless the test-suite's kernel simulator has been injected (``_lib``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import cabi

try:
    from argus.metrics import Metric
except ImportError:
    class Metric:
        """stand-in for argus.metrics.Metric: the three hooks a training engine calls"""
        name: str = ''
        better: str = 'min'

        def reset(self):
            pass

        def update(self, step_output: dict):
            pass

        def compute(self):
            pass

        def epoch_start(self, state):
            self.reset()

        def iteration_complete(self, state):
            self.update(state.step_output)

        def epoch_complete(self, state):
            pass


_DTYPES = {torch.float32: cabi.MDS_F32, torch.bfloat16: cabi.MDS_BF16}


class PerClassMetric(Metric):
    name: str = ''
    better: str = 'min'
    _what = 0

    def __init__(self, classes: list[str], capacity: int = 4096):
        if int(capacity) < 1:
            raise ValueError(f"{type(self).__name__}: capacity = {capacity} (>= 1)")
        self.target2class = {trg: cls for trg, cls in enumerate(classes)}
        self.threshold = 0.5
        self._capacity0 = int(capacity)
        self._lib = None          # tests inject the kernel simulator here
        self._count = 0
        self._pred = self._target = self._status = self._result = self._ws = None

    @property
    def num_classes(self):
        return len(self.target2class)

    @property
    def count(self):
        """rows pushed since the last reset (kept on the host)"""
        return self._count

    def reset(self):
        """keeps the buffers; the count goes to zero on the host, `status` by a fill on the current stream"""
        self._count = 0
        if self._status is not None:
            self._status.zero_()

    def _library(self, x):
        if self._lib is not None:
            return self._lib
        if not x.is_cuda:
            raise ValueError(f"{type(self).__name__} runs on MI355X only: keep the step output on cuda")
        return cabi.load()

    def _reserve(self, rows, dev):
        C = self.num_classes
        if self._pred is None or self._pred.device != dev:
            if self._count:
                raise ValueError(f"{type(self).__name__}: the step output moved from {self._pred.device} to {dev} inside an epoch")
            self._pred = self._target = None
            self._status = torch.zeros(2, dtype=torch.int32, device=dev)
            self._result = torch.empty(3 * C + 2, dtype=torch.float64, device=dev)
            self._ws = None
        cap = self._capacity0 if self._pred is None else self._pred.shape[0]
        while cap < rows:
            cap *= 2
        if self._pred is None or cap > self._pred.shape[0]:
            pred = torch.empty(cap, C, dtype=torch.float32, device=dev)
            target = torch.empty(cap, C, dtype=torch.float32, device=dev)
            if self._count:          # growth: device-to-device, ordered on the current stream
                pred[:self._count].copy_(self._pred[:self._count])
                target[:self._count].copy_(self._target[:self._count])
            self._pred, self._target = pred, target

    @staticmethod
    def _stream(dev):
        return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0

    @torch.no_grad()
    def update(self, step_output: dict):
        pred, target = step_output['prediction'], step_output['target']
        C = self.num_classes
        if not (torch.is_tensor(pred) and torch.is_tensor(target)):
            raise ValueError(f"{type(self).__name__}.update: 'prediction' and 'target' are tensors")
        if pred.dim() != 2 or pred.shape[1] != C or pred.shape[0] < 1 or target.shape != pred.shape:
            raise ValueError(f"{type(self).__name__}.update: prediction {tuple(pred.shape)} and target {tuple(target.shape)}, "
                             f"both (B, {C}) with B >= 1 are expected")
        if pred.device != target.device or pred.dtype not in _DTYPES:
            raise ValueError(f"{type(self).__name__}.update: fp32 or bf16 predictions and their targets on one device")
        lib = self._library(pred)
        dev = pred.device
        with torch.cuda.device(dev) if dev.type == "cuda" else _Null():
            B = pred.shape[0]
            self._reserve(self._count + B, dev)
            args = cabi.make("mds_metric_push_args", dtype=_DTYPES[pred.dtype], B=B, C=C, pred=pred.contiguous(),
                             target=target.to(torch.float32).contiguous(), dst_pred=self._pred, dst_target=self._target,
                             row=self._count, capacity=self._pred.shape[0], status=self._status)
            lib.call("metric_push", args, self._stream(dev))
        self._count += B

    @torch.no_grad()
    def _evaluate(self):
        """-> (AP (C), accuracy (C), P (C)) as float64 arrays: one launch, one device-to-host copy"""
        who = type(self).__name__
        if self._count < 1:
            raise ValueError(f"{who}.compute: no rows since the last reset")          # (the reference: np.concatenate of an empty list)
        dev, N, C = self._pred.device, self._count, self.num_classes
        lib = self._library(self._pred)
        need = cabi.MDS_METRIC_WS_BYTES * (-(-N // cabi.MDS_METRIC_TILE)) * C
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        args = cabi.make("mds_metric_eval_args", what=self._what, C=C, N=N, pred=self._pred, target=self._target,
                         threshold=float(np.float32(self.threshold)), status=self._status, result=self._result,
                         workspace=self._ws, workspace_bytes=self._ws.numel() * 8)
        with torch.cuda.device(dev) if dev.type == "cuda" else _Null():
            lib.call("metric_eval", args, self._stream(dev))
            host = self._result.cpu().numpy()                                   # the one device-to-host copy
        soft, wild = int(host[3 * C]), int(host[3 * C + 1])
        if wild:
            raise ValueError(f"{who}.compute: {wild} predictions are not finite")          # sklearn: "Input contains NaN" / "infinity"
        if soft and self._what & cabi.MDS_METRIC_AP:
            raise ValueError(f"{who}.compute: {soft} targets are neither 0 nor 1: continuous format is not supported")
        return host[:C].copy(), host[C:2 * C].copy(), host[2 * C:3 * C].copy()

    def compute(self) -> list[float]:
        raise NotImplementedError

    def epoch_complete(self, state):
        scores = self.compute()
        name_prefix = f"{state.phase}_" if state.phase else ''
        state.metrics[f"{name_prefix}{self.name}"] = np.mean(scores)
        for trg, cls in self.target2class.items():
            state.metrics[f"{name_prefix}{self.name}_{cls.lower()}"] = scores[trg]


class AveragePrecision(PerClassMetric):
    name = 'average_precision'
    better = 'max'
    _what = cabi.MDS_METRIC_AP

    def compute(self) -> np.ndarray:
        """float64 (C,), as sklearn's average_precision_score(average=None); 0.0 for a class without a positive row"""
        return self._evaluate()[0]


class Accuracy(PerClassMetric):
    name = 'binary_accuracy'
    better = 'max'
    _what = cabi.MDS_METRIC_ACC

    def __init__(self, classes: list[str], threshold: float = 0.5, capacity: int = 4096):
        super().__init__(classes, capacity)
        self.threshold = threshold

    def compute(self) -> list[float]:
        return self._evaluate()[1].tolist()


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False
