"""Generate tests/golden/metrics_ref.npz by running THE REFERENCE's own src/metrics.py (build container only; needs sklearn).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

/root/reference/src/metrics.py is loaded by path; its `from argus.metrics import Metric` (argus is absent here) is satisfied by a
placeholder module whose Metric is a bare class.  What the fixture pins is the reference's own classes - PerClassMetric.update
per step with CPU tensors, AveragePrecision / Accuracy.compute (sklearn's average_precision_score(average=None) and
accuracy_score), and epoch_complete on a stand-in state.  Only inputs and recorded results (data) are stored, case = <N>.<C>:

  pred.<case>, target.<case>         the epoch's rows, (N, C) fp32; the steps are rows [4 i, 4 i + 4) (`step`; a shorter last step)
  families.<case>                    the family of every column
  ap.<case>, acc.<case>              the two compute() results, float64 (C)
  keys.<case>.<phase>, values.<case>.<phase>   state.metrics after AveragePrecision's and then Accuracy's epoch_complete,
                                     phase in ("val", "train", ""): the keys in insertion order (the entry "none" is phase "")
  cases, step, threshold, classes

The generator asserts what the tests re-check from the fixture alone (tests/test_metrics.py)."""
import importlib.util
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_host  # noqa: E402

REF_FILE = "/root/reference/src/metrics.py"
SIZES = (1, 2, 3, 255, 256, 257, 513, 1000, 4099)
CLASSES = (2, 15)
LARGE_C_MAX_N = 1000          # the 15-class cases stop here: the fixture stays a few hundred KB
FAMILIES = ("cont", "ties", "sat", "corr", "allpos", "onepos", "nopos")
STEP = 4
THRESHOLD = 0.5
PHASES = ("val", "train", "")
NAMES = ["PASS", "DRIVE", "HEADER", "HIGH PASS", "OUT", "CROSS", "THROW IN", "SHOT", "BALL PLAYER BLOCK",
         "PLAYER SUCCESSFUL TACKLE", "FREE KICK", "GOAL", "Penalty", "Clearance", "Kick-off"]


def load_reference():
    argus = types.ModuleType("argus")
    argus_metrics = types.ModuleType("argus.metrics")
    argus_metrics.Metric = type("Metric", (), {})
    argus.metrics = argus_metrics
    sys.modules.setdefault("argus", argus)
    sys.modules.setdefault("argus.metrics", argus_metrics)
    spec = importlib.util.spec_from_file_location("ref_metrics", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def column(family, n, rng):
    """-> (fp32 scores (n), fp32 targets (n) of 0.0 / 1.0)"""
    t = (rng.random(n) < 0.3).astype(np.float32)
    z = 1.5 * rng.standard_normal(n)
    if family == "allpos":
        t[:] = 1.0
    elif family == "nopos":
        t[:] = 0.0
    elif family == "onepos":
        t[:] = 0.0
        t[rng.integers(n)] = 1.0
    if family == "corr":
        z = z + 2.0 * (2.0 * t - 1.0)
    s = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if family == "ties":
        s = (np.round(s * 8.0) / 8.0).astype(np.float32)
    if family == "sat":
        s[rng.random(n) < 0.5] = 1.0
    return s, t


def families_of(ci, C):
    return [FAMILIES[(2 * ci + c) % len(FAMILIES)] for c in range(C)] if C == 2 else [FAMILIES[c % len(FAMILIES)] for c in range(C)]


def mixed_tie_group(s, t):
    """a score shared by a positive and a negative row"""
    return bool(set(s[t == 1.0].tolist()) & set(s[t != 1.0].tolist()))


def main():
    ref = load_reference()
    rng = np.random.default_rng(20261020)
    d, cases, mixed = dict(step=np.array(STEP), threshold=np.array(THRESHOLD), classes=np.array(NAMES)), [], 0
    worst = 0.0
    for C in CLASSES:
        for ci, n in enumerate(SIZES):
            if C > 2 and n > LARGE_C_MAX_N:
                continue
            case = f"{n}.{C}"
            fams = families_of(ci, C)
            cols = [column(f, n, rng) for f in fams]
            pred = np.ascontiguousarray(np.stack([s for s, _ in cols], 1))
            target = np.ascontiguousarray(np.stack([t for _, t in cols], 1))
            if n == 257 and "corr" in fams:
                target[256, fams.index("corr")] = 1.0
            mixed += sum(f == "ties" and mixed_tie_group(pred[:, c], target[:, c]) for c, f in enumerate(fams))
            metrics = [ref.AveragePrecision(NAMES[:C]), ref.Accuracy(NAMES[:C], threshold=THRESHOLD)]
            for m in metrics:
                for r in range(0, n, STEP):
                    m.update(dict(prediction=torch.from_numpy(pred[r:r + STEP]), target=torch.from_numpy(target[r:r + STEP])))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")          # "No positive class found in y_true": the nopos columns
                ap = np.asarray(metrics[0].compute(), dtype=np.float64)
                acc = np.asarray(metrics[1].compute(), dtype=np.float64)
                for phase in PHASES:
                    state = types.SimpleNamespace(phase=phase, metrics={})
                    for m in metrics:
                        m.epoch_complete(state)
                    d[f"keys.{case}.{phase or 'none'}"] = np.array(list(state.metrics))
                    d[f"values.{case}.{phase or 'none'}"] = np.array([float(v) for v in state.metrics.values()], dtype=np.float64)
            assert ap.shape == acc.shape == (C,)
            d[f"pred.{case}"], d[f"target.{case}"], d[f"families.{case}"] = pred, target, np.array(fams)
            d[f"ap.{case}"], d[f"acc.{case}"] = ap, acc
            cases.append(case)
            # the host implementation against the recording
            hap, hp = metrics_host.average_precision(pred, target)
            assert np.array_equal(metrics_host.accuracy(pred, target, THRESHOLD).view(np.int64), acc.view(np.int64)), case
            err = np.abs(hap - ap).max()
            assert err <= metrics_host.ap_bound(n), (case, err, metrics_host.ap_bound(n))
            worst = max(worst, err / metrics_host.ap_bound(n))
            for c, f in enumerate(fams):
                if f == "nopos":
                    assert hp[c] == 0 and ap[c] == 0.0, (case, ap[c])
            if n == 257:
                assert (target[256] == 1.0).any()
    assert mixed >= 1, "no `ties` column with a tie group that holds a positive and a negative row"
    assert any("nopos" in d[f"families.{c}"].tolist() for c in cases)
    d["cases"] = np.array(cases)
    out = os.path.join(HERE, "metrics_ref.npz")
    np.savez_compressed(out, **d)
    print(len(cases), "cases,", os.path.getsize(out), "bytes, worst AP error / bound", worst)


if __name__ == "__main__":
    main()
