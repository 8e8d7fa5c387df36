"""Developer tool: the epoch metrics on the device (mds.metrics) against the reference's route on the host (src/metrics.py).

Both metrics the train scripts install (AveragePrecision, Accuracy) at N = 6,000 / C = 2 and N = 36,000 / C = 15, steps of 4 rows:
(a) ms per step of `update` for both metrics: mds = two launches, nothing comes back (host clock over all steps of the epoch,
    then one synchronise, divided by the steps; and the device time of the same steps between two events); reference = the four
    `.cpu().numpy()` copies of the (4, C) step output and two list appends.  Nothing else runs on the stream here: in a training
    step each of the reference's copies also waits for everything queued before it, which this tool does not show.
(b) ms per `compute` of both metrics: mds = two launches and one device-to-host copy each (events | host clock); reference =
    np.concatenate of the epoch's lists + sklearn's average_precision_score(average=None) and accuracy_score per class, where
    sklearn imports.  The first call of each side is compared: accuracy bit for bit, AP within 2 (N + 8) 2^-53.

    python tools/metrics_ab.py [--reps 5]        (prints and writes profiles/metrics_ab.txt)
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ball-action-spotting_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import metrics_host as mh
from mds import metrics

STEP = 4
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def make_epoch(N, C, dev, g):
    """scores correlated with 0 / 1 labels, 10 % positives: every tile holds positives, the kernel walks all of them"""
    t = (torch.rand(N, C, generator=g) < 0.1).float()
    s = torch.sigmoid(1.5 * torch.randn(N, C, generator=g) + 2.0 * (2.0 * t - 1.0))
    return s.to(dev), t.to(dev)


def reference_update(lists, pred, target):
    for preds, targets in lists:          # PerClassMetric.update, once per installed metric
        preds.append(pred.cpu().numpy())
        targets.append(target.cpu().numpy())


def reference_compute(lists, threshold, sk):
    (p0, t0), (p1, t1) = lists
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap = sk.average_precision_score(np.concatenate(t0, axis=0), np.concatenate(p0, axis=0), average=None)
    targets, predictions = np.concatenate(t1, axis=0), np.concatenate(p1, axis=0)
    y_true, y_pred = targets > threshold, predictions > threshold
    return ap, [sk.accuracy_score(y_true[:, c], y_pred[:, c]) for c in range(y_true.shape[1])]


def timed_device(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def spread(v, fmt="{:.3f}"):
    return f"{fmt.format(statistics.median(v))} ms  [{fmt.format(min(v))} - {fmt.format(max(v))}]"


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=5)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_ab.txt"))
    args = ap_.parse_args()
    assert torch.cuda.is_available(), "metrics_ab measures on the MI355X"
    try:
        import sklearn.metrics as sk
    except ImportError:
        sk = None
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    say(f"AveragePrecision + Accuracy(threshold 0.5), steps of {STEP} rows; median [min - max] of {args.reps} epochs")
    say("reference = src/metrics.py's route on the host" + ("" if sk else " - sklearn does not import here: its compute was NOT measured"))
    for N, C in ((6000, 2), (36000, 15)):
        names = [f"c{c}" for c in range(C)]
        s, t = make_epoch(N, C, dev, g)
        steps = [dict(prediction=s[r:r + STEP], target=t[r:r + STEP]) for r in range(0, N, STEP)]
        ms = [metrics.AveragePrecision(names), metrics.Accuracy(names, threshold=0.5)]
        upd_host, upd_dev, cmp_dev, cmp_host, ref_upd, ref_cmp = [], [], [], [], [], []
        same = None
        for rep in range(args.reps + 1):          # epoch 0 warms up (buffers grow, code objects load) and checks parity
            for m in ms:
                m.reset()
            torch.cuda.synchronize()

            def epoch():
                for out in steps:
                    for m in ms:
                        m.update(out)
            ev, host, _ = timed_device(epoch)
            got = timed_device(lambda: (ms[0].compute(), ms[1].compute()))
            lists = [([], []), ([], [])]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for out in steps:
                reference_update(lists, out["prediction"], out["target"])
            r_upd = (time.perf_counter() - t0) * 1e3
            r_cmp = None
            if sk:
                t0 = time.perf_counter()
                want = reference_compute(lists, 0.5, sk)
                r_cmp = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                if sk:
                    same = (float(np.abs(got[2][0] - want[0]).max()), got[2][1] == [float(v) for v in want[1]])
                continue
            upd_host.append(host / len(steps))
            upd_dev.append(ev / len(steps))
            cmp_dev.append(got[0])
            cmp_host.append(got[1])
            ref_upd.append(r_upd / len(steps))
            if sk:
                ref_cmp.append(r_cmp)
        say()
        say(f"N = {N}, C = {C} ({len(steps)} steps, {int(ms[0]._evaluate()[2].sum())} positive (row, class) pairs)")
        if same is not None:
            say(f"  parity with sklearn: max |dAP| = {same[0]:.2e} (bound {mh.ap_bound(N):.2e}), accuracy bit-equal: {same[1]}")
        say(f"  update, per step   mds        host clock {spread(upd_host, '{:.4f}')}   device {spread(upd_dev, '{:.4f}')}")
        say(f"                     reference  host clock {spread(ref_upd, '{:.4f}')}")
        say(f"  compute            mds        device {spread(cmp_dev)}   host clock {spread(cmp_host)}")
        if sk:
            say(f"                     reference  host clock {spread(ref_cmp, '{:.1f}')}")
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
