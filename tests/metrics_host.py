"""Host (numpy) implementation of mds_metric_push's and mds_metric_eval's normative arithmetic, written from the rules in
include/mds.h.  It is the bit-level expected value of the kernel tests; tests/test_metrics.py holds IT to the reference's recorded
results (tests/golden/metrics_ref.npz: the reference's own classes on sklearn) and, where sklearn imports, to sklearn itself.

numpy compares float32 arrays as fp32 and evaluates `a / b`, `a + b` on float64 scalars with one IEEE rounding each: the
expressions below are the header's, operation for operation."""
import numpy as np

TILE = 256          # MDS_METRIC_TILE


def ap_bound(n):
    """|AP(header) - AP(sklearn)| <= 2 (N + 8) 2^-53.  The header's form: at most P + 1 <= N + 1 roundings (the quotients q_j, the
    sums, the final division) of non-negative terms whose exact sum is at most 1 - absolute error <= (N + 2) 2^-53.  sklearn: one
    rounded precision and one rounded recall per threshold (at most N), their differences and a sum - <= (N + 10) 2^-53."""
    return 2.0 * (n + 8) * 2.0 ** -53


def push(dst_pred, dst_target, status, row, pred, target):
    """one step: pred (B, C) fp32 (a bf16 tensor widened by the caller: exact), target (B, C) fp32 -> rows [row, row + B) of the two
    (capacity, C) fp32 epoch buffers; status[0] += targets that are neither 0.0 nor 1.0, status[1] += scores that are not finite"""
    pred = np.asarray(pred, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    b = pred.shape[0]
    assert 0 <= row and row + b <= dst_pred.shape[0]
    dst_pred[row:row + b] = pred
    dst_target[row:row + b] = target
    status[0] += int(np.count_nonzero(~((target == np.float32(0.0)) | (target == np.float32(1.0)))))
    status[1] += int(np.count_nonzero(~np.isfinite(pred)))


def average_precision_1(s, t):
    """one class: fp32 scores s (N), fp32 targets t (N) -> (AP as a Python float (an IEEE double), P)"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    pos = np.asarray(t, dtype=np.float32) == np.float32(1.0)
    n_rows = len(s)
    total = 0.0
    for k0 in range(0, n_rows, TILE):
        rows = k0 + np.flatnonzero(pos[k0:k0 + TILE])          # the tile's positive rows, ascending
        S = 0.0
        if len(rows):
            ge = s[None, :] >= s[rows][:, None]                # fp32 compares; False where a NaN takes part
            n = ge.sum(1)
            tp = (ge & pos[None, :]).sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                q = tp.astype(np.float64) / n.astype(np.float64)
            for v in q.tolist():
                S = S + v
        total = total + S
    P = int(pos.sum())
    return (total / float(P) if P else 0.0), P


def average_precision(pred, target):
    """(N, C) fp32, (N, C) fp32 -> (float64 (C), int64 (C)): AP and P per class"""
    pred, target = np.asarray(pred), np.asarray(target)
    out = [average_precision_1(pred[:, c], target[:, c]) for c in range(pred.shape[1])]
    return np.array([a for a, _ in out], dtype=np.float64), np.array([p for _, p in out], dtype=np.int64)


def accuracy(pred, target, threshold=0.5):
    """(N, C) fp32 twice -> float64 (C): hits / N with hit = ((t > thr) == (s > thr)), thr rounded to fp32"""
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    thr = np.float32(threshold)
    hits = ((target > thr) == (pred > thr)).sum(0)
    return hits.astype(np.float64) / np.float64(pred.shape[0])
