"""mds_metric_push / mds_metric_eval (csrc/k_metric.hip) and mds.metrics.

  1. the header's constants and prototypes;
  2. tests/metrics_host.py (numpy, written from the header's rules) against the reference's own classes as recorded in
     tests/golden/metrics_ref.npz (make_golden_metrics.py), the fixture's preconditions, and sklearn itself where it imports;
  3. mds_metric_push and 4. mds_metric_eval on the simulator and on the GPU, every buffer guarded, refusals included;
  5. the Python API against the recording;  6. GPU only: no synchronisation in update, identical bytes from two compute() calls.

Accuracy, P and the kernel-against-host comparisons are exact (== on bits).  Average precision against sklearn holds within the
DERIVED bound 2 (N + 8) 2^-53 (metrics_host.ap_bound): the header's form makes at most N + 1 roundings of non-negative terms whose
exact sum is at most 1, sklearn's at most N + 10 - neither figure is fitted to results."""
import types

import numpy as np
import pytest
import torch

import metrics_host as mh
from backends import be, be_gpu  # noqa: F401
from mds import cabi, metrics

SIZES = (1, 2, 3, 255, 256, 257, 513, 1000, 4099)
FAMILIES = ("cont", "ties", "sat", "corr", "allpos", "onepos", "nopos")
CASES = [f"{n}.2" for n in SIZES] + [f"{n}.15" for n in SIZES if n <= 1000]
AP, ACC = cabi.MDS_METRIC_AP, cabi.MDS_METRIC_ACC
BAD = cabi.MDS_ERR_BAD_ARG
FILL = -7.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same(got, want, msg):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{msg}: {bad.size} of {got.size} values differ in their bits, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


def assert_within(got, want, n, msg):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    assert np.all(err <= mh.ap_bound(n)), f"{msg}: |dAP| = {err.max():.3e} above 2 (N + 8) 2^-53 = {mh.ap_bound(n):.3e}"


def draw(rng, n, family):
    """fresh data of one family: fp32 scores, fp32 0 / 1 targets"""
    t = (rng.random(n) < 0.3).astype(np.float32)
    if family == "allpos":
        t[:] = 1.0
    elif family in ("nopos", "onepos"):
        t[:] = 0.0
        if family == "onepos":
            t[rng.integers(n)] = 1.0
    z = 1.5 * rng.standard_normal(n) + (2.0 * (2.0 * t - 1.0) if family == "corr" else 0.0)
    s = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if family == "ties":
        s = (np.round(s * 8.0) / 8.0).astype(np.float32)
    if family == "sat":
        s[rng.random(n) < 0.5] = 1.0
    return s, t


def draw_case(seed, n, C):
    rng = np.random.default_rng(seed)
    cols = [draw(rng, n, FAMILIES[(seed + c) % len(FAMILIES)]) for c in range(C)]
    return np.ascontiguousarray(np.stack([s for s, _ in cols], 1)), np.ascontiguousarray(np.stack([t for _, t in cols], 1))


@pytest.fixture(scope="module")
def ref(golden):
    return golden("metrics_ref")


@pytest.fixture(scope="module")
def host(ref):
    """the host implementation on every fixture case, computed once: case -> (AP, P, accuracy)"""
    out = {}
    for case in ref["cases"].tolist():
        ap, p = mh.average_precision(ref[f"pred.{case}"], ref[f"target.{case}"])
        out[case] = (ap, p, mh.accuracy(ref[f"pred.{case}"], ref[f"target.{case}"], float(ref["threshold"])))
    return out


# ================================================================================================ 1. the header
def test_header_constants():
    assert cabi.MDS_VERSION >= 142 and cabi.MDS_METRIC_TILE == 256 == mh.TILE
    assert (AP, ACC) == (1, 2) and cabi.MDS_METRIC_WS_BYTES == 16
    assert ("mds_metric_push", "const mds_metric_push_args* a, mds_stream_t stream") in cabi.LONG_FUNCS
    assert ("mds_metric_eval", "const mds_metric_eval_args* a, mds_stream_t stream") in cabi.LONG_FUNCS


# ================================================================================================ 2. host against the fixture
def test_fixture_preconditions(ref):
    cases = ref["cases"].tolist()
    assert cases == CASES and int(ref["step"]) == 4 and float(ref["threshold"]) == 0.5
    mixed, nopos, seen = 0, 0, set()
    for case in cases:
        n, C = map(int, case.split("."))
        pred, target, fams = ref[f"pred.{case}"], ref[f"target.{case}"], ref[f"families.{case}"].tolist()
        assert pred.shape == target.shape == (n, C) and pred.dtype == target.dtype == np.float32 and len(fams) == C
        assert np.isin(target, (0.0, 1.0)).all() and np.isfinite(pred).all()
        seen |= set(fams)
        for c, f in enumerate(fams):
            s, t = pred[:, c], target[:, c]
            if f == "ties":
                mixed += bool(set(s[t == 1.0].tolist()) & set(s[t != 1.0].tolist()))
            if f == "sat" and n >= 255:
                assert 0.3 < (s == 1.0).mean() < 0.7
            if f == "nopos":
                nopos += 1
                assert not t.any() and ref[f"ap.{case}"][c] == 0.0
            if f == "allpos":
                assert t.all() and abs(ref[f"ap.{case}"][c] - 1.0) <= mh.ap_bound(n)          # (sklearn's own sum: 1 - 2^-53 in places)
        if n == 257:
            assert (target[256] == 1.0).any()          # a positive row alone in the last tile
    assert seen == set(FAMILIES) and mixed >= 1 and nopos >= 1


def test_host_reproduces_the_recorded_reference(ref, host):
    for case in CASES:
        n = int(case.split(".")[0])
        ap, p, acc = host[case]
        assert_same(acc, ref[f"acc.{case}"], case + " accuracy")
        assert_within(ap, ref[f"ap.{case}"], n, case + " AP")
        assert np.array_equal(p, (ref[f"target.{case}"] == 1.0).sum(0))


def test_host_against_sklearn_directly():
    sk = pytest.importorskip("sklearn.metrics")
    import warnings
    for seed, n in enumerate((1, 2, 5, 255, 256, 257, 700)):
        pred, target = draw_case(seed, n, 7)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # the column without a positive row
            want = sk.average_precision_score(target, pred, average=None)
        ap, _ = mh.average_precision(pred, target)
        assert_within(ap, want, n, f"n = {n}")
        for thr in (0.5, 0.3):
            want = [sk.accuracy_score(target[:, c] > thr, pred[:, c] > thr) for c in range(7)]
            assert_same(mh.accuracy(pred, target, thr), want, f"accuracy n = {n}")


# ================================================================================================ 3. mds_metric_push
def push(be, pred, target, dst_pred, dst_target, status, row, fields=None):
    B, C = pred.shape
    kw = dict(dtype=cabi.MDS_BF16 if pred.dtype == torch.bfloat16 else cabi.MDS_F32, B=B, C=C, pred=pred, target=target,
              dst_pred=dst_pred, dst_target=dst_target, row=row, capacity=dst_pred.shape[0], status=status)
    kw.update(fields or {})
    rc = be.rc("metric_push", cabi.make("mds_metric_push_args", **kw))
    be.sync()
    return rc


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_push_writes_its_rows_and_nothing_else(be, dt):
    rng = np.random.default_rng(3)
    cap = 11
    for C in (1, 2, 15, 17):
        for B in (1, 4, 5):
            for row in (0, 3, cap - B):          # at row 0, in the middle, ending exactly at `capacity`
                p = torch.from_numpy(rng.random((B, C)).astype(np.float32)).to(dt)
                t = (rng.random((B, C)) < 0.5).astype(np.float32)
                dp = be.out((cap, C), fill=FILL, name="dst_pred")
                dtg = be.out((cap, C), fill=FILL, name="dst_target")
                status = be.out((2,), torch.int32, fill=0, name="status")
                assert push(be, be.t(p, name="pred"), be.t(t, name="target"), dp, dtg, status, row) == 0
                want_p, want_t = np.full((cap, C), FILL, np.float32), np.full((cap, C), FILL, np.float32)
                st = np.zeros(2, np.int64)
                mh.push(want_p, want_t, st, row, p.float().numpy(), t)
                assert np.array_equal(dp.cpu().numpy(), want_p) and np.array_equal(dtg.cpu().numpy(), want_t), (C, B, row)
                assert status.cpu().tolist() == [0, 0] == st.tolist()


def test_push_counts_what_compute_must_refuse(be):
    p = np.full((5, 3), 0.25, np.float32)
    t = np.zeros((5, 3), np.float32)
    p[0, 1], p[4, 2] = np.nan, -np.inf
    t[1, 0], t[2, 2], t[3, 1] = 0.3, -0.0, 1.0
    dp, dtg = be.out((8, 3), fill=FILL), be.out((8, 3), fill=FILL)
    status = be.out((2,), torch.int32, fill=5, name="status")          # the launch ADDS
    assert push(be, be.t(p), be.t(t), dp, dtg, status, 2) == 0
    assert status.cpu().tolist() == [6, 7]          # 0.3 | NaN and -inf; -0.0 == 0.0 does not count
    st = np.array([5, 5])
    mh.push(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32), st, 2, p, t)
    assert st.tolist() == [6, 7]
    got = dp.cpu().numpy()[2:7]
    assert np.array_equal(got.view(np.int32), p.view(np.int32)) and np.signbit(dtg.cpu().numpy()[4, 2])
    assert push(be, be.t(p), be.t(t), dp, dtg, status, 3) == 0          # a second step accumulates
    assert status.cpu().tolist() == [7, 9]


def test_push_refusals_launch_nothing(be):
    p, t = np.full((4, 2), 0.5, np.float32), np.ones((4, 2), np.float32)
    be.reset_launches()

    def refused(row=0, **fields):
        dp, dtg = be.out((8, 2), fill=FILL), be.out((8, 2), fill=FILL)
        status = be.out((2,), torch.int32, fill=0)
        assert push(be, be.t(p), be.t(t), dp, dtg, status, row, fields) == BAD, fields
        assert (dp == FILL).all() and (dtg == FILL).all() and status.cpu().tolist() == [0, 0]
    refused(B=0)
    refused(C=0)
    refused(row=-1)
    refused(row=5)          # row + B > capacity
    refused(capacity=3)
    refused(dtype=2)
    for field in ("pred", "target", "dst_pred", "dst_target", "status"):
        refused(**{field: None})
    rec = be.launches()
    assert rec is None or rec == []


# ================================================================================================ 4. mds_metric_eval
def evaluate(be, pred, target, what=AP | ACC, threshold=0.5, status=(0, 0), fields=None):
    """one launch over (N, C) rows -> dict(rc, result (3 C + 2) as numpy).  Every buffer is guarded, the workspace is NaN."""
    N, C = pred.shape
    need = cabi.MDS_METRIC_WS_BYTES * (-(-N // cabi.MDS_METRIC_TILE)) * C
    st = be.t(torch.tensor(status, dtype=torch.int32), name="status")
    result = be.out((3 * C + 2,), torch.float64, fill=FILL, name="result")
    ws = be.out((need // 8,), torch.float64, fill=float("nan"), name="workspace")
    kw = dict(what=what, C=C, N=N, pred=be.t(pred, name="pred"), target=be.t(target, name="target"),
              threshold=float(np.float32(threshold)), status=st, result=result, workspace=ws, workspace_bytes=need)
    kw.update(fields or {})
    rc = be.rc("metric_eval", cabi.make("mds_metric_eval_args", **kw))
    be.sync()
    return dict(rc=rc, result=result.cpu().numpy())


def assert_result(out, C, ap=None, acc=None, p=None, status=(0, 0), msg=""):
    """a part that is None must have kept its fill"""
    r = out["result"]
    assert out["rc"] == 0, msg
    for part, want in ((r[:C], ap), (r[C:2 * C], acc), (r[2 * C:3 * C], p)):
        if want is None:
            assert (part == FILL).all(), msg + ": a part that was not asked for was written"
        else:
            assert_same(part, want, msg)
    assert r[3 * C:].tolist() == [float(status[0]), float(status[1])]


@pytest.mark.parametrize("case", CASES)
def test_eval_reproduces_the_recorded_reference(be, ref, host, case):
    n, C = map(int, case.split("."))
    ap, p, acc = host[case]
    out = evaluate(be, ref[f"pred.{case}"], ref[f"target.{case}"], status=(0, 0))
    assert_result(out, C, ap, acc, p, msg=case)
    assert_same(out["result"][C:2 * C], ref[f"acc.{case}"], case + " accuracy against the recording")
    assert_within(out["result"][:C], ref[f"ap.{case}"], n, case + " AP against the recording")


@pytest.mark.parametrize("n,C", [(300, 1), (257, 17), (5, 17)])
def test_eval_other_class_counts_against_the_host(be, n, C):
    pred, target = draw_case(n + C, n, C)
    ap, p = mh.average_precision(pred, target)
    for thr in (0.5, 0.3):
        out = evaluate(be, pred, target, threshold=thr, status=(3, 0))
        assert_result(out, C, ap, mh.accuracy(pred, target, thr), p, status=(3, 0), msg=f"{n} x {C}, threshold {thr}")


def test_eval_writes_only_what_it_is_asked_for(be, ref, host):
    case = "513.2"
    ap, p, acc = host[case]
    pred, target = ref[f"pred.{case}"], ref[f"target.{case}"]
    be.reset_launches()
    assert_result(evaluate(be, pred, target, what=AP, status=(0, 4)), 2, ap, None, p, status=(0, 4), msg="AP alone")
    assert_result(evaluate(be, pred, target, what=ACC, status=(9, 0)), 2, None, acc, None, status=(9, 0), msg="accuracy alone")
    assert_result(evaluate(be, pred, target, what=AP | ACC), 2, ap, acc, p, msg="both")
    rec = be.launches("metric")
    if rec is not None:          # the simulator's launch record: two kernels per call, one block per (tile, class), then per class
        assert [(l.gx, l.gy, l.bx) for l in rec] == [(3, 2, 256), (2, 1, 256)] * 3


def test_eval_soft_targets_are_no_positives(be):
    """mixup's soft targets: only t == 1.0f is a positive row; accuracy compares t with the threshold"""
    pred, target = draw_case(1, 40, 2)
    soft = target.copy()
    soft[::3] = 0.7
    ap, p = mh.average_precision(pred, soft)
    assert (p < (target == 1.0).sum(0)).any()
    assert_result(evaluate(be, pred, soft), 2, ap, mh.accuracy(pred, soft), p, msg="soft targets")


def test_eval_refusals_launch_nothing(be):
    pred, target = draw_case(2, 300, 2)
    need = cabi.MDS_METRIC_WS_BYTES * 2 * 2
    be.reset_launches()

    def refused(**fields):
        out = evaluate(be, pred, target, fields=fields)
        assert out["rc"] == BAD, fields
        assert (out["result"] == FILL).all()
    refused(N=0)
    refused(C=0)
    refused(N=1 << 30, C=2)          # N x C >= 2^31
    refused(N=1 << 31, C=1)
    refused(what=0)
    refused(what=4)
    for field in ("pred", "target", "status", "result", "workspace"):
        refused(**{field: None})
    refused(workspace_bytes=need - 1)
    rec = be.launches()
    assert rec is None or rec == []
    assert evaluate(be, pred, target, fields=dict(workspace_bytes=need))["rc"] == 0


# ================================================================================================ 5. the Python API
def make_metrics(be, C, ref, **kw):
    names = ref["classes"].tolist()[:C]
    ms = [metrics.AveragePrecision(names, **kw), metrics.Accuracy(names, threshold=float(ref["threshold"]), **kw)]
    for m in ms:
        m._lib = be.lib if be.name == "emu" else None
    return ms


def replay(ms, pred, target, step, dev):
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
    for m in ms:
        for r in range(0, len(pred), step):
            m.update(dict(prediction=p[r:r + step], target=t[r:r + step]))


@pytest.mark.parametrize("case", CASES)
def test_api_replays_the_recorded_epoch(be, ref, host, case):
    n, C = map(int, case.split("."))
    pred, target = ref[f"pred.{case}"], ref[f"target.{case}"]
    ms = make_metrics(be, C, ref, capacity=8)
    assert [m.name for m in ms] == ["average_precision", "binary_accuracy"] and all(m.better == "max" for m in ms)
    assert ms[0].target2class == dict(enumerate(ref["classes"].tolist()[:C]))
    for epoch in range(2):          # reset and a second epoch give the same answer
        for m in ms:
            m.reset()
        replay(ms, pred, target, int(ref["step"]), be.device)
        assert all(m.count == n for m in ms)
        ap, acc = ms[0].compute(), ms[1].compute()
        assert isinstance(ap, np.ndarray) and ap.dtype == np.float64 and ap.shape == (C,)
        assert isinstance(acc, list) and len(acc) == C and all(type(v) is float for v in acc)
        assert_same(ap, host[case][0], f"{case} AP, epoch {epoch}")
        assert_within(ap, ref[f"ap.{case}"], n, case)
        assert_same(acc, ref[f"acc.{case}"], f"{case} accuracy, epoch {epoch}")
        for phase in ("val", "train", ""):
            state = types.SimpleNamespace(phase=phase, metrics={})
            for m in ms:
                m.epoch_complete(state)
            keys, values = ref[f"keys.{case}.{phase or 'none'}"].tolist(), ref[f"values.{case}.{phase or 'none'}"]
            assert list(state.metrics) == keys
            for key, want in zip(keys, values):
                if "binary_accuracy" in key:
                    assert_same(state.metrics[key], want, key)
                else:
                    assert_within(state.metrics[key], want, n, key)
    if n > 8:          # the buffers doubled from 8 rows, at least twice where the epoch is longer than 16
        assert ms[0]._pred.shape[0] >= n and ms[0]._pred.shape[0] % 8 == 0 and (n <= 16 or ms[0]._pred.shape[0] >= 32)


def test_api_default_capacity_and_bf16(be, ref):
    ms = make_metrics(be, 2, ref)
    rng = np.random.default_rng(9)
    p = torch.from_numpy(rng.random((6, 2)).astype(np.float32)).to(torch.bfloat16)
    t = torch.from_numpy((rng.random((6, 2)) < 0.5).astype(np.float32))
    for m in ms:
        m.update(dict(prediction=p.to(be.device), target=t.to(be.device)))
        assert m._pred.shape == (4096, 2)
    ap, _ = mh.average_precision(p.float().numpy(), t.numpy())
    assert_same(ms[0].compute(), ap, "bf16 predictions")
    assert_same(ms[1].compute(), mh.accuracy(p.float().numpy(), t.numpy()), "bf16 predictions")


def test_api_raises_where_the_reference_does(be, ref):
    dev = be.device
    ap, acc = make_metrics(be, 2, ref, capacity=8)
    for m in (ap, acc):
        with pytest.raises(ValueError, match="no rows"):
            m.compute()
    good = dict(prediction=torch.full((4, 2), 0.25, device=dev), target=torch.ones(4, 2, device=dev))
    soft = dict(prediction=torch.full((4, 2), 0.25, device=dev), target=torch.full((4, 2), 0.3, device=dev))
    wild = dict(prediction=torch.full((4, 2), float("nan"), device=dev), target=torch.ones(4, 2, device=dev))
    for m in (ap, acc):
        m.update(good)
        m.update(soft)
    with pytest.raises(ValueError, match="continuous"):
        ap.compute()
    assert acc.compute() == [0.5, 0.5]          # accuracy takes soft targets, as the reference's does
    for m in (ap, acc):
        m.reset()
        m.update(good)
        m.update(wild)
        with pytest.raises(ValueError, match="not finite"):
            m.compute()
        m.reset()          # status is cleared with the count
        m.update(good)
    assert ap.compute().tolist() == [1.0, 1.0] and acc.compute() == [0.0, 0.0]
    for bad in (dict(prediction=torch.zeros(4, 3, device=dev), target=torch.zeros(4, 3, device=dev)),
                dict(prediction=torch.zeros(4, device=dev), target=torch.zeros(4, device=dev)),
                dict(prediction=torch.zeros(4, 2, device=dev), target=torch.zeros(3, 2, device=dev))):
        with pytest.raises(ValueError):
            ap.update(bad)
    plain = metrics.AveragePrecision(["a", "b"])          # no library injected: CPU tensors raise, nothing is computed eagerly
    with pytest.raises(ValueError, match="cuda"):
        plain.update(dict(prediction=torch.zeros(4, 2), target=torch.zeros(4, 2)))
    with pytest.raises(ValueError):
        metrics.Accuracy(["a"], capacity=0)


def test_api_hooks_of_the_stand_in_base(be, ref):
    """where argus does not import: epoch_start -> reset, iteration_complete -> update(state.step_output)"""
    if metrics.Metric.__module__ != metrics.__name__:
        return          # argus is installed: its own Metric is the base class, and its hooks are its own
    ap, _ = make_metrics(be, 2, ref, capacity=8)
    out = dict(prediction=torch.full((4, 2), 0.25, device=be.device), target=torch.ones(4, 2, device=be.device))
    state = types.SimpleNamespace(phase="val", metrics={}, step_output=out)
    ap.iteration_complete(state)
    ap.epoch_start(state)
    assert ap.count == 0
    ap.iteration_complete(state)
    ap.epoch_complete(state)
    assert ap.count == 4 and state.metrics["val_average_precision"] == 1.0


# ================================================================================================ 6. GPU only
@pytest.mark.gpu
def test_update_never_synchronises_and_compute_is_deterministic(be_gpu, ref, host):
    case = "1000.15"
    pred, target = ref[f"pred.{case}"], ref[f"target.{case}"]
    ms = make_metrics(be_gpu, 15, ref, capacity=8)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m in ms:
            m.reset()
            for r in range(0, len(pred), 4):
                m.update(dict(prediction=p[r:r + 4], target=t[r:r + 4]))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    a, b = ms[0].compute(), ms[0].compute()
    assert a.tobytes() == b.tobytes()
    assert_same(a, host[case][0], "AP")
    assert ms[1].compute() == ms[1].compute() == ref[f"acc.{case}"].tolist()
