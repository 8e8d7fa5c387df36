"""mds_spot (csrc/k_spot.hip), mds.spotting and StreamPredictor.predict_track.

Every comparison is exact (== on bits): the header's arithmetic is normative.
  1. tests/spotting_host.py (numpy, written from the header's rules) against the reference's own post_processing as recorded in
     tests/golden/spotting_ref.npz (make_golden_spotting.py) - and against scipy itself where it imports;
  2. the fixture's precondition: no case in which scipy's result hangs on its unstable sort;
  3. the kernel against the fixture, given the fixture's recorded weights, on the simulator and on the GPU, guard-banded;
  4. - 6. the peak rules on hand-made signals, the tile and chunk seams, the refusals;
  7. the Python API against the host implementation;  8. predict_track against predict_stream.
"""
import numpy as np
import pytest
import torch

import spotting_host as sh
from backends import be  # noqa: F401
from mds import cabi, spotting

SIZES = (1, 2, 3, 12, 13, 25, 26, 97, 1000, 4500)
FAMILIES = ("noise", "bumps", "flat", "const", "edge_l", "edge_r")
SINGLE, BLEND = cabi.MDS_SPOT_SINGLE, cabi.MDS_SPOT_BLEND
BAD = cabi.MDS_ERR_BAD_ARG


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(ibits(got).ravel() != ibits(want).ravel())
    assert bad.size == 0, f"{msg}: {bad.size} of {got.size} values differ in their bits, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


def families_of(n):
    return FAMILIES if n < 1000 else ("noise", "bumps", "const")


@pytest.fixture(scope="module")
def ref(golden):
    return golden("spotting_ref")


def test_header_constants():
    assert cabi.MDS_VERSION >= 141 and (SINGLE, BLEND) == (0, 1)
    assert cabi.MDS_SPOT_MAX_TRACKS == 16 and cabi.MDS_SPOT_MAX_RADIUS == 64
    assert ("mds_spot", "const mds_spot_args* a, mds_stream_t stream") in cabi.LONG_FUNCS


# ================================================================================================ 1. host against the fixture
def test_fixture_covers_the_cases(ref):
    cases = set(ref["cases"].tolist())
    assert ref["params"].tolist() == [[3.0, 0.2, 15], [1.0, 0.5, 1], [3.0, 0.0, 40]]
    for n in SIZES:
        for fam in families_of(n):
            for dt in ("f32", "f64"):
                assert f"{fam}.{n}.{dt}.0" in cases
                assert ref[f"series.{fam}.{n}.{dt}"].dtype == (np.float32 if dt == "f32" else np.float64)
    plateau = [c for c in cases if c.startswith("flat.97.")]
    assert plateau and all(len(ref[f"peaks.{c}.idx"]) >= 1 for c in plateau)
    assert all(len(ref[f"peaks.{c}.idx"]) == 0 for c in cases if c.startswith("const."))
    assert sum(len(ref[f"peaks.{c}.idx"]) for c in cases) > 1000


def test_host_weights_are_scipys(ref):
    for sigma in (1.0, 3.0):
        assert_same(sh.gaussian_weights(sigma), ref[f"weights.{sigma}"], f"sigma {sigma}")
        assert_same(spotting.gaussian_weights(sigma), ref[f"weights.{sigma}"], f"mds.spotting, sigma {sigma}")


@pytest.mark.parametrize("family", FAMILIES)
def test_host_reproduces_the_recorded_reference(ref, family):
    seen = 0
    for case in ref["cases"].tolist():
        fam, n, dt, pi = case.split(".")
        if fam != family:
            continue
        sigma, height, distance = ref["params"][int(pi)]
        x = ref[f"series.{fam}.{n}.{dt}"]
        y, p, v = sh.spot(x.astype(np.float64), ref[f"weights.{sigma}"], height, int(distance), single=dt == "f32")
        assert_same(y, ref[f"smoothed.{fam}.{n}.{dt}.{sigma}"], case + " smoothed")
        assert_same(p, ref[f"peaks.{case}.idx"], case + " indexes")
        assert_same(v, ref[f"peaks.{case}.conf"], case + " confidences")
        seen += 1
    assert seen >= 24


def test_host_reproduces_the_recorded_blend(ref):
    for bi, K in ((0, 3), (1, 14)):
        firsts = ref[f"blend.{bi}.first"].tolist()
        tracks = [ref[f"blend.{bi}.track.{k}"] for k in range(K)]
        x, lo = sh.blend(tracks, firsts)
        assert_same(x, ref[f"blend.{bi}.x"], "blend")
        assert lo == ref[f"blend.{bi}.frame_indexes"][0] and len(x) == len(ref[f"blend.{bi}.frame_indexes"])
        for c in range(x.shape[1]):
            y, p, v = sh.spot(x[:, c], ref["weights.3.0"], 0.2, 15, single=False)
            assert_same(y, ref[f"blend.{bi}.smoothed.{c}"], "blend smoothed")
            assert_same(p + lo, ref[f"blend.{bi}.idx.{c}"], "blend indexes")
            assert_same(v, ref[f"blend.{bi}.conf.{c}"], "blend confidences")


def test_host_against_scipy_directly(ref):
    ndimage = pytest.importorskip("scipy.ndimage")
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 11, 12, 13, 24, 25, 26, 333):
        for dt in (np.float32, np.float64):
            x = (1.0 / (1.0 + np.exp(-3.0 * rng.standard_normal(n)))).astype(dt)
            for sigma, height, distance in ((3.0, 0.2, 15), (1.0, 0.5, 1), (0.6, 0.0, 4)):
                if sh.has_tie(ndimage.gaussian_filter(x, sigma), height, distance):
                    continue          # (scipy's order is unspecified there; never met with this seed)
                y, p, v = sh.spot(x.astype(np.float64), sh.gaussian_weights(sigma), height, distance, single=dt == np.float32)
                assert_same(y, ndimage.gaussian_filter(x, sigma), f"gaussian_filter n={n}")
                peaks, _ = signal.find_peaks(y, height=height, distance=distance)
                assert_same(p, peaks.astype(np.int64), f"find_peaks n={n}")


# ================================================================================================ 2. the precondition
def test_no_fixture_case_hangs_on_scipys_unstable_sort(ref):
    """from the fixture alone: no two candidate peaks that pass `height`, lie closer than `distance` and have bit-equal values"""
    checked = 0
    for case in ref["cases"].tolist():
        fam, n, dt, pi = case.split(".")
        sigma, height, distance = ref["params"][int(pi)]
        assert not sh.has_tie(ref[f"smoothed.{fam}.{n}.{dt}.{sigma}"], height, int(distance)), case
        checked += 1
    for bi in (0, 1):
        for c in range(2):
            assert not sh.has_tie(ref[f"blend.{bi}.smoothed.{c}"], 0.2, 15)
            checked += 1
    assert checked == len(ref["cases"]) + 4


# ================================================================================================ 3. the kernel
def launch(be, tracks, firsts, weights, height, distance, mode, cap=None, smoothed=True, f64=False, fields=None):
    """tracks: numpy (n_k, C) arrays -> dict(rc, smoothed (N, C), index (C, cap), conf (C, cap), count (C), cap) as numpy.
    Every buffer is guarded; `fields` replaces members of the argument struct (the refusals)."""
    K, C = len(tracks), tracks[0].shape[1]
    lo = min(firsts)
    N = max(f + len(t) for f, t in zip(firsts, tracks)) - lo
    if cap is None:
        cap = max(1, (N - 3) // distance + 1 if N >= 3 else 1)
    tdt = torch.float64 if f64 else torch.float32
    tt = [be.t(torch.from_numpy(np.ascontiguousarray(t)), dtype=tdt, name=f"track{k}") for k, t in enumerate(tracks)]
    w = be.t(torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)), name="weights")
    sdt = torch.float32 if mode == SINGLE else torch.float64
    sm = be.out((N, C), sdt, fill=-3.0, name="smoothed") if smoothed else None
    index = be.out((C, cap), torch.int32, fill=-1, name="peak_index")
    conf = be.out((C, cap), torch.float64, fill=-1.0, name="peak_conf")
    count = be.out((C,), torch.int32, fill=-1, name="peak_count")
    ws = be.out((cabi.MDS_SPOT_WS_BYTES * N * C + 7) // 8, torch.float64, fill=float("nan"), name="workspace")
    pad = [0] * (cabi.MDS_SPOT_MAX_TRACKS - K)
    kw = dict(mode=mode, K=K, C=C, track=[t.data_ptr() for t in tt] + pad, track_f64=int(f64), first=list(firsts) + pad,
              rows=[len(t) for t in tracks] + pad, weights=w, radius=(len(weights) - 1) // 2, distance=distance, height=height,
              cap=cap, peak_index=index, peak_conf=conf, peak_count=count, smoothed=sm, workspace=ws, workspace_bytes=ws.numel() * 8)
    kw.update(fields or {})
    args = cabi.make("mds_spot_args", **kw)
    args._keep.extend(tt)
    rc = be.rc("spot", args)
    be.sync()
    return dict(rc=rc, smoothed=None if sm is None else sm.cpu().numpy(), index=index.cpu().numpy(), conf=conf.cpu().numpy(),
                count=count.cpu().numpy(), cap=cap, N=N)


def assert_peaks(out, c, rows, confs, msg):
    n = len(rows)
    assert out["count"][c] == n, f"{msg}: class {c}: {out['count'][c]} peaks, expected {n}"
    m = min(n, out["cap"])
    assert_same(out["index"][c, :m], np.asarray(rows[:m], dtype=np.int32), f"{msg}: class {c} rows")
    assert_same(out["conf"][c, :m], np.asarray(confs[:m], dtype=np.float64), f"{msg}: class {c} confidences")
    assert (out["index"][c, m:] == -1).all() and (out["conf"][c, m:] == -1.0).all(), f"{msg}: class {c}: entries past the count were written"


CASES3 = [(n, c, 0) for n in SIZES for c in (1, 2, 15)] + [(n, 15, pi) for n in (2, 12, 26, 97, 1000) for pi in (1, 2)]


@pytest.mark.parametrize("n,C,pi", CASES3)
def test_kernel_reproduces_the_recorded_reference(be, ref, n, C, pi):
    """the fixture's series of one length interleaved as the C classes of one launch; r = 12 > N for the small lengths.
    SINGLE on the fp32 series, BLEND (K = 1, float64 track) on the float64 series."""
    sigma, height, distance = ref["params"][pi]
    fams = [families_of(n)[c % len(families_of(n))] for c in range(C)]
    for dt, mode in (("f32", SINGLE), ("f64", BLEND)):
        x = np.stack([ref[f"series.{f}.{n}.{dt}"] for f in fams], 1)
        out = launch(be, [x], [0], ref[f"weights.{sigma}"], float(height), int(distance), mode, f64=dt == "f64")
        assert out["rc"] == 0
        want = np.stack([ref[f"smoothed.{f}.{n}.{dt}.{sigma}"] for f in fams], 1)
        assert_same(out["smoothed"], want, f"{dt} smoothed")
        for c, f in enumerate(fams):
            assert_peaks(out, c, ref[f"peaks.{f}.{n}.{dt}.{pi}.idx"], ref[f"peaks.{f}.{n}.{dt}.{pi}.conf"], f"{dt} {f}")


@pytest.mark.parametrize("bi,K", [(0, 3), (1, 14)])
def test_kernel_blends_as_the_recorded_reference(be, ref, bi, K):
    firsts = ref[f"blend.{bi}.first"].tolist()
    tracks = [ref[f"blend.{bi}.track.{k}"] for k in range(K)]
    out = launch(be, tracks, firsts, ref["weights.3.0"], 0.2, 15, BLEND)
    assert out["rc"] == 0
    lo = min(firsts)
    assert_same(out["smoothed"], np.stack([ref[f"blend.{bi}.smoothed.{c}"] for c in range(2)], 1), "blend smoothed")
    for c in range(2):
        assert_peaks(out, c, ref[f"blend.{bi}.idx.{c}"] - lo, ref[f"blend.{bi}.conf.{c}"], "blend")
    # r = 0, weights [1.0]: the smoothed series IS the blend
    out = launch(be, tracks, firsts, np.ones(1), 0.2, 15, BLEND)
    assert_same(out["smoothed"], ref[f"blend.{bi}.x"], "blend (r = 0)")
    # a track that covers everything, listed last, fills no gap twice: K stays the divisor where a track is skipped
    x, _ = sh.blend(tracks[::-1], firsts[::-1])
    out = launch(be, tracks[::-1], firsts[::-1], np.ones(1), 0.2, 15, BLEND)
    assert_same(out["smoothed"], x, "blend, reversed track order")


# ================================================================================================ 4. peak logic, r = 0
def run_plain(be, cols, height, distance, cap=None, msg=""):
    """weights = [1.0]: y == x.  cols: the classes' fp32 series.  Checks smoothed == x and every class against the host implementation;
    returns the launch's output"""
    x = np.stack([np.asarray(c, dtype=np.float32) for c in cols], 1)
    out = launch(be, [x], [0], np.ones(1), height, distance, SINGLE, cap=cap)
    assert out["rc"] == 0
    assert_same(out["smoothed"], x, msg + " y == x")
    for c in range(x.shape[1]):
        p, v = sh.find_peaks(x[:, c], height, distance)
        assert_peaks(out, c, p, v, msg)
    return out


def spikes(n, rows, heights):
    x = np.zeros(n, dtype=np.float32)
    x[list(rows)] = np.asarray(heights, dtype=np.float32)
    return x


def test_staircases_take_one_dependency_round_per_peak(be):
    rows = [8 * k + 4 for k in range(40)]
    up = spikes(328, rows, [0.1 + 0.02 * k for k in range(40)])
    out = run_plain(be, [up, up[::-1].copy(), np.zeros(328)], 0.05, 15, msg="staircase")
    # rising: every peak is outranked by its right neighbour, 8 rows away - the greedy keeps 39, 37, ... ; falling mirrors it
    assert out["index"][0, :out["count"][0]].tolist() == rows[1::2]
    assert out["index"][1, :out["count"][1]].tolist() == [327 - r for r in rows[1::2]][::-1]
    assert out["count"][2] == 0


def test_equal_peaks_within_distance_the_lower_row_wins(be):
    two = spikes(64, [10, 17], [0.5, 0.5])
    chain = spikes(64, [10, 17, 24, 31, 50], [0.5, 0.5, 0.5, 0.5, 0.5])
    mixed = spikes(64, [10, 17, 24], [0.5, 0.75, 0.5])
    out = run_plain(be, [two, chain, mixed], 0.2, 15, msg="ties")
    assert out["index"][0, :out["count"][0]].tolist() == [10]
    assert out["index"][1, :out["count"][1]].tolist() == [10, 31, 50]
    assert out["index"][2, :out["count"][2]].tolist() == [17]


def test_height_equal_to_a_peaks_value_keeps_it(be):
    x = spikes(32, [5, 20], [0.25, 0.2499999])
    out = run_plain(be, [x], 0.25, 3, msg="height")
    assert out["index"][0, :out["count"][0]].tolist() == [5]


def test_plateaus_edges_and_distance_one(be):
    x = np.zeros(64, dtype=np.float32)
    x[10:14] = 0.5          # even length: (10 + 13) // 2 = 11
    x[30:33] = 0.7          # odd length: 31
    x[40:42] = 0.3          # rises again without falling: no peak
    x[42] = 0.6
    edge = np.zeros(64, dtype=np.float32)
    edge[0:4] = 0.9         # plateaus that touch an edge: no peaks
    edge[60:64] = 0.9
    edge[1], edge[62] = 1.0, 1.0          # ... but rows 1 and N - 2 can be peaks
    every_other = spikes(64, range(1, 63, 2), [0.3 + 0.01 * k for k in range(31)])
    out = run_plain(be, [x, edge, every_other], 0.2, 1, msg="plateaus, distance 1")
    assert out["index"][0, :out["count"][0]].tolist() == [11, 31, 42]
    assert out["index"][1, :out["count"][1]].tolist() == [1, 62]
    assert out["count"][2] == 31
    flat_edges = np.full(64, 0.4, dtype=np.float32)
    flat_edges[20:30] = 0.1          # two plateaus that touch the edges around a dip
    out = run_plain(be, [flat_edges], 0.2, 5, msg="edge plateaus")
    assert out["count"][0] == 0


def test_cap_smaller_than_the_count(be):
    many = spikes(100, range(5, 95, 9), [0.3 + 0.01 * k for k in range(10)])
    few = spikes(100, [50], [0.9])
    out = run_plain(be, [many, few, many], 0.2, 2, cap=3, msg="cap")
    assert out["count"].tolist() == [10, 1, 10] and out["index"][0].tolist() == [5, 14, 23] and out["index"][1].tolist() == [50, -1, -1]


# ================================================================================================ 5. tile seams
def test_tile_and_chunk_seams(be):
    """peaks and one long plateau across the smoothing kernel's row tiles and the selection kernel's per-thread chunks"""
    T, TH = cabi.MDS_SPOT_TILE, cabi.MDS_SPOT_THREADS
    n = 5 * T + 3
    L = -(-n // TH)
    rng = np.random.default_rng(11)
    x = (0.05 + 0.1 * rng.random(n)).astype(np.float32)
    x[T - 3:T + 41] = 1.0                                     # a saturated run across tile 0 | 1 and a dozen chunks
    for t in (2, 3, 4):
        x[[t * T - 1, t * T + 4]] = [0.8 + 0.01 * t, 0.7]     # peaks on both sides of a seam, closer than `distance`
    x[3 * L * 40 - 1] = 0.6
    y2 = (0.1 + 0.8 * rng.random(n)).astype(np.float32)
    xs = np.stack([x, y2], 1)
    be.reset_launches()
    for w in (sh.gaussian_weights(1.0), sh.gaussian_weights(3.0), np.ones(1)):
        out = launch(be, [xs], [0], w, 0.2, 15, SINGLE)
        assert out["rc"] == 0
        for c in range(2):
            y, p, v = sh.spot(xs[:, c].astype(np.float64), w, 0.2, 15, single=True)
            assert_same(out["smoothed"][:, c], y, "seams smoothed")
            assert_peaks(out, c, p, v, "seams")
        if len(w) == 9:          # sigma 1: the run's interior is one exact plateau whose midpoint is reported
            p, _ = sh.spot(xs[:, 0].astype(np.float64), w, 0.2, 15, single=True)[1:]
            assert (T - 3 + T + 40) // 2 in p.tolist()
    rec = be.launches("spot")
    if rec is not None:          # the simulator's launch record: the geometry the series was built for
        smooth = [l for l in rec if "smooth" in l.kernel]
        select = [l for l in rec if "select" in l.kernel]
        assert len(smooth) == len(select) == 3 and len(rec) == 6          # two kernels per launch
        assert all((l.gx, l.gy, l.bx) == (-(-n // T), 1, TH) for l in smooth)
        assert all((l.gx, l.bx) == (2, TH) for l in select)


# ================================================================================================ 6. refusals
def test_refusals_launch_nothing(be):
    x = np.full((40, 2), 0.5, dtype=np.float32)
    w = sh.gaussian_weights(3.0)
    be.reset_launches()

    def refused(tracks=(x,), firsts=(0,), mode=SINGLE, f64=False, **fields):
        """`fields` replace members of the argument struct after it was filled for a good launch"""
        out = launch(be, list(tracks), list(firsts), w, 0.2, 15, mode, f64=f64, fields=fields)
        assert out["rc"] == BAD, (fields, out["rc"])
        assert (out["count"] == -1).all() and (out["smoothed"] == -3.0).all()
    refused(rows=[0] * 16)                                     # N < 1
    refused(C=0)
    refused(K=0)
    refused(K=17)
    refused(tracks=[x, x], firsts=[0, 10])                     # SINGLE with K != 1
    refused(mode=2)
    refused(mode=SINGLE, f64=True)
    refused(radius=-1)
    refused(radius=65)
    refused(distance=0)
    refused(cap=0)
    for field in ("weights", "peak_index", "peak_conf", "peak_count", "workspace"):
        refused(**{field: None})
    refused(track=[0] * 16)
    refused(workspace_bytes=cabi.MDS_SPOT_WS_BYTES * 40 * 2 - 1)
    refused(tracks=[x, x], firsts=[0, 41], mode=BLEND)         # a one-frame gap
    refused(tracks=[x, x, x], firsts=[100, 0, 39], mode=BLEND)  # [0, 40) [39, 79) | [100, 140)
    rec = be.launches()
    assert rec is None or rec == []
    out = launch(be, [x, x, x], [80, 0, 40], w, 0.2, 15, BLEND)      # touching ranges in any order are contiguous
    assert out["rc"] == 0 and out["N"] == 120


# ================================================================================================ 7. the Python API
def test_api_against_the_host_implementation(be, ref):
    dev = be.device
    x = np.stack([ref["series.noise.1000.f32"], ref["series.bumps.1000.f32"], ref["series.const.1000.f32"]], 1)
    fi = np.arange(250, 1250)
    track = spotting.PredictionTrack.from_numpy(fi, x, dev)
    assert track.first_index == 250 and track.count == 1000 and track.capacity == 1000 and track.num_classes == 3
    assert_same(track.numpy(), x, "round trip")
    assert np.array_equal(track.frame_indexes(), fi)
    with pytest.raises(ValueError):
        spotting.PredictionTrack.from_numpy(fi[::2], x[::2], dev)
    if be.name == "emu":          # no library injected: CPU tensors raise, nothing is computed eagerly
        with pytest.raises(cabi.MdsError):
            spotting.Spotter()(track)
    sp = spotting.Spotter(3.0, 0.2, 14.2)          # find_peaks ceils the distance
    sp._lib = be.lib
    assert sp.distance == 15 and sp.radius == 12
    w = sh.gaussian_weights(3.0)
    got = sp(track)
    sm = sp.smoothed(track)
    assert isinstance(got, list) and len(got) == 3 and sm.dtype == torch.float32 and sm.device.type == dev.type
    for c in range(3):
        y, p, v = sh.spot(x[:, c].astype(np.float64), w, 0.2, 15, single=True)
        assert_same(sm[:, c].cpu().numpy(), y, "Spotter.smoothed")
        idx, conf = got[c]
        assert idx == (p + 250).tolist() and conf == v.tolist()
        assert all(type(i) is int for i in idx) and all(type(f) is float and f == float(np.float32(f)) for f in conf)
    assert len(got[0][0]) > 10 and got[2] == ([], [])
    # a list of tracks: BLEND, float64
    t2 = spotting.PredictionTrack.from_numpy(np.arange(200, 900), x[::-1][:700].copy(), dev)
    xb, lo = sh.blend([x, x[::-1][:700]], [250, 200])
    got = sp([track, t2])
    smb = sp.smoothed([track, t2])
    assert smb.dtype == torch.float64
    for c in range(3):
        y, p, v = sh.spot(xb[:, c], w, 0.2, 15, single=False)
        assert_same(smb[:, c].cpu().numpy(), y, "Spotter.smoothed, blend")
        assert got[c] == ((p + lo).tolist(), v.tolist())
    bx, bfi = spotting.blend([track, t2], _lib=be.lib)
    assert_same(bx, xb, "blend")
    assert np.array_equal(bfi, np.arange(200, 1250))
    with pytest.raises(ValueError):
        spotting.Spotter(distance=0.5)
    with pytest.raises(ValueError):
        spotting.Spotter(gauss_sigma=0.0)
    with pytest.raises(cabi.MdsError):          # the launch's refusal of a gap reaches the caller
        sp([track, spotting.PredictionTrack.from_numpy(np.arange(2000, 2010), x[:10].copy(), dev)])


def test_reference_signatures(be, ref):
    dev = be.device
    for dt in ("f32", "f64"):
        x = ref[f"series.noise.1000.{dt}"]
        for pi, (sigma, height, distance) in enumerate(ref["params"]):
            idx, conf = spotting.post_processing(list(range(7, 1007)), x, sigma, height, int(distance), device=dev, _lib=be.lib)
            _, p, v = sh.spot(x.astype(np.float64), sh.gaussian_weights(sigma), height, int(distance), single=dt == "f32")
            assert idx == (p + 7).tolist() and conf == v.tolist()
            assert idx == (ref[f"peaks.noise.1000.{dt}.{pi}.idx"] + 7).tolist() and conf == ref[f"peaks.noise.1000.{dt}.{pi}.conf"].tolist()
        idx, conf = spotting.post_processing([0], torch.from_numpy(x), 3.0, 0.2, 15, device=dev, _lib=be.lib)      # a tensor
        assert idx == ref[f"peaks.noise.1000.{dt}.0.idx"].tolist()
    raw = np.stack([ref["series.noise.1000.f32"], ref["series.bumps.1000.f32"]], 1)
    params = dict(gauss_sigma=3.0, height=0.2, distance=15)
    acts = spotting.raw_predictions_to_actions(np.arange(3, 1003), raw, {"PASS": 0, "DRIVE": 1}, params, device=dev, _lib=be.lib)
    assert list(acts) == ["PASS", "DRIVE"]
    for cls, fam in (("PASS", "noise"), ("DRIVE", "bumps")):
        assert isinstance(acts[cls], tuple) and len(acts[cls]) == 2
        assert acts[cls][0] == (ref[f"peaks.{fam}.1000.f32.0.idx"] + 3).tolist() and acts[cls][1] == ref[f"peaks.{fam}.1000.f32.0.conf"].tolist()


# ================================================================================================ 8. the predictor
def test_predict_track_rows_are_predict_streams_results(be):
    """emu: (64, 32) frames, no graphs, the plain-call path of a CPU module; gpu: (96, 64), TTA, chunk 5 on 3 lanes - and a Spotter
    on the resulting track against the host implementation on track.numpy()"""
    import mds
    from det_init import fill_deterministic
    from oracle import multidim_stacker_ref as orc
    from mds.predict import StreamPredictor
    gpu = be.name == "gpu"
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    prod = fill_deterministic(mds.MultiDimStacker(**kw), 5, scale=0.02).to(be.device).eval()
    if not gpu:
        prod._lib = be.lib
    g = torch.Generator().manual_seed(3)
    if gpu:
        n, size, chunk, opts, lanes = 75, (96, 64), 5, dict(tta=True), 3
        frames = torch.randint(0, 256, (n, 58, 90), generator=g).to(torch.uint8).cuda()
    else:
        n, size, chunk, opts, lanes = 45, (64, 32), 4, dict(use_graphs=False), None
        frames = torch.randint(0, 256, (n, 32, 64), generator=g, dtype=torch.uint8)
    a = StreamPredictor(prod, frame_size=size, **opts)
    track = a.predict_track(frames, 0, chunk=chunk, lanes=lanes)
    if gpu:
        torch.cuda.current_stream().synchronize()      # the caller's stream is behind the lanes: no device-wide wait is needed
    b = StreamPredictor(prod, frame_size=size, **opts)
    res = list(b.predict_stream(iter(frames), 0, chunk=chunk, lanes=lanes))
    want = [(p, i) for p, i in res if p is not None]
    assert track.first_index == want[0][1] == a.predict_offset and track.count == len(want) == n - 2 * a.predict_offset
    assert track.capacity == n and track.data.device.type == be.device.type
    rows = track.numpy()
    assert_same(rows, torch.stack([p for p, _ in want]).float().cpu().numpy(), "predict_track rows")
    assert np.array_equal(track.frame_indexes(), np.array([i for _, i in want]))
    assert np.abs(rows[1:] - rows[:-1]).max() > 1e-6          # distinct frames, distinct rows: the comparison is not vacuous
    # a given track that is too short refuses to grow (b holds the frames and their stacks already: no new encoder work)
    with pytest.raises(cabi.MdsError, match="cannot grow"):
        b.predict_track(iter(frames[:32]), 0, chunk=chunk, lanes=lanes, track=spotting.PredictionTrack(1, track.num_classes, be.device))
    if gpu:
        torch.cuda.synchronize()
        sp = spotting.Spotter(1.0, 0.0, 3)
        got = sp(track)
        for c in range(track.num_classes):
            _, p, v = sh.spot(rows[:, c].astype(np.float64), sh.gaussian_weights(1.0), 0.0, 3, single=True)
            assert got[c] == ((p + track.first_index).tolist(), v.tolist())
    for s in (a, b):
        s.close()


def test_predict_track_needs_a_capacity_before_the_first_pass():
    import mds
    from oracle import multidim_stacker_ref as orc
    from mds.predict import StreamPredictor
    prod = mds.MultiDimStacker(**dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0))
    sp = StreamPredictor(prod, frame_size=(64, 32), use_graphs=False)
    with pytest.raises(ValueError, match="num_frames"):
        sp.predict_track(iter([torch.zeros(32, 64, dtype=torch.uint8)]), 0)
