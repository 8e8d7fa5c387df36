"""Developer tool: spotting on the device against the reference's route on the host, and predict_track against predict_stream.

(a) mds.spotting.Spotter on device-resident tracks of one half (N = 67,500 rows), C in {2, 15} classes, K in {1, 14} tracks:
    ms per call (the launch and the one device-to-host copy of the peaks; HIP events on the stream and a host clock around the
    call, which ends in that copy).  Baseline, the reference's route: a device-to-host copy of the tracks, then on the host the
    float64 blend (K > 1) and, per class, smoothing + peaks - with tests/spotting_host.py (numpy; its peak loops are Python) and,
    where it imports, with scipy as src/utils.py::post_processing calls it.  The first call of each side checks equal results.
(b) StreamPredictor.predict_track, frames/s at 720 x 1280 raw frames, fp32, no TTA, chunk 8 x 3 lanes, against predict_stream
    consumed the reference's way (.cpu().numpy() per result) and with the results left on the device (twice: the run-to-run
    spread); the four runs alternate on one predictor each, after a warm-up that takes every lane past its graph capture.

    python tools/spot_ab.py [--frames 4000] [--reps 10]        (prints and writes profiles/spot_ab.txt)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ball-action-spotting_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import spotting_host as sh
from mds import spotting

N_HALF = 67500
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def make_tracks(K, C, dev, g):
    """K tracks of a half with slightly different first frames, sigmoid of noise on a slow wave: random, non-zero, peaks everywhere"""
    tracks = []
    for k in range(K):
        first = 14 + (k % 3)
        n = N_HALF - (k % 5)
        i = torch.arange(n, dtype=torch.float32)[:, None]
        x = torch.sigmoid(3.0 * torch.randn(n, C, generator=g) + 2.5 * torch.sin(i / 37.0 + k) - 0.5)
        t = spotting.PredictionTrack(n, C, dev)
        t.data.copy_(x)
        t.first_index, t.count = first, n
        tracks.append(t)
    return tracks


def host_route(tracks, sp, use_scipy):
    """the reference's route: tracks to the host, blend, per class gaussian_filter + find_peaks"""
    raws = [t.numpy() for t in tracks]                       # the device-to-host copies
    if len(tracks) == 1:
        x, lo, single = raws[0], tracks[0].first_index, True
    else:
        x, lo = sh.blend(raws, [t.first_index for t in tracks])
        single = False
    out = []
    for c in range(x.shape[1]):
        if use_scipy:
            from scipy.ndimage import gaussian_filter
            from scipy.signal import find_peaks
            y = gaussian_filter(x[:, c], sp.gauss_sigma)
            p, _ = find_peaks(y, height=sp.height, distance=sp.distance)
            out.append(((p + lo).tolist(), y[p].tolist()))
        else:
            _, p, v = sh.spot(x[:, c].astype(np.float64), sp.weights, sp.height, sp.distance, single)
            out.append(((p + lo).tolist(), v.tolist()))
    return out


def timed_device(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def part_a(reps):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    say(f"(a) Spotter(3.0, 0.2, 15), N = {N_HALF} rows; ms per call, median of 3 rounds' medians [rounds' min - max], {reps} calls per round")
    say("    mds: launch + one device-to-host copy of the peaks (events | host clock).  host: tracks to the host + blend + per-class")
    say(f"    smoothing and peaks, host clock: tests/spotting_host.py one call, scipy {'3 calls, as the reference calls it' if have_scipy else 'does not import here'}")
    for C in (2, 15):
        for K in (1, 14):
            tracks = make_tracks(K, C, dev, g)
            arg = tracks[0] if K == 1 else tracks
            sp = spotting.Spotter(3.0, 0.2, 15)
            got = sp(arg)                                   # warm-up (buffers, code objects) + parity
            t0 = time.perf_counter()
            want = host_route(tracks, sp, False)
            numpy_ms = (time.perf_counter() - t0) * 1e3          # one call: its peak loops are Python, seconds per call
            same = got == want
            same_scipy = (got == host_route(tracks, sp, True)) if have_scipy else None
            rounds_ev, rounds_host = [], []
            for _ in range(3):
                ms = [timed_device(lambda: sp(arg))[:2] for _ in range(reps)]
                rounds_ev.append(statistics.median(m[0] for m in ms))
                rounds_host.append(statistics.median(m[1] for m in ms))
            base = {"numpy host": [numpy_ms]}
            for name, flag in ((("scipy", True),) if have_scipy else ()):
                ts = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    host_route(tracks, sp, flag)
                    ts.append((time.perf_counter() - t0) * 1e3)
                base[name] = ts
            mb = sum(t.count for t in tracks) * C * 4 / 1e6
            say(f"  C = {C:2d}, K = {K:2d} ({mb:5.1f} MB of tracks, {sum(len(i) for i, _ in got)} peaks): equal to the numpy host: {same}"
                + (f", to scipy: {same_scipy}" if have_scipy else ""))
            say(f"      mds           {statistics.median(rounds_ev):9.3f} ms  [{min(rounds_ev):.3f} - {max(rounds_ev):.3f}]   host clock "
                f"{statistics.median(rounds_host):.3f} ms")
            for name, ts in base.items():
                say(f"      {name:13s} {statistics.median(ts):9.1f} ms  [{min(ts):.1f} - {max(ts):.1f}]")


def part_b(frames):
    import mds
    from mds.predict import StreamPredictor
    from oracle import multidim_stacker_ref as orc
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = mds.MultiDimStacker(**dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)).to(dev)
    for bn in model.modules():      # realistic running statistics: one training-mode pass with momentum 1
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(torch.rand(1, 15, 736, 1280, device=dev))
    model.eval()
    model.clear_plans()
    pool = torch.randint(0, 256, (64, 720, 1280), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(99))
    chunk, lanes, warm = 8, 3, 6 * 8 * 3 + 28 + 4

    def feed(first, n):
        return (pool[(first + j) % 64] for j in range(n))

    def stream_cpu(sp, first, n):
        rows = []
        for p, _ in sp.predict_stream(feed(first, n), first, chunk=chunk, lanes=lanes):
            if p is not None:
                rows.append(p.cpu().numpy())            # scripts/ball_action/predict.py::get_raw_predictions
        return len(rows)

    def stream_dev(sp, first, n):
        rows = [p for p, _ in sp.predict_stream(feed(first, n), first, chunk=chunk, lanes=lanes) if p is not None]
        return len(rows)

    def track(sp, first, n):
        return sp.predict_track(feed(first, n), first, chunk=chunk, lanes=lanes, num_frames=n).count

    runs = [("predict_stream, .cpu().numpy() per result", stream_cpu), ("predict_stream, results left on the device (1)", stream_dev),
            ("predict_track", track), ("predict_stream, results left on the device (2)", stream_dev)]
    say()
    say(f"(b) frames/s, 720 x 1280 raw frames, fp32, no TTA, chunk {chunk} x {lanes} lanes, {frames} frames per run after {warm} warm-up frames,")
    say("    host clock around the run and a device synchronise; the runs alternate, two rounds")
    sps = [StreamPredictor(model, frame_size=(1280, 736)) for _ in runs]
    for sp, (_, fn) in zip(sps, runs):
        fn(sp, 0, warm)
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in runs}
    first = warm
    for _ in range(2):
        for sp, (name, fn) in zip(sps, runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = fn(sp, first, frames)
            torch.cuda.synchronize()
            rates[name].append(frames / (time.perf_counter() - t0))
            assert rows == frames, (name, rows)
        first += frames
    for name, r in rates.items():
        say(f"  {name:48s} {r[0]:8.1f}  {r[1]:8.1f} frames/s")
    for sp in sps:
        sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spot_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spot_ab measures on the MI355X"
    part_a(args.reps)
    part_b(args.frames)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
