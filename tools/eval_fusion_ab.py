"""A/B of the opt-in inference fusions in ONE process: MultiDimStacker.eval_fusion ("A": the 2D blocks' 1x1 expansion inside
the depthwise launch), MultiDimStacker.eval_se_fusion ("SE": the squeeze-excite gate computed by the pooling depthwise launch) and
MultiDimStacker.eval_er_fusion ("ER": the edge-residual blocks' 3x3 expansion + 1x1 projection in one launch).
The chosen settings (--settings, default off / A / SE / A+SE) alternate over the same seeded raw 720 x 1280 frames.

  python tools/eval_fusion_ab.py [--frames K] [--rounds R]      the table (profiles/r08_eval_se_fusion_ab.txt)
  python tools/eval_fusion_ab.py --settings off,ER,A+SE+ER --blocks er      (profiles/r09_eval_er_fusion_ab.txt)
  python tools/eval_fusion_ab.py --trace off|A|SE|A+SE|ER|A+SE+ER   only predict() fp32 frame by frame with one setting (a child
                                                                 for rocprofv3 --kernel-trace --stats; fused / unfused = A / off)

Reports frames/s (median of R alternating rounds, and the min - max of the off rounds: the run-to-run spread a ratio has to beat)
of predict() fp32 frame by frame with TTA off / on, predict_stream 8 x 3, and predict() bf16; launches per 2D-encoder pass; the
largest difference between each setting's predictions and the off predictions of the same frames; and, per inverted-residual
block, the event-timed fused depthwise launch of A against the expansion pw_fwd + dw_fwd pair it replaces (a HIP event pair around
every launch of one encoder pass: launches serialised, small ones inflated alike); --blocks er: per edge-residual block, the fused
conv_fwd launch of ER against the conv_fwd + projection pw_fwd pair it replaces, timed the same way."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ball-action-spotting_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
import mds  # noqa: E402
from mds.predict import StreamPredictor  # noqa: E402

dev = torch.device("cuda:0")


def make_model():
    torch.manual_seed(0)
    m = mds.MultiDimStacker(**dict(bench.CONFIG, drop_rate=0.0, drop_path_rate=0.0)).to(dev)
    for bn in m.modules():      # realistic running statistics (random-init ones blow eval mode up)
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    m.train()
    with torch.no_grad():
        m(torch.rand(1, 15, 736, 1280, device=dev))
    return m.eval()


# (eval_fusion, eval_se_fusion, eval_er_fusion)
SETTINGS = {"off": (False, False, False), "A": (True, False, False), "SE": (False, True, False), "A+SE": (True, True, False),
            "ER": (False, False, True), "A+SE+ER": (True, True, True)}


def run(m, pool, setting, K, tta=False, cdt=None, chunk=1, lanes=0):
    """frames/s of K frames after the window is full and the graphs are captured; the predictions of the timed frames"""
    sp = StreamPredictor(m, frame_size=(1280, 736), tta=tta, compute_dtype=cdt, eval_fusion=SETTINGS[setting][0],
                         eval_se_fusion=SETTINGS[setting][1], eval_er_fusion=SETTINGS[setting][2])
    outs = []

    def feed(first, n, keep):
        if lanes:
            for out, _ in sp.predict_stream((pool[(first + j) % len(pool)] for j in range(n)), first, chunk=chunk, lanes=lanes):
                if keep and out is not None:
                    outs.append(out.float().clone())
            return
        for i in range(first, first + n):
            out, _ = sp.predict(pool[i % len(pool)], i)
            if keep:
                outs.append(out.float().clone())
    W = max(40, 6 * chunk * max(lanes, 1) + 28)
    W = -(-W // chunk) * chunk
    feed(0, W, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    feed(W, K, True)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    p2d = sp.plans[min(sp.plans)]["p2d"][0]
    n_launch = len(p2d.segs["f2d"])
    sp.close()
    return K / el, torch.stack(outs[-8:]), n_launch


def block_times(m, fusion, reps=5):
    """per inverted-residual block: the event-timed launches of one fp32 2D-encoder pass (1 x 3 x 736 x 1280), median of reps"""
    m.eval_fusion = fusion
    x = torch.rand(1, 3, 736, 1280, device=dev)
    with torch.no_grad():
        m.forward_2d(x)
    plan = next(p for pool in m._cache.plans.values() for p in pool if p.kind == "2d" and p.eval_fusion == fusion
                and not p.need_grad and p.ingest is None and p.B == 1)
    ops = plan.segs["f2d"]
    samples = []
    for _ in range(reps):
        plan.profile = []
        with torch.no_grad():
            m.forward_2d(x)
        torch.cuda.synchronize()
        prof = [e0.elapsed_time(e1) * 1e3 for name, seg, e0, e1, _ in plan.profile if seg == "f2d"]
        samples.append(prof)
        plan.profile = None
    us = [statistics.median(s[i] for s in samples) for i in range(len(ops))]
    rows = []      # (shape, expansion us, depthwise us)
    for i, (name, kw) in enumerate(ops):
        if name != "dw_fwd" or kw["kt"] != 1:
            continue
        ex = kw.get("expand")
        if ex:
            rows.append(((ex["cin"], kw["C"], kw["IH"], kw["IW"], kw["stride"]), 0.0, us[i]))
        else:
            j = next(j for j in range(i - 1, -1, -1) if ops[j][0] == "pw_fwd" and ops[j][1]["y"] is kw["x"])
            rows.append(((ops[j][1]["K"], kw["C"], kw["IH"], kw["IW"], kw["stride"]), us[j], us[i]))
    m.eval_fusion = False
    return rows


def er_block_times(m, fusion, reps=5):
    """per edge-residual block: the event-timed launches of one fp32 2D-encoder pass (1 x 3 x 736 x 1280), median of reps"""
    m.eval_er_fusion = fusion
    x = torch.rand(1, 3, 736, 1280, device=dev)
    with torch.no_grad():
        m.forward_2d(x)
    plan = next(p for pool in m._cache.plans.values() for p in pool if p.kind == "2d" and p.eval_er_fusion == fusion and not p.eval_fusion
                and not p.eval_se_fusion and not p.need_grad and p.ingest is None and p.B == 1)
    ops = plan.segs["f2d"]
    samples = []
    for _ in range(reps):
        plan.profile = []
        with torch.no_grad():
            m.forward_2d(x)
        torch.cuda.synchronize()
        samples.append([e0.elapsed_time(e1) * 1e3 for name, seg, e0, e1, _ in plan.profile if seg == "f2d"])
        plan.profile = None
    us = [statistics.median(s[i] for s in samples) for i in range(len(ops))]
    rows = []      # (shape, conv us, projection us)
    for i, (name, kw) in enumerate(ops):
        if name != "conv_fwd":
            continue
        if kw.get("project"):
            rows.append(((kw["Cin"], kw["Cout"], kw["project"]["cout"], kw["IH"], kw["IW"], kw["is"]), us[i], 0.0))
            continue
        j = next((j for j in range(i + 1, len(ops)) if ops[j][0] == "pw_fwd" and ops[j][1]["x"] is kw["y"]), None)
        if j is not None:
            rows.append(((kw["Cin"], kw["Cout"], ops[j][1]["N"], kw["IH"], kw["IW"], kw["is"]), us[i], us[j]))
    m.eval_er_fusion = False
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", choices=list(SETTINGS) + ["fused", "unfused"])
    ap.add_argument("--settings", default="off,A,SE,A+SE", help="comma-separated settings to alternate; the first is the baseline")
    ap.add_argument("--blocks", choices=["ir", "er", "both", "none"], default="ir", help="per-block event-timed table(s)")
    ap.add_argument("--cases", default="0,1,2,3", help="which of the four predictor cases to run")
    a = ap.parse_args()
    chosen = a.settings.split(",")
    assert chosen and all(k in SETTINGS for k in chosen), f"settings are {list(SETTINGS)}"
    base = chosen[0]
    m = make_model()
    pool = torch.randint(0, 256, (64, 720, 1280), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(99))
    if a.trace:
        setting = {"fused": "A", "unfused": "off"}.get(a.trace, a.trace)
        fps, _, n = run(m, pool, setting, a.frames)
        print(f"{setting}: predict() fp32 frame by frame {fps:.1f} frames/s, {n} launches per 2D-encoder pass")
        return
    cases = [("predict() fp32, TTA off", dict()), ("predict() fp32, TTA on", dict(tta=True)),
             ("predict_stream fp32, chunk 8 x 3 lanes", dict(chunk=8, lanes=3)), ("predict() bf16, TTA off", dict(cdt="bf16"))]
    cases = [cases[int(c)] for c in a.cases.split(",")]
    print(f"# inference fusions A/B ({' / '.join(chosen)}; baseline {base}): {a.frames} timed frames per run, {a.rounds} alternating rounds (median), "
          f"device {torch.cuda.get_device_name(0)}")
    print(f"{'case':40s} {'setting':>7s} {'frames/s':>9s} {'ratio':>6s} {'rounds min - max':>17s} {'launches 2D pass':>17s} {'max |diff|':>10s}")
    for label, kw in cases:
        res = {k: [] for k in chosen}
        outs, nl = {}, {}
        for _ in range(a.rounds):
            for k in chosen:
                fps, out, n = run(m, pool, k, a.frames, **kw)
                res[k].append(fps)
                outs[k], nl[k] = out, n
        u = statistics.median(res[base])
        for k in chosen:
            f = statistics.median(res[k])
            diff = (outs[k] - outs[base]).abs().max().item()
            print(f"{label if k == base else '':40s} {k:>7s} {f:9.1f} {f / u:6.3f} {min(res[k]):8.1f} - {max(res[k]):<6.1f} {nl[k]:>17d} {diff:10.2e}")
    if a.blocks in ("er", "both"):
        print()
        print("# per edge-residual block, fp32, 1 x 736 x 1280 (event-timed launches, median of 5 passes)")
        print(f"{'cin->mid->cout':>16s} {'input':>9s} {'s':>2s} {'conv_fwd us':>12s} {'pw_fwd us':>10s} {'pair us':>8s} {'fused us':>9s} {'ratio':>6s}")
        un, fu = er_block_times(m, False), er_block_times(m, True)
        tot_u = tot_f = 0.0
        for (shape, cv, pw), (shape2, fz, _) in zip(un, fu):
            assert shape == shape2, (shape, shape2)
            cin, mid, cout, ih, iw, s_ = shape
            tot_u += cv + pw; tot_f += fz
            print(f"{cin:4d}->{mid:4d}->{cout:<4d} {ih:4d}x{iw:<4d} {s_:2d} {cv:12.1f} {pw:10.1f} {cv + pw:8.1f} {fz:9.1f} {fz / (cv + pw):6.3f}")
        print(f"{'total':>30s} {'':>23s} {tot_u:8.1f} {tot_f:9.1f} {tot_f / tot_u:6.3f}")
    if a.blocks not in ("ir", "both"):
        return
    print()
    print("# per inverted-residual block, fp32, 1 x 736 x 1280 (event-timed launches, median of 5 passes)")
    print(f"{'cin->mid':>10s} {'input':>9s} {'s':>2s} {'pw_fwd us':>10s} {'dw_fwd us':>10s} {'pair us':>8s} {'fused us':>9s} {'ratio':>6s}")
    un, fu = block_times(m, False), block_times(m, True)
    tot_u = tot_f = 0.0
    for (shape, pw, dw), (shape2, _, fz) in zip(un, fu):
        assert shape == shape2
        cin, mid, ih, iw, s = shape
        tot_u += pw + dw; tot_f += fz
        print(f"{cin:4d}->{mid:<5d} {ih:4d}x{iw:<4d} {s:2d} {pw:10.1f} {dw:10.1f} {pw + dw:8.1f} {fz:9.1f} {fz / (pw + dw):6.3f}")
    print(f"{'total':>23s} {'':>21s} {tot_u:8.1f} {tot_f:9.1f} {tot_f / tot_u:6.3f}")


if __name__ == "__main__":
    main()
