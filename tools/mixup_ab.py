"""Developer tool: mds.augment.TimmMixup against the torch-op restatement of the reference's TimmMixup (tests/mixup_host.py)
moved to the GPU, at the training shape 4 x 15 x 736 x 1280 fp32.  HIP events around each call (host draws included on both
sides, the same np.random seed), the two sides alternating, three rounds of `--reps` calls; per round the median call, then the
median of the rounds and the rounds' min - max.  The first call of each side checks that both give the same bits.

    python tools/mixup_ab.py [--reps 10] > profiles/mixup_ab.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ball-action-spotting_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import mixup_host
from mds import augment

SHAPE = (4, 15, 736, 1280)
SETTINGS = {       # name -> (constructor arguments, np.random seed of every call)
    "batch blend": (dict(mixup_alpha=0.4, cutmix_alpha=0.0, mode="batch"), 4),
    "batch cut": (dict(mixup_alpha=0.0, cutmix_alpha=1.0, mode="batch"), 4),
    "elem, mixed jobs": (dict(mixup_alpha=0.4, cutmix_alpha=1.0, mode="elem"), 2),
}


def timed(fn, x, target, seed):
    np.random.seed(seed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(x, target)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    reps = ap.parse_args().reps
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand(*SHAPE, generator=g).to(dev)
    target = (torch.rand(SHAPE[0], 2, generator=g) < 0.5).float().to(dev)
    mb = x0.numel() * 4 / 1e6
    print(f"shape {SHAPE} fp32 = {mb:.0f} MB, {reps} calls per round, ms per call: median of the rounds' medians [rounds' min - max]")
    for name, (kw, seed) in SETTINGS.items():
        kw = dict(kw, prob=1.0, label_smoothing=0.1, num_classes=2)
        sides = {"mds": augment.TimmMixup(**kw), "torch ops": mixup_host.TimmMixup(**kw)}
        np.random.seed(seed)
        jobs = augment.TimmMixup(**kw)._jobs(SHAPE[0], SHAPE[2], SHAPE[3])
        first = {}
        for side, fn in sides.items():                       # warm-up + parity
            xs = x0.clone()
            _, (xo, to) = timed(fn, xs, target, seed)
            first[side] = (xo.view(torch.int32).clone(), to.view(torch.int32).clone())
        same = all(torch.equal(a, b) for a, b in zip(first["mds"], first["torch ops"]))
        rounds = {side: [] for side in sides}
        xs = {side: x0.clone() for side in sides}
        for _ in range(3):
            ms = {side: [] for side in sides}
            for _ in range(reps):
                for side, fn in sides.items():               # alternating
                    ms[side].append(timed(fn, xs[side], target, seed)[0])
            for side in sides:
                rounds[side].append(statistics.median(ms[side]))
        desc = ", ".join(f"{('none', 'blend', 'cut')[m]}" + (f"{tuple(b)}" if m == 2 else "") for m, _, _, b in jobs)
        print(f"{name}: jobs [{desc}], bit-identical results: {same}")
        for side in sides:
            r = rounds[side]
            print(f"    {side:10s} {statistics.median(r):8.3f} ms  [{min(r):.3f} - {max(r):.3f}]")
        print(f"    ratio torch ops / mds (medians): {statistics.median(rounds['torch ops']) / statistics.median(rounds['mds']):.2f}")


if __name__ == "__main__":
    main()
