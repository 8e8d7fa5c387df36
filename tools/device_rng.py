"""MultiDimStacker.device_rng on the GPU: A/B timing of the training step.

  python tools/device_rng.py ab --rounds 3 --steps 30
      config 2's step (bench.py's shape and recipe, the reference's drop rates) in ONE process, the default plan (masks from
      torch's generator: bernoulli_ + div_) and the device_rng plan (one mds_mask_fill) alternating, --rounds rounds: ms/step
      and windows/s of both, the spread between the default rounds, and the fill's own kernel time (the plan's launch,
      back to back on an idle GPU).
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ball-action-spotting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

import mds
from mds import train as mtrain


def fill_time(plan, reps=200):
    """the plan's own mds_mask_fill launch, `reps` times back to back between two events: us per launch"""
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            plan.lib.check(plan.lib.fn["mask_fill"](plan._fill_ref, stream), "mask_fill")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(times[1:])


def ab(args):
    dev = torch.device("cuda:0")
    import bench
    torch.manual_seed(0)
    model = mds.MultiDimStacker(**bench.CONFIG).to(dev).train()
    opt = mtrain.FusedAdamW(list(model.parameters()), lr=3e-4)
    loss_fn = mtrain.FocalLoss(alpha=-1.0, gamma=1.2)
    x = torch.rand(args.batch, 15, args.height, args.width, device=dev, generator=torch.Generator(dev).manual_seed(1234))
    target = torch.randint(0, 2, (args.batch, 2), device=dev, generator=torch.Generator(dev).manual_seed(4321)).float()
    start = copy.deepcopy(model.state_dict())

    def run(on, steps):
        model.device_rng = on
        model.load_state_dict(start)
        t0 = None
        for k in range(args.warmup + steps):
            if k == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = loss_fn(model(x), target)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    ms = {False: [], True: []}
    for r in range(args.rounds):
        for on in (False, True):
            ms[on].append(run(on, args.steps))
            print(f"round {r + 1} {'device_rng' if on else 'default   '}: {ms[on][-1]:.3f} ms/step  {args.batch / ms[on][-1] * 1e3:.1f} windows/s", flush=True)
    plan = next(pl for pool in model._cache.plans.values() for pl in pool if pl.need_grad and pl.device_rng)
    med = {d: statistics.median(v) for d, v in ms.items()}
    print(f"drop rates: drop_rate {model.drop_rate}, mask arena {plan.mask_arena.numel} floats in {len(plan.masks)} masks")
    print(f"median default    {med[False]:.3f} ms/step  {args.batch / med[False] * 1e3:.1f} windows/s   (rounds: {', '.join(f'{v:.3f}' for v in ms[False])})")
    print(f"median device_rng {med[True]:.3f} ms/step  {args.batch / med[True] * 1e3:.1f} windows/s   (rounds: {', '.join(f'{v:.3f}' for v in ms[True])})")
    print(f"device_rng - default = {med[True] - med[False]:+.3f} ms/step; spread of the default rounds {max(ms[False]) - min(ms[False]):.3f} ms")
    print(f"mds_mask_fill: {fill_time(plan):.2f} us per launch, back to back on an idle GPU ({plan.mask_arena.numel} floats)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=736)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    {"ab": ab}[a.mode](a)
