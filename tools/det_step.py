"""MultiDimStacker.deterministic on the GPU: repeatability check and A/B timing of the training step.

  python tools/det_step.py check --config train --batch 4 --height 736 --width 1280 --dtype bf16 --deterministic 1
      runs the same training step --repeats times, each from a restored copy of the same parameters, buffers, optimizer state
      and generator state, and prints one JSON line: how many elements of logits / loss / BatchNorm buffers / the flat gradient
      arena / the parameters after the optimizer step differ from the first run (0 everywhere = bit-identical).
      tests/test_deterministic_step_gpu.py runs this in a child process per case, each under its own time limit.
  python tools/det_step.py ab --rounds 3 --steps 30
      config 2's step (bench.py's shape and recipe) in ONE process, default and deterministic plans alternating, --rounds rounds:
      median ms/step and windows/s of both, the workspace bytes, and the finishing launches' own time (every mds_wgrad_finish of
      the step's shapes, timed back to back on an idle GPU, in total and per entry-point family).
"""
import argparse
import copy
import ctypes as C
import json
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
from mds import cabi, train as mtrain
from oracle import multidim_stacker_ref as orc


def build(args, dev):
    torch.manual_seed(0)
    long = args.config == "long004"
    kw = dict(orc.BASIC_CONFIG_KWARGS, num_frames=33 if long else 15)      # the reference's drop rates: DropPath / dropout masks are drawn
    model = mds.MultiDimStacker(**kw).to(dev).train()
    if long:      # ball_finetune_long_004: encoder frozen (BatchNorm stays in train mode), SGD + Nesterov
        for p in model.conv2d_encoder.parameters():
            p.requires_grad_(False)
    trainable = [p for p in model.parameters() if p.requires_grad]
    opt = mtrain.FusedSGD(trainable, lr=1e-3, momentum=0.9, nesterov=True) if long else mtrain.FusedAdamW(trainable, lr=3e-4)
    loss_fn = mtrain.FocalLoss(alpha=0.4 if long else -1.0, gamma=1.2, deterministic=True)
    T = 33 if long else 15
    x = torch.rand(args.batch, T, args.height, args.width, device=dev, generator=torch.Generator(dev).manual_seed(1234))
    target = torch.randint(0, 2, (args.batch, 2), device=dev, generator=torch.Generator(dev).manual_seed(4321)).float()
    return model, opt, loss_fn, x, target


def make_step(model, opt, loss_fn, x, target, amp):
    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            logits = model(x)
            loss = loss_fn(logits, target)
        loss.backward()
        plan = next(pl for pool in model._cache.plans.values() for pl in pool if pl.need_grad and pl.deterministic == bool(model.deterministic))
        arena = plan.grad_arena.tensor.clone()
        opt.step()
        return logits.detach().clone(), loss.detach().clone(), arena, plan
    return step


def check(args):
    dev = torch.device("cuda:0")
    model, opt, loss_fn, x, target = build(args, dev)
    model.deterministic = bool(args.deterministic)
    step = make_step(model, opt, loss_fn, x, target, args.dtype == "bf16")
    step()                                                   # one step first: the optimizer's moments exist and are not zero
    torch.cuda.synchronize()
    state = copy.deepcopy(model.state_dict())
    ostate = copy.deepcopy(opt.state_dict())
    rng = torch.cuda.get_rng_state(dev)
    runs = []
    for _ in range(args.repeats):
        model.load_state_dict(state)
        opt.load_state_dict(copy.deepcopy(ostate))
        torch.cuda.set_rng_state(rng, dev)
        logits, loss, arena, plan = step()
        torch.cuda.synchronize()
        runs.append(dict(logits=logits, loss=loss.view(1), arena=arena,
                         buffers=torch.cat([b.detach().reshape(-1).double() for b in model.buffers()]),
                         params=torch.cat([p.detach().reshape(-1) for p in model.parameters()])))
    diff = {k: max(int((r[k] != runs[0][k]).sum().item()) for r in runs[1:]) for k in runs[0]}
    finite = all(bool(torch.isfinite(r[k].float()).all()) for r in runs for k in r)
    print(json.dumps(dict(config=args.config, shape=[args.batch, x.shape[1], args.height, args.width], dtype=args.dtype,
                          deterministic=bool(args.deterministic), plan_deterministic=bool(plan.deterministic), repeats=args.repeats,
                          differing_elements=diff, sizes={k: int(v.numel()) for k, v in runs[0].items()}, finite=finite,
                          arena_nonzero=int((runs[0]["arena"] != 0).sum().item()), det_workspace_bytes=int(plan.det_workspace_bytes),
                          loss=float(runs[0]["loss"].item()))))


FINISH_NUMEL = {"pw_wgrad": lambda s: s.N * s.K, "conv_wgrad": lambda s: s.Cout * s.Cin * s.wtaps, "stem_wgrad": lambda s: s.Cout * 27,
                "dw_bwd": lambda s: s.C * s.kt * 9, "gem_bwd": lambda s: 1}


def finish_time(plan, reps=20):
    """every finishing launch of the plan's step (its numel and slot count), on its own: back to back, median of `reps` passes"""
    lib, jobs = plan.lib, []
    for seg, ops in plan.bound.items():
        for name, fn, st, _ in ops:
            base = name.split("@")[0]
            if base in FINISH_NUMEL and st.partial.buf:
                numel = FINISH_NUMEL[base](st)
                stride = (numel + 3) // 4 * 4
                jobs.append((base, numel, st.partial.floats // stride, stride))
    if not jobs:
        return 0.0, [], {}
    part = torch.zeros(max(s * st for _, _, s, st in jobs), device=plan.device)
    dst = torch.zeros(max(n for _, n, _, _ in jobs), device=plan.device)
    args = [cabi.make("mds_wgrad_finish_args", partial=part, dst=dst, numel=n, slots=s, slot_stride=st) for _, n, s, st in jobs]
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for a in args:
            lib.check(lib.fn["wgrad_finish"](C.byref(a), stream), "wgrad_finish")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    fam = {}
    for base in sorted({j[0] for j in jobs}):      # the same per entry-point family
        sel, ts = [a for a, j in zip(args, jobs) if j[0] == base], []
        for _ in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for a in sel:
                lib.check(lib.fn["wgrad_finish"](C.byref(a), stream), "wgrad_finish")
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        fam[base] = (len(sel), statistics.median(ts[2:]))
    return statistics.median(times[2:]), jobs, fam


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

    def run(det, steps):
        model.deterministic = det
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
        for det in (False, True):
            ms[det].append(run(det, args.steps))
            print(f"round {r + 1} {'deterministic' if det else 'default      '}: {ms[det][-1]:.3f} ms/step  {args.batch / ms[det][-1] * 1e3:.1f} windows/s", flush=True)
    plan = next(pl for pool in model._cache.plans.values() for pl in pool if pl.need_grad and pl.deterministic)
    fin_ms, jobs, fam = finish_time(plan)
    med = {d: statistics.median(v) for d, v in ms.items()}
    print(f"median default       {med[False]:.3f} ms/step  {args.batch / med[False] * 1e3:.1f} windows/s   (rounds: {', '.join(f'{v:.3f}' for v in ms[False])})")
    print(f"median deterministic {med[True]:.3f} ms/step  {args.batch / med[True] * 1e3:.1f} windows/s   (rounds: {', '.join(f'{v:.3f}' for v in ms[True])})")
    print(f"deterministic / default = {med[True] / med[False]:.4f}")
    print(f"workspace: {plan.det_workspace_bytes} bytes ({plan.det_workspace_bytes / 2 ** 20:.1f} MiB) in two buffers (chain stream, weight-gradient stream)")
    print(f"finishing launches: {len(jobs)} per step, {sum(s * st * 4 for _, _, s, st in jobs) / 2 ** 20:.1f} MiB of slots read, {fin_ms:.3f} ms back to back on an idle GPU")
    print("per family (launches, ms back to back): " + "; ".join(f"{b} {n} x, {t:.3f} ms ({'chain' if b in ('dw_bwd', 'stem_wgrad', 'gem_bwd') else 'weight-gradient'} stream)" for b, (n, t) in fam.items()))
    big = sorted(jobs, key=lambda j: -j[2] * j[3])[:5]
    print("largest: " + "; ".join(f"{b} {n} floats x {s} slots" for b, n, s, _ in big))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["check", "ab"])
    ap.add_argument("--config", default="train", choices=["train", "long004"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=736)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--deterministic", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    {"check": check, "ab": ab}[a.mode](a)
