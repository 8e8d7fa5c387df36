"""Developer tool: the training ingest at the training shape - 4 clips of 15 x 720 x 1280 uint8 luma frames -> the
(4, 15, 736, 1280) fp32 batch.  Four forms, HIP events around each call, alternating, three rounds of `--reps` calls; per round
the median call, then the median of the rounds and the rounds' min - max:

    (a) torch ops    the reference's chain restated with torch ops on the device: per clip F.pad, .to(float32), / 255.0
                     (src/frames.py), then the loader's stack
    (b) mds          mds.frames.PadNormalizeFramesProcessor on the stacked raw batch: one mds_pad_normalize launch
    (c) two-step     (a) followed by the fp32 augmentation call
    (d) fused        the augmentation call on the raw uint8 batch (frames_processor= given): no padded fp32 input
    (e) mds two-step (b) followed by the fp32 augmentation call: what the fusion has to beat
    (d'), (e')       (d) and (e) with the host side of the call prepared beforehand (prepared=): the launches alone

(c), (d) and (e) run get_train_augmentations in its default reference-order mode with parameters drawn at the reference's
probabilities from a fixed seed - call k of every round uses the k-th drawn set on both sides, host preparation included on both.
Random frames (every byte value); the first call of each form is the warm-up and the parity check (bits).

    python tools/frames_ingest_ab.py [--reps 10] > profiles/frames_ingest_ab.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ball-action-spotting_amd")]
import torch
import torch.nn.functional as F

from mds import augment, frames

RAW = (4, 15, 720, 1280)
SIZE = (1280, 736)
SEED = 5


def timed(fn, *args):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(*args)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    reps = ap.parse_args().reps
    dev = "cuda:0"
    x = torch.randint(0, 256, RAW, dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    clips = [x[i] for i in range(RAW[0])]
    proc = frames.get_frames_processor("pad_normalize", dict(size=SIZE))
    H, W, top, left, fill = proc.geometry(RAW[2], RAW[3])
    pads = [left, W - RAW[3] - left, top, H - RAW[2] - top]
    plain = augment.get_train_augmentations(SIZE)
    fused = augment.get_train_augmentations(SIZE, frames_processor=proc)
    sets = augment.TrainAugmentations(SIZE, seed=SEED).sample_params(RAW[0] * reps, RAW[1], H, W)
    sets = [sets[k * RAW[0]:(k + 1) * RAW[0]] for k in range(reps)]

    def torch_chain(k):
        return torch.stack([F.pad(c, pads, mode="constant", value=fill).to(torch.float32) / 255.0 for c in clips])

    forms = {
        "(a) torch ops: pad, float, / 255, stack": torch_chain,
        "(b) mds_pad_normalize": lambda k: proc(x),
        "(c) (a) + fp32 augmentations": lambda k: plain(torch_chain(k), params=sets[k]),
        "(d) fused: augmentations on uint8": lambda k: fused(x, params=sets[k]),
        "(e) (b) + fp32 augmentations": lambda k: plain(proc(x), params=sets[k]),
        # the launches alone: the host side of the call (job tables, maps, their upload) prepared outside the timed window
        "(d') fused, launches alone": lambda k: fused(x, prepared=prep[k]),
        "(e') (b) + fp32, launches alone": lambda k: plain(proc(x), prepared=prep[k]),
    }
    prep = [fused.prepare(s, RAW[1], H, W, torch.device(dev)) for s in sets]
    raw_mb, out_mb = x.numel() / 1e6, RAW[0] * RAW[1] * H * W * 4 / 1e6
    print(f"raw {RAW} uint8 = {raw_mb:.0f} MB -> ({RAW[0]}, {RAW[1]}, {H}, {W}) fp32 = {out_mb:.0f} MB; pads top {top} left {left}; "
          f"{reps} calls per round, ms per call: median of the rounds' medians [rounds' min - max]")
    first = {name[:4].strip(): timed(fn, 0)[1].clone() for name, fn in forms.items()}      # warm-up + parity
    names = list(forms)
    host = F.pad(x.cpu(), pads, mode="constant", value=fill).to(torch.float32) / 255.0      # the reference's expression where the fixture was made: on the host
    bits = lambda u, v: torch.equal(u.view(torch.int32), v.view(torch.int32))
    same = {"(b) to the host's torch expression": bits(first["(b)"].cpu(), host), "(d) to (e)": bits(first["(d)"], first["(e)"]),
            "(d') to (d)": bits(first["(d')"], first["(d)"]), "(e') to (e)": bits(first["(e')"], first["(e)"])}
    print("bit-identical: " + "; ".join(f"{k}: {v}" for k, v in same.items()))
    # torch's DEVICE kernel for `tensor / host scalar` multiplies by the scalar's reciprocal: (a) is the other function there
    ramp = torch.arange(256, dtype=torch.uint8)
    dev_div, host_div = (ramp.to(dev).to(torch.float32) / 255.0).cpu(), ramp.to(torch.float32) / 255.0
    diff = first["(a)"] != first["(b)"]
    print(f"(a) on the device against (b): {int(diff.sum())} of {diff.numel()} elements differ, max |difference| {float((first['(a)'] - first['(b)']).abs().max()):.2e}; "
          f"byte values for which the device's `/ 255.0` differs from the host's: {int((dev_div != host_div).sum())} of 256, from x * (1 / 255): "
          f"{int((dev_div != ramp.to(torch.float32) * torch.tensor(1.0 / 255.0, dtype=torch.float32)).sum())}")
    del first, host, diff
    stages = {}
    for s in sets:
        for p in s:
            for key in p:
                stages[key] = stages.get(key, 0) + 1
    print(f"augmentation parameters: seed {SEED}, {reps} sets of {RAW[0]} samples, stages fired: {dict(sorted(stages.items()))}")
    rounds = {name: [] for name in forms}
    for _ in range(3):
        ms = {name: [] for name in forms}
        for k in range(reps):
            for name, fn in forms.items():               # alternating
                ms[name].append(timed(fn, k)[0])
        for name in forms:
            rounds[name].append(statistics.median(ms[name]))
    med = {}
    for name in forms:
        r = rounds[name]
        med[name] = statistics.median(r)
        print(f"    {name:42s} {med[name]:8.3f} ms  [{min(r):.3f} - {max(r):.3f}]")
    a, b, c, d, e, d1, e1 = (med[n] for n in names)
    print(f"    (a) / (b): {a / b:.2f}    (c) / (d): {c / d:.2f}    (e) / (d): {e / d:.2f}    (e') / (d'): {e1 / d1:.2f}")
    print(f"    (b) moves {raw_mb + out_mb:.0f} MB: {(raw_mb + out_mb) / 1e3 / b:.2f} TB/s")


if __name__ == "__main__":
    main()
