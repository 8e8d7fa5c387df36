"""MultiDimStacker.deterministic = True on the MI355X: the same training step, run three times from a restored copy of the same
parameters, buffers, optimizer state and generator state, gives torch.equal logits, loss, BatchNorm buffers, gradient arena
and (after the fused optimizer's step) parameters.  DropPath / dropout are on (the reference's rates), both streams run.

Every case is one child process (tools/det_step.py check) under its own time limit; after a child that faulted, aborted or
ran out of time nothing more is started on the GPU: the remaining cases fail at once.

Figures: profiles/LOG.md ("Training: fixed-order weight-gradient sums")."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_fault = []


def _check(limit, **kw):
    if _fault:
        pytest.fail(f"not started: an earlier GPU step ended badly ({_fault[0]})")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "det_step.py"), "check"] + [f"--{k}={v}" for k, v in kw.items()]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _fault.append(f"{kw}: no result after {limit} s")
        pytest.fail(_fault[0])
    if r.returncode != 0:
        _fault.append(f"{kw}: exit status {r.returncode}")
        pytest.fail(_fault[0] + "\n" + r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("[deterministic step]", json.dumps(out))
    return out


def _assert_repeats(out):
    assert out["plan_deterministic"] and out["finite"] and out["det_workspace_bytes"] > 0
    assert out["arena_nonzero"] > 0, "the gradient arena is empty"
    assert out["differing_elements"] == dict(logits=0, loss=0, arena=0, buffers=0, params=0), out["differing_elements"]


def test_benchmarked_shape_bf16_repeats_bit_for_bit():
    _assert_repeats(_check(600, config="train", batch=4, height=736, width=1280, dtype="bf16", deterministic=1))


def test_small_fp32_step_repeats_bit_for_bit():
    _assert_repeats(_check(300, config="train", batch=1, height=128, width=128, dtype="f32", deterministic=1))


def test_config4_frozen_encoder_sgd_repeats_bit_for_bit():
    _assert_repeats(_check(600, config="long004", batch=1, height=736, width=1280, dtype="bf16", deterministic=1))


def test_default_mode_at_the_benchmarked_shape_information_only():
    """how many arena elements differ between two default-mode runs (float atomics): printed and recorded, never asserted -
    a run in which the atomics happen to arrive in the same order is not a failure"""
    out = _check(600, config="train", batch=4, height=736, width=1280, dtype="bf16", deterministic=0, repeats=2)
    assert not out["plan_deterministic"] and out["finite"]
    print(f"[deterministic step] default mode, two runs: {out['differing_elements']['arena']} of {out['sizes']['arena']} gradient-arena "
          f"elements differ, {out['differing_elements']['params']} parameters after AdamW")
