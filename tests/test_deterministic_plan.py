"""MultiDimStacker.deterministic through the planner, on the host kernel simulator (the set-up of tests/test_module_emu.py):
every launch of the backward schedule that adds into a parameter gradient carries a partial buffer, the step still matches the
oracle and the default plan at test_full_model_train_step_fp32_vs_oracle's bar, and the switch is engine state like
compute_dtype / eval_fusion."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from oracle import multidim_stacker_ref as orc
import mds
from mds import cabi
from mds.engine import Plan
from test_module_emu import _pair, _cmp

KW = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
# every entry point of include/mds.h that ends in fp32 atomics on a parameter gradient
ATOMIC_GRAD_OPS = {"pw_wgrad", "conv_wgrad", "stem_wgrad", "dw_bwd", "gem_bwd"}


def _train_step(model, x, tgt):
    model.zero_grad(set_to_none=True)
    out = model(x)
    orc.sigmoid_focal_loss(out, tgt, alpha=-1.0, gamma=1.2).backward()
    return out


def _plans(prod, **want):
    return [pl for pool in prod._cache.plans.values() for pl in pool if all(getattr(pl, k) == v for k, v in want.items())]


def _grad_errors(prod, ref):
    rp, pp = dict(ref.named_parameters()), dict(prod.named_parameters())
    floor = 1e-2 * float(np.median([p.grad.abs().max().item() for p in rp.values()]))
    worst = sorted(((((pp[n].grad - rp[n].grad).abs().max().item() / max(rp[n].grad.abs().max().item(), floor)), n) for n in rp), reverse=True)
    return worst


def test_switch_is_engine_state():
    m = mds.MultiDimStacker(**orc.BASIC_CONFIG_KWARGS)
    assert m.deterministic is False
    keys = list(m.state_dict())
    m.deterministic = True
    assert list(m.state_dict()) == keys                                   # not part of state_dict
    assert copy.deepcopy(m).deterministic is True and pickle.loads(pickle.dumps(m)).deterministic is True
    old = copy.deepcopy(m)
    del old.__dict__["deterministic"]                                     # a module pickled before the attribute existed: off
    from hipemu.loader import load_emulator
    old._lib = load_emulator()
    assert not old.train()._plan(torch.rand(1, 15, 32, 32), "full", 1, 15, 32, 32, True).deterministic


def test_every_gradient_launch_of_a_deterministic_plan_has_a_partial_buffer():
    ref, prod = _pair(KW)
    prod.train()
    x = torch.rand(1, 15, 48, 40, generator=torch.Generator().manual_seed(1))
    tgt = torch.tensor([[1.0, 0.0]])
    _train_step(prod, x, tgt)
    (off,) = _plans(prod, kind="full", need_grad=True)
    assert not off.deterministic and off.det_workspace_bytes == 0
    prod.deterministic = True
    _train_step(prod, x, tgt)
    (on,) = _plans(prod, kind="full", need_grad=True, deterministic=True)      # flipping the flag built another plan
    assert on is not off and on.det_workspace_bytes > 0
    seen = set()
    for plan, want in ((on, True), (off, False)):
        for seg, ops in plan.bound.items():
            for name, fn, st, _ in ops:
                base = name.split("@")[0]
                has = hasattr(st, "partial")
                assert has == (base in ATOMIC_GRAD_OPS), f"{base}: the ABI and this test disagree about which launches end in fp32 atomics"
                if not has:
                    continue
                assert seg[0] == "b", (seg, base)
                assert bool(st.partial.buf) == want, (seg, base)
                if want:
                    seen.add(base)
                    need = plan.lib.fn[base + "_partial_floats"](C.byref(st))
                    assert 0 < need == st.partial.floats, (base, need, st.partial.floats)
    assert seen == ATOMIC_GRAD_OPS, seen
    # both streams' workspaces are what the plan reports; the forward-only plans ignore the switch
    with torch.no_grad():
        prod(x)
    assert all(not pl.deterministic for pl in _plans(prod, need_grad=False))
    prod.eval()
    with torch.no_grad():
        prod(x)
    assert all(not pl.deterministic for pl in _plans(prod, need_grad=False))


def test_deterministic_train_step_fp32_vs_oracle_and_vs_the_default_plan():
    ref, prod = _pair(KW)
    ref.train(); prod.train()
    x = torch.rand(1, 15, 48, 40, generator=torch.Generator().manual_seed(1))
    tgt = torch.tensor([[1.0, 0.0]])
    state = copy.deepcopy(prod.state_dict())
    lr = _train_step(ref, x, tgt)
    l0 = _train_step(prod, x, tgt).detach().clone()
    g0 = {n: p.grad.clone() for n, p in prod.named_parameters()}
    b0 = {n: b.clone() for n, b in prod.named_buffers()}
    prod.load_state_dict(state)
    prod.deterministic = True
    l1 = _train_step(prod, x, tgt)
    assert _plans(prod, kind="full", need_grad=True, deterministic=True)
    # the oracle, at test_full_model_train_step_fp32_vs_oracle's bar
    _cmp("logits", l1, lr, 1e-4, 1e-4)
    worst = _grad_errors(prod, ref)
    assert worst[0][0] < 2e-3, f"worst relative grad errors: {worst[:8]}"
    for (n, b), (_, b2) in zip(ref.named_buffers(), prod.named_buffers()):
        _cmp("buffer " + n, b2, b, 1e-4, 1e-4)
    # the default plan, at the same bar: the forward is the same launches (bit-identical), the gradients differ by summation order
    assert torch.equal(l1, l0)
    for n, b in prod.named_buffers():
        assert torch.equal(b, b0[n]), n
    floor = 1e-2 * float(np.median([g.abs().max().item() for g in g0.values()]))
    worst = sorted((((p.grad - g0[n]).abs().max().item() / max(g0[n].abs().max().item(), floor), n) for n, p in prod.named_parameters()), reverse=True)
    print(f"[deterministic emu] deterministic against default gradients, worst: {worst[:3]}")
    assert worst[0][0] < 2e-3, worst[:8]
    # and it repeats bit for bit on the simulator too
    g1 = {n: p.grad.clone() for n, p in prod.named_parameters()}
    prod.load_state_dict(state)
    l2 = _train_step(prod, x, tgt)
    assert torch.equal(l2, l1) and all(torch.equal(p.grad, g1[n]) for n, p in prod.named_parameters())


def _assert_all_bound(pl):
    n = 0
    for seg, ops in pl.bound.items():
        for name, fn, st, _ in ops:
            if hasattr(st, "partial"):
                assert st.partial.buf and st.partial.floats > 0, (pl.kind, seg, name)
                n += 1
    assert n > 0, pl.kind
    return n


def test_the_frozen_encoder_plan_binds_the_tail_only():
    ref, prod = _pair(KW)
    prod.train()
    prod.deterministic = True
    for p in prod.conv2d_encoder.parameters():
        p.requires_grad_(False)
    _train_step(prod, torch.rand(1, 15, 48, 40, generator=torch.Generator().manual_seed(1)), torch.tensor([[1.0, 0.0]]))
    (plan,) = _plans(prod, kind="full", need_grad=True)
    assert plan.deterministic and not plan.enc_grad
    names = {n.split("@")[0] for seg, ops in plan.bound.items() if seg[0] == "b" for n, *_ in ops}
    assert "stem_wgrad" not in names and "conv_wgrad" not in names and {"pw_wgrad", "dw_bwd", "gem_bwd"} <= names      # only the tail's launches exist
    _assert_all_bound(plan)
    frozen = {id(p) for p in prod.conv2d_encoder.parameters()}
    assert all(p.grad is None for p in prod.parameters() if id(p) in frozen) and all(p.grad is not None for p in prod.parameters() if id(p) not in frozen)


@pytest.mark.parametrize("kind", ["tail", "2d", "3d", "head"])
def test_sub_forward_plans_honour_the_switch(kind):
    """forward_tail and forward_2d / forward_3d / forward_head under autograd (the one autograd bridge, every sub kind): the plan of that kind
    is a deterministic one, every gradient launch of its backward schedule is bound, and its gradients match the default plan's"""
    ref, prod = _pair(KW)
    prod.train()
    g = torch.Generator().manual_seed(2)
    S, C3, F = prod.num_stacks, prod.num_3d_features, prod.num_features
    inp = {"tail": lambda: torch.rand(1, S, C3, 3, 3, generator=g), "3d": lambda: torch.rand(1, S, C3, 3, 3, generator=g),
           "2d": lambda: torch.rand(1, 15, 48, 40, generator=g), "head": lambda: torch.rand(1, F, 3, 3, generator=g)}[kind]()
    fwd = {"tail": prod.forward_tail, "2d": prod.forward_2d, "3d": prod.forward_3d, "head": prod.forward_head}[kind]
    state = copy.deepcopy(prod.state_dict())
    grads = {}
    for det in (False, True):
        prod.load_state_dict(state)
        prod.deterministic = det
        prod.zero_grad(set_to_none=True)
        x = inp.clone().requires_grad_(kind != "2d")
        out = fwd(x)
        (out * torch.linspace(0.5, 1.5, out.numel()).view(out.shape)).sum().backward()
        plans = _plans(prod, kind=kind, need_grad=True, deterministic=det)
        assert len(plans) == 1, [(pl.kind, pl.deterministic) for pl in _plans(prod, need_grad=True)]
        if det:
            assert _assert_all_bound(plans[0]) > 0 and plans[0].det_workspace_bytes > 0
        grads[det] = {n: p.grad.clone() for n, p in prod.named_parameters() if p.grad is not None}
    assert grads[True].keys() == grads[False].keys() and grads[True]
    floor = 1e-2 * float(np.median([v.abs().max().item() for v in grads[False].values()]))
    worst = max((grads[True][n] - v).abs().max().item() / max(v.abs().max().item(), floor) for n, v in grads[False].items())
    assert worst < 2e-3, worst
