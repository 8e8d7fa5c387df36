"""MultiDimStacker.device_rng on the MI355X: the mask arena of a training step is the host prediction bit for bit (small fp32
and the benchmarked bf16 shape with the side stream), torch's CUDA generator is not touched, a step repeats bit for bit from a
restored rng_state when deterministic is on as well, and the fp32 step with the reference's drop rates meets the 1e-3 bar of
tests/test_fullsize_gpu.py against the float64 oracle fed host-predicted masks."""
import copy

import numpy as np
import pytest
import torch

from oracle import multidim_stacker_ref as orc
import mds
from mds import train as mtrain
from det_init import fill_deterministic
import device_rng_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.2, drop_path_rate=0.2)


def _plan(model):
    (plan,) = [pl for pool in model._cache.plans.values() for pl in pool if pl.need_grad and pl.kind == "full"]
    return plan


@pytest.mark.parametrize("B,H,W,bf16", [(1, 128, 128, False), (4, 736, 1280, True)])
def test_mask_arena_equals_the_host_prediction_and_torch_generator_is_untouched(B, H, W, bf16):
    torch.manual_seed(0)
    m = mds.MultiDimStacker(**KW).to(DEV).train()
    m.device_rng = True
    m.seed_rng((7 << 32) + 11)
    x = torch.rand(B, 15, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    tgt = torch.randint(0, 2, (B, 2), device=DEV, generator=torch.Generator(DEV).manual_seed(6)).float()
    before = torch.cuda.get_rng_state(DEV)
    for draw in range(3):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            logits = m(x)
        orc.sigmoid_focal_loss(logits.float(), tgt, alpha=-1.0, gamma=1.2).backward()
        torch.cuda.synchronize()
        plan = _plan(m)
        assert plan.device_rng and (not bf16 or plan._side_stream() is not None)
        want = host.mask(host.plan_keep(plan), (7 << 32) + 11, 0, draw)
        assert torch.equal(plan.mask_arena.tensor.cpu(), want), draw
        assert torch.isfinite(logits).all()
    assert m.rng_draws == 3
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)


def test_step_repeats_bit_for_bit_from_a_restored_rng_state():
    torch.manual_seed(0)
    m = mds.MultiDimStacker(**KW).to(DEV).train()
    m.device_rng = m.deterministic = True
    m.seed_rng(123)
    opt = mtrain.FusedAdamW(list(m.parameters()), lr=3e-4)
    loss_fn = mtrain.FocalLoss(alpha=-1.0, gamma=1.2, deterministic=True)
    x = torch.rand(2, 15, 256, 256, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    tgt = torch.tensor([[1.0, 0.0], [0.0, 1.0]], device=DEV)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = m(x)
            loss = loss_fn(logits, tgt)
        loss.backward()
        grads = torch.cat([p.grad.flatten() for p in m.parameters()])
        opt.step()
        torch.cuda.synchronize()
        return logits.detach().clone(), grads, torch.cat([p.detach().flatten() for p in m.parameters()])

    step()                                                  # the optimizer's moments exist and are not zero
    state, ostate, rng = copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict()), m.rng_state()
    runs = []
    for _ in range(2):
        m.load_state_dict(state)
        opt.load_state_dict(copy.deepcopy(ostate))
        m.set_rng_state(rng)
        torch.rand(17, device=DEV)                          # other users of torch's generator do not matter any more
        runs.append([step(), step()])                       # two steps from the same rng_state
    for (a, b) in zip(runs[0], runs[1]):
        for what, p, q in zip(("logits", "gradients", "parameters"), a, b):
            assert torch.isfinite(p.float()).all() and torch.equal(p, q), what
    assert not torch.equal(runs[0][0][0], runs[0][1][0])    # the second step drew other masks


def test_fp32_step_with_drop_rates_vs_float64_oracle_fed_predicted_masks():
    ref = fill_deterministic(orc.MultiDimStacker(**KW), 11, scale=0.05).train()
    prod = mds.MultiDimStacker(**KW)
    prod.load_state_dict(ref.state_dict())
    prod = prod.to(DEV).train()
    prod.device_rng = True
    prod.seed_rng(20261017)
    x = torch.rand(1, 15, 128, 128, generator=torch.Generator().manual_seed(111))
    tgt = torch.tensor([[1.0, 0.0]])
    ref = ref.double()
    arena = host.feed_oracle(ref, 1, 20261017, 0, 0, dtype=torch.float64)
    assert 0 < int((arena == 0).sum()) < arena.numel()
    lr = ref(x.double())
    orc.sigmoid_focal_loss(lr, tgt.double(), alpha=-1.0, gamma=1.2).backward()
    gr = {n: p.grad.detach().float() for n, p in ref.named_parameters() if p.grad is not None}
    lp = prod(x.to(DEV))
    orc.sigmoid_focal_loss(lp, tgt.to(DEV), alpha=-1.0, gamma=1.2).backward()
    rel = lambda got, want, floor=0.0: (got.detach().float().cpu() - want.detach().float()).abs().max().item() / max(want.detach().float().abs().max().item(), floor, 1e-20)
    gp = {n: p.grad for n, p in prod.named_parameters()}
    floor = 1e-2 * float(np.median([g.abs().max().item() for g in gr.values()]))
    errs = sorted(((rel(gp[n], gr[n], floor), n) for n in gr), reverse=True)
    print(f"[device rng gpu] logits rel err {rel(lp, lr):.2e}, worst gradient errors {errs[:3]}")
    assert rel(lp, lr) < 1e-3
    assert errs[0][0] < 1e-3, errs[:6]
    for (n, b), (_, b2) in zip(ref.named_buffers(), prod.named_buffers()):
        assert rel(b2, b, 1e-6) < 1e-3, n
