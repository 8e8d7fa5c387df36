"""Parity of the drop-in module on a real MI355X (through libmds_hip.so / the C ABI) against the
oracle on CPU and against the committed golden vectors of the reference.

Tolerances (BASELINE.json north_star: logits/grads within 1e-3 rel of reference):
  fp32 kernels  : |err| <= 1e-3 * max|ref| for logits and every parameter gradient
  bf16 kernels  : compared with the *fp32* oracle; the bar is 2x the error that torch's own
                  bf16-autocast run of the oracle shows (bf16 noise through 25 blocks is ~1e-2;
                  SURVEY.md §7 "Tolerance").
"""
import numpy as np
import pytest
import torch

from oracle import multidim_stacker_ref as orc
from det_init import fill_deterministic
import mds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def relerr(got, want, floor=0.0):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return (got - want).abs().max().item() / max(want.abs().max().item(), floor, 1e-20)


def build_pair(kw, seed=3, scale=0.05):
    ref = fill_deterministic(orc.MultiDimStacker(**kw), seed, scale=scale)
    prod = mds.MultiDimStacker(**kw)
    prod.load_state_dict(ref.state_dict())
    return ref, prod.to(DEV)


def step(model, x, tgt):
    model.zero_grad(set_to_none=True)
    logits = model(x)
    loss = orc.sigmoid_focal_loss(logits, tgt, alpha=-1.0, gamma=1.2)
    loss.backward()
    return logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def grad_errors(gp, gr):
    floor = 1e-2 * float(np.median([g.abs().max().item() for g in gr.values()]))
    return sorted(((relerr(gp[n], gr[n], floor), n) for n in gr), reverse=True)


def test_native_library_is_loaded():
    lib = mds.load()
    assert lib.path.endswith("libmds_hip.so") and not lib.missing


def test_fp32_train_step_vs_oracle_128():
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    ref, prod = build_pair(kw)
    ref.train(); prod.train()
    x = torch.rand(2, 15, 128, 160, generator=torch.Generator().manual_seed(1))
    tgt = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    lr, gr = step(ref, x, tgt)
    lp, gp = step(prod, x.to(DEV), tgt.to(DEV))
    assert relerr(lp, lr) < 1e-3
    errs = grad_errors(gp, gr)
    assert errs[0][0] < 1e-3, errs[:6]
    for (n, b), (_, b2) in zip(ref.named_buffers(), prod.named_buffers()):
        assert relerr(b2, b, 1e-6) < 1e-3, n
    # second step reuses the plan (buffers, arenas) — must stay correct
    lr2, gr2 = step(ref, x, tgt)
    lp2, gp2 = step(prod, x.to(DEV), tgt.to(DEV))
    assert relerr(lp2, lr2) < 1e-3
    assert grad_errors(gp2, gr2)[0][0] < 1e-3


def test_fp32_matches_reference_golden_config1(golden):
    """BASELINE configs[0] vectors produced by the reference's own MultiDimStacker code."""
    d = {**golden("full_cfg1"), **golden("full_cfg1_x")}      # (the input is a fixture of its own: files < 1 MiB)
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    prod = mds.MultiDimStacker(**kw)
    fill_deterministic(prod, 14, scale=0.02)
    prod = prod.to(DEV).train()
    x = torch.from_numpy(d["x"]).to(DEV)
    tgt = torch.from_numpy(d["target"]).to(DEV)
    logits, grads = step(prod, x, tgt)
    assert relerr(logits, torch.from_numpy(d["logits"])) < 1e-3
    for k in d:
        if k.startswith("grad."):
            assert relerr(grads[k[5:]], torch.from_numpy(d[k]), 1e-7) < 2e-3, k
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).item()
    np.testing.assert_allclose(total, d["gradnorm_total"], rtol=1e-3)


def test_bf16_autocast_within_2x_of_torch_bf16():
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    ref, prod = build_pair(kw, scale=0.03)
    ref.train(); prod.train()
    x = torch.rand(2, 15, 128, 160, generator=torch.Generator().manual_seed(2))
    tgt = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    l32, g32 = step(ref, x, tgt)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        l16, g16 = step(ref, x, tgt)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lp, gp = step(prod, x.to(DEV), tgt.to(DEV))
    e_ref, e_prod = relerr(l16, l32), relerr(lp, l32)
    assert e_prod <= 2 * e_ref + 5e-3, (e_prod, e_ref)
    # gradient direction: cosine with the fp32 gradient at least as good as torch-bf16's (minus slack)
    def cos(ga):
        a = torch.cat([ga[n].float().cpu().flatten() for n in g32]); b = torch.cat([g32[n].flatten() for n in g32])
        return torch.dot(a, b).item() / (a.norm().item() * b.norm().item())
    assert cos(gp) > min(cos(g16), 0.999) - 0.02, (cos(gp), cos(g16))


def test_stochastic_layers_with_shared_masks_fp32():
    """DropPath 0.2 / dropout 0.2 (config-faithful rates) with host-supplied masks on both sides."""
    kw = dict(orc.BASIC_CONFIG_KWARGS)
    ref, prod = build_pair(kw)
    ref.train(); prod.train()
    B, S = 2, 5
    x = torch.rand(B, 15, 96, 128, generator=torch.Generator().manual_seed(4))
    tgt = torch.tensor([[1.0, 0.0], [1.0, 1.0]])
    g = torch.Generator().manual_seed(5)
    masks = []
    for blk in [b for st in ref.conv2d_encoder.blocks for b in st]:
        if blk.has_skip and isinstance(blk.drop_path, orc.DropPath):
            keep = 1 - blk.drop_path.drop_prob
            mk = (torch.rand(B * S, generator=g) < keep).float() / keep
            blk.drop_path.forced_mask = mk
            masks.append(mk)
    for blk in ref.conv3d_encoder:
        mk = (torch.rand(B, generator=g) < 0.8).float() / 0.8
        blk.drop_path.forced_mask = mk
        masks.append(mk)
    dm = (torch.rand(B, 1280, generator=g) < 0.8).float() / 0.8
    ref.forced_dropout_mask = dm
    masks.append(dm.flatten())
    prod._mask_override = torch.cat(masks)
    lr, gr = step(ref, x, tgt)
    lp, gp = step(prod, x.to(DEV), tgt.to(DEV))
    assert relerr(lp, lr) < 1e-3
    assert grad_errors(gp, gr)[0][0] < 1e-3


def test_eval_and_predictor_style_calls():
    """forward_2d / forward_3d / forward_head called separately (src/predictors.py:58-70) in eval."""
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    ref, prod = build_pair(kw)
    x = torch.rand(2, 15, 96, 128, generator=torch.Generator().manual_seed(6))
    for bn in ref.modules():
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(x)
    prod.load_state_dict(ref.state_dict())
    ref.eval(); prod.eval()
    with torch.no_grad():
        assert relerr(prod(x.to(DEV)), ref(x)) < 1e-3
        stacks = [prod.forward_2d(x[:, 3 * s:3 * s + 3].to(DEV)) for s in range(5)]     # b=2, t=3 like TTA
        feats = torch.cat(stacks, dim=1)
        fr = ref.forward_2d(x)
        assert feats.shape == fr.shape and relerr(feats, fr) < 1e-3
        y3 = prod.forward_3d(feats)
        yr = ref.forward_3d(fr)
        assert y3.shape == yr.shape and relerr(y3, yr) < 1e-3
        assert relerr(prod.forward_head(y3), ref.forward_head(yr)) < 1e-3


def test_frozen_encoder_long_window():
    """config 4 shape of the hot path: num_frames=33, encoder frozen (src/argus_models.py:104-110)."""
    kw = dict(orc.BASIC_CONFIG_KWARGS, num_frames=33, drop_rate=0.0, drop_path_rate=0.0)
    ref, prod = build_pair(kw)
    for m_ in (ref, prod):
        for p in m_.conv2d_encoder.parameters():
            p.requires_grad_(False)
        m_.train()
    x = torch.rand(1, 33, 64, 96, generator=torch.Generator().manual_seed(7))
    tgt = torch.tensor([[0.0, 1.0]])
    lr, gr = step(ref, x, tgt)
    lp, gp = step(prod, x.to(DEV), tgt.to(DEV))
    assert relerr(lp, lr) < 1e-3
    assert set(gp) == set(gr)
    assert grad_errors(gp, gr)[0][0] < 1e-3
    assert relerr(prod.conv2d_encoder.bn1.running_mean, ref.conv2d_encoder.bn1.running_mean, 1e-6) < 1e-3


def test_rccl_world1_gradient_allreduce_path():
    """The data-parallel code path over RCCL itself (backend 'nccl'), in a world of one: process-group init on the
    GPU, state broadcast, and the flat-gradient all-reduce issued for real (the world==1 shortcut bypassed)."""
    import os
    import socket
    import torch.distributed as dist
    from mds import parallel
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
        ref, prod = build_pair(kw)
        ref.train(); prod.train()
        parallel.data_parallel(prod, force_collective=True)
        calls = []
        sync = prod._grad_sync
        prod._grad_sync = lambda flat: (calls.append(flat.numel()), sync(flat))[1]
        x = torch.rand(1, 15, 96, 128, generator=torch.Generator().manual_seed(8))
        tgt = torch.tensor([[1.0, 0.0]])
        lr, gr = step(ref, x, tgt)
        lp, gp = step(prod, x.to(DEV), tgt.to(DEV))
        torch.cuda.synchronize()
        assert calls == [6_770_547]                      # ONE collective over the whole flat gradient arena
        assert relerr(lp, lr) < 1e-3
        assert grad_errors(gp, gr)[0][0] < 1e-3          # mean over a world of one == the local gradient
        # the default path: slices of the arena all-reduced from the communication stream while backward still runs
        prod._grad_sync = sync
        lp2, gp2 = step(prod, x.to(DEV), tgt.to(DEV))
        torch.cuda.synchronize()
        assert len(sync.buckets) >= 3 and sync.buckets[0][1] == 6_770_547 and sync.buckets[-1][0] == 0
        assert relerr(lp2, lp, 1e-6) < 1e-4     # BN running statistics moved between the two steps, logits of the same weights agree
        assert grad_errors(gp2, gr)[0][0] < 1e-3
        t = torch.ones(4, device=DEV)
        dist.all_reduce(t)
        assert t.sum().item() == 4.0
    finally:
        dist.destroy_process_group()


def test_fp16_autocast_with_gradscaler():
    """The reference's actual AMP recipe (src/argus_models.py:36,54,58): fp16 autocast + GradScaler.  fp16 autocast
    maps to bf16 storage in the kernels (fp32 range: the 65536 loss scale cannot overflow); after unscaling the
    gradients must be finite, the scaler must not skip the step, and they must match the un-scaled bf16 run."""
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    ref, prod = build_pair(kw, scale=0.03)
    prod.train()
    x = torch.rand(2, 15, 96, 128, generator=torch.Generator().manual_seed(9)).to(DEV)
    tgt = torch.tensor([[1.0, 0.0], [0.0, 1.0]], device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, g_plain = step(prod, x, tgt)
    prod.load_state_dict(ref.state_dict())
    opt = torch.optim.SGD(prod.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        logits = prod(x)
    assert logits.dtype == torch.float32
    loss = orc.sigmoid_focal_loss(logits, tgt, alpha=-1.0, gamma=1.2)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    grads = {n: p.grad.detach().clone() for n, p in prod.named_parameters()}
    assert all(torch.isfinite(g).all() for g in grads.values())
    w0 = prod.classifier.weight.detach().clone()
    scaler.step(opt); scaler.update()
    assert scaler.get_scale() == 65536.0 and not torch.equal(w0, prod.classifier.weight)      # step taken, scale kept
    # Same kernels, same bf16 storage; the power-of-two loss scale changes no rounding, so the two runs differ only by the
    # order of the fp32 atomics -> by bf16 rounding flips.  Cancellation-dominated sums (BatchNorm biases on the residual
    # stream) are noise between ANY two bf16 runs (measured: > 100 % on some), exactly as with torch's own autocast, so
    # the comparison is on the whole gradient's direction/size and on the well-conditioned head.
    a = torch.cat([grads[n].flatten() for n in g_plain]); b = torch.cat([g_plain[n].flatten() for n in g_plain])
    cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
    # (measured over builds and boxes: cosine 0.98-0.99, norm ratio within 2-6 %)
    assert cos > 0.95 and abs(a.norm().item() / b.norm().item() - 1) < 0.12, (cos, a.norm().item(), b.norm().item())
    assert relerr(grads["classifier.weight"], g_plain["classifier.weight"]) < 0.3     # measured 0.15 between two bf16 runs


@pytest.mark.parametrize("amp", [False, True])
def test_run_to_run_reproducibility(amp):
    """Every cross-block sum that feeds an activation or its gradient (BatchNorm statistics forward and backward, the
    squeeze-excite pool and its backward, GeM) is accumulated in fp64: two runs of the same step give BIT-IDENTICAL logits,
    running statistics and gradients of every BatchNorm / squeeze-excite / GeM / bias parameter, whatever order the blocks
    arrive in.  The convolution and Linear WEIGHT gradients are still fp32 atomics into the gradient arena (they feed nothing
    else): equal up to summation order."""
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    _, prod = build_pair(kw, seed=9)
    prod.train()
    x = torch.rand(2, 15, 256, 320, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    tgt = torch.tensor([[1.0, 0.0], [0.0, 1.0]], device=DEV)
    state = {k: v.clone() for k, v in prod.state_dict().items()}

    def run():
        prod.load_state_dict(state)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            return step(prod, x, tgt) + ({k: v.clone() for k, v in prod.state_dict().items() if "running" in k},)
    l1, g1, b1 = run()
    for _ in range(2):
        l2, g2, b2 = run()
        assert torch.equal(l1, l2)
        assert all(torch.equal(b1[k], b2[k]) for k in b1)
        exact = [n for n in g1 if ".bn" in n or "bn1." in n or ".se." in n or n.endswith(".bias") or n == "global_pool.p" or ".1.weight" in n or ".1.bias" in n]
        assert len(exact) > 150
        bad = [n for n in exact if not torch.equal(g1[n], g2[n]) and n != "global_pool.p"]
        assert not bad, bad[:8]
        for n in g1:      # the atomically accumulated weight gradients: same values up to fp32 summation order
            assert relerr(g2[n], g1[n], 1e-12) < (1e-2 if amp else 1e-4), n


def test_train_step_and_predictor_on_a_non_default_stream():
    """a caller that owns its HIP stream: every launch of the plan (both of its streams), the fused loss and the predictor follow
    torch's CURRENT stream; same results as on the null stream (weight gradients to atomic-order noise, the rest exactly)"""
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    _, prod = build_pair(kw)
    prod.train()
    x = torch.rand(2, 15, 128, 160, generator=torch.Generator().manual_seed(1)).to(DEV)
    tgt = torch.tensor([[1.0, 0.0], [0.0, 1.0]]).to(DEV)
    buffers0 = {n: b.detach().clone() for n, b in prod.named_buffers()}
    l0, g0 = step(prod, x, tgt)
    torch.cuda.synchronize()
    for n, b in prod.named_buffers():       # same BatchNorm running statistics at the start of the second run
        b.data.copy_(buffers0[n])
    own = torch.cuda.Stream(DEV)
    own.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(own):
        l1, g1 = step(prod, x, tgt)
        prod.eval()
        with torch.no_grad():
            e1 = prod(x).clone()
    own.synchronize()
    with torch.no_grad():
        e0 = prod(x)
    torch.cuda.synchronize()
    assert torch.equal(l0, l1)
    assert torch.equal(e0, e1)
    errs = grad_errors(g1, g0)
    assert errs[0][0] < 1e-4, errs[:3]


def test_conv_post_statistics_opt_in_matches_the_separate_reduce_passes(monkeypatch):
    """MDS_FUSE_CONV_POST=1 (opt-in: measured slower): the BatchNorm-backward sums of the first 3x3 layer, the stem and
    two edge-residual projections ride on the 3x3 data gradients above them (k_c3.hip store waves, mds_poststat_t PLAIN / MASK /
    SILU).  Same weights, same window (one 15 x 736 x 1280 window: the layers are above the kernel's size bar), same DropPath
    masks: four bn_bwd_reduce launches fewer, every parameter gradient within bf16 noise of the default schedule's."""
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.2)
    ref = fill_deterministic(orc.MultiDimStacker(**kw), 7, scale=0.05)
    x = torch.rand(1, 15, 736, 1280, generator=torch.Generator().manual_seed(5)).to(DEV)
    tgt = torch.tensor([[0.0, 1.0]], device=DEV)
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("MDS_FUSE_CONV_POST", flag)
        prod = mds.MultiDimStacker(**kw)
        prod.load_state_dict(ref.state_dict())
        prod = prod.to(DEV).train()
        torch.manual_seed(11)                         # the DropPath masks come from torch's generator
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = prod(x)
        orc.sigmoid_focal_loss(logits.float(), tgt, alpha=-1.0, gamma=1.2).backward()
        torch.cuda.synchronize()
        plan = next(p for pool in prod._cache.plans.values() for p in pool if p.kind == "full" and p.need_grad)
        nred = sum(1 for seg in ("b2d", "b3d", "bhead") for name, *_ in plan.bound[seg] if name == "bn_bwd_reduce")
        out[flag] = (logits.detach().float().cpu(), {n: p.grad.detach().float().cpu() for n, p in prod.named_parameters()}, nred)
    assert out["0"][2] - out["1"][2] == 4, (out["0"][2], out["1"][2])
    assert torch.equal(out["0"][0], out["1"][0])                              # the forward does not change
    top = max(g.norm().item() for g in out["0"][1].values())
    worst = max((((out["1"][1][n] - g).norm() / max(g.norm().item(), 1e-4 * top)).item(), n) for n, g in out["0"][1].items())
    # (worst: the stem's weight gradient, 4e-2 - its dy is formed from g = u * silu'(z) that the fused form has rounded to bf16 once
    #  more; the same tensor's error against the fp32 oracle is ~0.2 in either schedule: tests/test_fullsize_gpu.py)
    assert worst[0] < 6e-2, worst


def test_handoff_event_flags_do_not_change_the_weight_gradients(monkeypatch):
    """the ~71 hand-offs to the weight-gradient stream use events without the system-scope fence
    (hipEventDisableTiming | hipEventDisableSystemFence); with default events (MDS_EVENT_FLAGS=0) the same step must give the
    same gradients bit for bit where the kernels are deterministic (the BatchNorm / SE / bias gradients: fp64 slot sums) and within
    atomic-order noise elsewhere - a hand-off that let a weight gradient read its operands early shows up as a gross mismatch"""
    kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
    ref = fill_deterministic(orc.MultiDimStacker(**kw), 9, scale=0.05)
    x = torch.rand(2, 15, 256, 384, generator=torch.Generator().manual_seed(6)).to(DEV)
    tgt = torch.tensor([[0.0, 1.0], [1.0, 0.0]], device=DEV)
    out = {}
    for flags in ("default", "0"):
        if flags == "0":
            monkeypatch.setenv("MDS_EVENT_FLAGS", "0")
        prod = mds.MultiDimStacker(**kw)
        prod.load_state_dict(ref.state_dict())
        prod = prod.to(DEV).train()
        for _ in range(2):                               # the second step runs with every event already created
            prod.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = prod(x)
            orc.sigmoid_focal_loss(logits.float(), tgt, alpha=-1.0, gamma=1.2).backward()
        torch.cuda.synchronize()
        plan = next(p for pool in prod._cache.plans.values() for p in pool if p.kind == "full" and p.need_grad)
        out[flags] = ({n: p.grad.detach().float().cpu() for n, p in prod.named_parameters()}, getattr(plan, "_ext", None) and plan._ext.flags)
    assert out["default"][1] in (0x20000002, 0x2, 0x0) and out["0"][1] == 0
    top = max(g.norm().item() for g in out["default"][0].values())
    for n, g in out["default"][0].items():
        d = (out["0"][0][n] - g).norm().item() / max(g.norm().item(), 1e-4 * top)
        assert d < 1e-3, (n, d)
        if n.endswith(".bias") or "bn" in n:
            assert torch.equal(out["0"][0][n], g), n
