"""MultiDimStacker.eval_fusion: the 2D inverted-residual blocks of inference plans expand their input inside the depthwise
launch (mds_expand_t).  The plan loses the 16 expansion launches of the b0 encoder and nothing else changes; the module and
the stream predictor stay on the oracle."""
import copy
import pickle

import pytest
import torch

from backends import be  # noqa: F401
from det_init import fill_deterministic
from oracle import multidim_stacker_ref as orc
import mds
from mds.predict import StreamPredictor
from test_predictor import RefPredictor

KW = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)


def _emu():
    from hipemu.loader import load_emulator
    return load_emulator()


def _conditioned_pair(x, device, lib=None, seed=6):
    """oracle + product with running statistics taken from x (momentum 1): a contractive eval network (the raw deterministic
    fill blows the eval logits up to ~1e5)"""
    ref = fill_deterministic(orc.MultiDimStacker(**KW), seed, scale=0.02)
    for bn in ref.modules():
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(x)
    ref.eval()
    prod = mds.MultiDimStacker(**KW)
    prod.load_state_dict(ref.state_dict())
    prod = prod.to(device).eval()
    if lib is not None:
        prod._lib = lib
    return ref, prod


def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-12)).item()


def _ops(plan, seg="f2d"):
    return [(name, sorted(k for k in kw if k != "expand")) for name, kw in plan.segs[seg]]


def test_eval_plan_loses_the_sixteen_expansion_launches():
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    x = torch.rand(2, 3, 64, 96)
    with torch.no_grad():
        off = prod._plan(x, "2d", 2, 3, 64, 96, False)
        prod.eval_fusion = True
        on = prod._plan(x, "2d", 2, 3, 64, 96, False)
    assert on is not off and on.eval_fusion and not off.eval_fusion
    assert len(on.segs["f2d"]) == len(off.segs["f2d"]) - 16
    fused = [kw for name, kw in on.segs["f2d"] if name == "dw_fwd" and kw.get("expand")]
    assert len(fused) == 16
    assert all(kw["x"] is None for kw in fused)
    # no pw_fwd writes a tensor that a depthwise launch reads (the expansions are gone, not moved)
    dw_in = {id(kw["x"]) for name, kw in on.segs["f2d"] if name == "dw_fwd" and kw["x"] is not None}
    assert not [kw for name, kw in on.segs["f2d"] if name == "pw_fwd" and id(kw["y"]) in dw_in]
    # ... while the unfused plan has exactly those 16
    dw_in_off = {id(kw["x"]) for name, kw in off.segs["f2d"] if name == "dw_fwd"}
    assert len([kw for name, kw in off.segs["f2d"] if name == "pw_fwd" and id(kw["y"]) in dw_in_off]) == 16
    # the packed expansion filters are part of the weight-dependent prefix (refresh_weights / stale)
    pws = {id(blk.conv_pw.weight) for blk in prod.conv2d_encoder.modules() if hasattr(blk, "conv_pw")}
    assert len({id(p) for p in on.weight_tensors()} & pws) >= 16


@pytest.mark.parametrize("training,need_grad", [(True, True), (False, True), (True, False)])
def test_training_and_grad_plans_do_not_change(training, need_grad):
    prod = mds.MultiDimStacker(**KW).train(training)
    prod._lib = _emu()
    x = torch.rand(1, 3, 64, 96)
    plans = []
    for flag in (False, True):
        prod.eval_fusion = flag
        plans.append(prod._plan(x, "2d", 1, 3, 64, 96, need_grad))
    assert not plans[1].eval_fusion
    for seg in plans[0].segs:
        assert _ops(plans[0], seg) == _ops(plans[1], seg), seg


def test_flag_survives_copies_and_is_not_state():
    m = mds.MultiDimStacker(**KW)
    assert m.eval_fusion is False
    m.eval_fusion = True
    assert copy.deepcopy(m).eval_fusion is True
    assert pickle.loads(pickle.dumps(m)).eval_fusion is True
    assert not any("fusion" in k for k in m.state_dict())


def test_module_parity_emu():
    x = torch.rand(1, 15, 48, 40, generator=torch.Generator().manual_seed(1))      # odd sizes down the pyramid
    ref, prod = _conditioned_pair(x, "cpu", _emu())
    with torch.no_grad():
        l0, f0 = prod(x), prod.forward_2d(x[:, :3])
        prod.eval_fusion = True
        l1, f1 = prod(x), prod.forward_2d(x[:, :3])
        # the oracle bar of the unfused inference plans (split-bf16 products: ~3e-4 here for both); fused against unfused tighter
        assert relerr(l1, ref(x)) < 1e-3 and relerr(f1, ref.forward_2d(x[:, :3])) < 1e-3
        assert relerr(l1, l0) < 2e-4 and relerr(f1, f0) < 2e-4
    assert any(kw.get("expand") for p in prod._cache.plans.values() for pl in p for name, kw in pl.segs["f2d"] if name == "dw_fwd")


def test_predictor_matches_reference_logic_emu():
    lib = _emu()
    size = (96, 64)
    g = torch.Generator().manual_seed(1)
    ref = fill_deterministic(orc.MultiDimStacker(**KW), 5, scale=0.02)
    for bn in ref.modules():
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    ref.train()
    rp0 = RefPredictor(ref, size, False)

    def new_frame():
        return torch.randint(0, 256, (58, 90), generator=g).to(torch.uint8)
    with torch.no_grad():
        ref(torch.stack([torch.stack([rp0.process(new_frame()[None, None])[0, 0] for _ in range(15)]) for _ in range(4)]))
    prod = mds.MultiDimStacker(**KW)
    prod.load_state_dict(ref.state_dict())
    prod._lib = lib
    rp = RefPredictor(ref, size, False)
    sp = StreamPredictor(prod, frame_size=size, eval_fusion=True)
    refs, outs = [], []
    for index in range(30):
        frame = new_frame()
        pr, _ = rp.predict(frame, index)
        pp, _ = sp.predict(frame, index)
        assert (pr is None) == (pp is None)
        if pr is not None:
            refs.append(pr); outs.append(pp.float())
    assert len(refs) == 2 and prod.eval_fusion is False          # the predictor's setting does not leak into the module
    lref, lg = torch.logit(torch.stack(refs).double()), torch.logit(torch.stack(outs).double())
    assert (lg - lref).abs().max().item() < 1e-3 * lref.abs().max().item() + 1e-4
    assert any(kw.get("expand") for name, kw in sp.plans[1]["p2d"][0].segs["f2d"] if name == "dw_fwd")
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_module_parity_fullsize_gpu(dt):
    """one 15 x 736 x 1280 window: fused against the oracle (fp32) and against the unfused plan of the same dtype"""
    torch.set_num_threads(min(32, torch.get_num_threads()))
    x = torch.rand(1, 15, 736, 1280, generator=torch.Generator().manual_seed(5))
    ref, prod = _conditioned_pair(x, "cuda:0")
    xd = x.cuda()
    with torch.no_grad():
        want = ref(x) if dt == "f32" else None
        prod.compute_dtype = "f32"
        lf, ff = prod(xd).clone(), prod.forward_2d(xd[:, :3]).clone()      # the unfused fp32 plan
        prod.compute_dtype = dt
        l0, f0 = prod(xd).clone(), prod.forward_2d(xd[:, :3]).clone()
        prod.eval_fusion = True
        l1, f1 = prod(xd).clone(), prod.forward_2d(xd[:, :3]).clone()
    torch.cuda.synchronize()
    if dt == "f32":
        assert relerr(l1, want) < 1e-3
        assert relerr(l1, l0) < 2e-4 and relerr(f1, f0) < 2e-4
    else:
        # bf16 storage: the fused launch keeps y1 in fp32 (the unfused plan rounds it to bf16), so the two bf16 plans differ by
        # bf16 noise; against the fp32 plan the fused one must be as good as the unfused one
        assert relerr(l1, lf) <= 1.5 * relerr(l0, lf) + 5e-3, (relerr(l1, lf), relerr(l0, lf))
        assert relerr(f1, ff) <= 1.5 * relerr(f0, ff) + 5e-3, (relerr(f1, ff), relerr(f0, ff))


@pytest.mark.gpu
@pytest.mark.parametrize("tta", [False, True])
def test_predictor_at_the_real_frame_size_gpu(tta):
    """720 x 1280 uint8 frames padded to 736 x 1280, fp32, eval_fusion=True: frame by frame against the reference's predictor
    logic on the oracle, then predict_stream with 8 frames per pass and 3 lanes against the same oracle outputs"""
    g = torch.Generator().manual_seed(2)
    size = (1280, 736)
    torch.set_num_threads(min(32, torch.get_num_threads()))

    def new_frame():
        return torch.randint(0, 256, (720, 1280), generator=g).to(torch.uint8)
    ref = fill_deterministic(orc.MultiDimStacker(**KW), 6, scale=0.02)
    for bn in ref.modules():
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    ref.train()
    rp0 = RefPredictor(ref, size, tta)
    with torch.no_grad():
        ref(torch.stack([rp0.process(new_frame()[None, None])[0, 0] for _ in range(15)])[None])
    prod = mds.MultiDimStacker(**KW)
    prod.load_state_dict(ref.state_dict())
    prod = prod.to("cuda:0")
    rp = RefPredictor(ref, size, tta)
    sp = StreamPredictor(prod, frame_size=size, tta=tta, eval_fusion=True)
    refs, outs, frames = [], [], []
    for index in range(30):
        frame = new_frame()
        frames.append(frame)
        pr, _ = rp.predict(frame, index)
        pp, _ = sp.predict(frame.cuda(), index)
        assert (pr is None) == (pp is None) == (index < 28)
        if pr is not None:
            refs.append(pr); outs.append(pp.float().cpu())
    lref, lg = torch.logit(torch.stack(refs).double()), torch.logit(torch.stack(outs).double())
    assert torch.isfinite(lref).all()
    err = (lg - lref).abs().max().item()
    assert err < 1e-3 * lref.abs().max().item() + 1e-4, (err, lref)
    ss = StreamPredictor(prod, frame_size=size, tta=tta, eval_fusion=True)
    res = list(ss.predict_stream((f.cuda() for f in frames), 0, chunk=8, lanes=3))
    torch.cuda.synchronize()
    assert [pp is None for pp, _ in res] == [i < 28 for i in range(30)]
    ls = torch.logit(torch.stack([pp.float().cpu() for pp, _ in res[28:]]).double())
    err = (ls - lref).abs().max().item()
    assert err < 1e-3 * lref.abs().max().item() + 1e-4, ("predict_stream 8 x 3", err, lref)
    assert any(kw.get("expand") for name, kw in sp.plans[1]["p2d"][0].segs["f2d"] if name == "dw_fwd")
    ss.close(); sp.close()


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_weights_written_between_two_frames_are_picked_up(device):
    src = fill_deterministic(orc.MultiDimStacker(**KW), 7, scale=0.02)
    other = fill_deterministic(orc.MultiDimStacker(**KW), 8, scale=0.02)
    g = torch.Generator().manual_seed(3)
    frames = [torch.randint(0, 256, (32, 64), generator=g).to(torch.uint8) for _ in range(32)]

    def model(state):
        m = mds.MultiDimStacker(**KW)
        m.load_state_dict(state)
        m = m.to(device)
        if device == "cpu":
            m._lib = _emu()
        return m
    prod = model(src.state_dict())
    sp = StreamPredictor(prod, frame_size=(64, 32), use_graphs=False, eval_fusion=True)
    for i in range(30):
        p_old, _ = sp.predict(frames[i], i)
    assert p_old is not None
    prod.load_state_dict(other.state_dict())          # in place: data pointers unchanged, versions bumped
    p_new, _ = sp.predict(frames[30], 30)
    # a fresh predictor on the new weights, fed the old-weight features of the four older stacks the same way
    fresh = model(src.state_dict())
    sf = StreamPredictor(fresh, frame_size=(64, 32), use_graphs=False, eval_fusion=True)
    for i in range(30):
        sf.predict(frames[i], i)
    fresh.load_state_dict(other.state_dict())
    p_want, _ = sf.predict(frames[30], 30)
    assert not torch.equal(p_new.cpu(), p_old.cpu())
    assert torch.allclose(p_new.cpu().float(), p_want.cpu().float(), rtol=1e-5, atol=1e-6)
    # a write to one expansion filter alone (BatchNorms untouched) shows in the next frame's new stack: only the fused launch
    # reads that packed copy
    with torch.no_grad():
        blk = next(b for b in prod.conv2d_encoder.modules() if hasattr(b, "conv_pw"))
        blk.conv_pw.weight.mul_(-1.0)
    p_flip, _ = sp.predict(frames[31], 31)
    p_keep, _ = sf.predict(frames[31], 31)
    assert not torch.equal(p_flip.cpu(), p_keep.cpu()), "a write to an expansion filter between two frames was not picked up"
    sp.close(); sf.close()
