"""MultiDimStacker.eval_se_fusion: in inference plans the pooling depthwise launch also computes the squeeze-excite gate
(mds_se_tail_t) - one se_fc_fwd launch fewer per inverted-residual block, 2D and 3D.  Independent of eval_fusion: all four
combinations are planned, run and compared with the oracle; only the gate's producer changes, so fused and unfused outputs of
the same weights agree far below the bars eval_fusion is held to."""
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
from test_eval_fusion import KW, _emu, _conditioned_pair, relerr

COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (eval_fusion, eval_se_fusion)


@pytest.fixture(autouse=True, scope="module")
def _leave_the_allocator_as_found():
    """the GPU cases of this file allocate (and free) full-size tensors: give the blocks back to the driver afterwards, so
    that later test files start from the caching allocator they would have had without this one"""
    yield
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _ops(plan, seg):
    return [(name, sorted(kw)) for name, kw in plan.segs[seg]]


def _names(plan, seg):
    return [name for name, _ in plan.segs[seg]]


def _set(m, a, se):
    m.eval_fusion, m.eval_se_fusion = a, se


def test_eval_2d_plan_loses_the_sixteen_se_fc_launches():
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    x = torch.rand(2, 3, 64, 96)
    plans = {}
    with torch.no_grad():
        for a, se in COMBOS:
            _set(prod, a, se)
            plans[a, se] = prod._plan(x, "2d", 2, 3, 64, 96, False)
    assert len({id(p) for p in plans.values()}) == 4, "the flag is part of the plan-cache key"
    off, on, both = plans[False, False], plans[False, True], plans[True, True]
    assert on.eval_se_fusion and not on.eval_fusion and not off.eval_se_fusion
    assert _names(off, "f2d").count("se_fc_fwd") == 16
    assert len(on.segs["f2d"]) == len(off.segs["f2d"]) - 16
    assert len(plans[True, False].segs["f2d"]) == len(off.segs["f2d"]) - 16
    assert len(both.segs["f2d"]) == len(off.segs["f2d"]) - 32
    for p in (on, both):
        assert "se_fc_fwd" not in _names(p, "f2d")
        tails = [kw for name, kw in p.segs["f2d"] if name == "dw_fwd" and kw.get("se")]
        assert len(tails) == 16 and all(kw["pool"] is not None for kw in tails)
        assert len({id(kw["se"]["ticket"]) for kw in tails}) == 1 and p._se_ticket.numel >= 2
        # every gate a projection's prologue reads is written by a depthwise launch
        written = {id(kw["se"]["gate"]) for kw in tails}
        read = [id(kw["pro"]["gate"]) for name, kw in p.segs["f2d"] if name == "pw_fwd" and kw["pro"].get("gate") is not None]
        assert len(read) == 16 and set(read) == written
    assert len([kw for name, kw in both.segs["f2d"] if name == "dw_fwd" and kw.get("se") and kw.get("expand")]) == 16
    # the FC weights and the packed w2t stay in the weight-dependent prefix (refresh_weights / stale)
    w2 = {id(blk.se.conv_expand.weight) for blk in prod.conv2d_encoder.modules() if hasattr(blk, "se")}
    assert len({id(p) for p in on.weight_tensors()} & w2) == 16


def test_eval_3d_tail_plan_loses_one_se_fc_per_block():
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    f = torch.rand(1, 5, prod.num_3d_features, 4, 6)
    nblk = len([b for b in prod.modules() if isinstance(b, mds.structure.InvertedResidual3dP)])
    with torch.no_grad():
        off = prod._plan(f, "tail", 1, 15, 4, 6, False)
        prod.eval_se_fusion = True
        on = prod._plan(f, "tail", 1, 15, 4, 6, False)
    assert nblk > 0 and _names(off, "f3d").count("se_fc_fwd") == nblk
    assert "se_fc_fwd" not in _names(on, "f3d") and len(on.segs["f3d"]) == len(off.segs["f3d"]) - nblk
    assert len([kw for name, kw in on.segs["f3d"] if name == "dw_fwd" and kw.get("se") and kw["kt"] == 3]) == nblk
    assert _ops(on, "fhead") == _ops(off, "fhead")


def test_blocks_without_the_fused_pool_keep_their_op_list(monkeypatch):
    monkeypatch.setenv("MDS_EVAL_POOL", "0")
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    x = torch.rand(1, 3, 64, 96)
    with torch.no_grad():
        off = prod._plan(x, "2d", 1, 3, 64, 96, False)
        prod.eval_se_fusion = True
        on = prod._plan(x, "2d", 1, 3, 64, 96, False)
    assert on is not off and _ops(on, "f2d") == _ops(off, "f2d") and _names(on, "f2d").count("se_fc_fwd") == 16


@pytest.mark.parametrize("kind,shape", [("2d", (1, 3, 64, 96)), ("tail", None)])
@pytest.mark.parametrize("training,need_grad", [(True, True), (False, True), (True, False)])
def test_training_and_grad_plans_do_not_change(training, need_grad, kind, shape):
    prod = mds.MultiDimStacker(**KW).train(training)
    prod._lib = _emu()
    x = torch.rand(*shape) if shape else torch.rand(1, prod.num_stacks, prod.num_3d_features, 4, 6)
    T = 3 if shape else prod.num_stacks * prod.stack_size
    plans = []
    for flag in (False, True):
        prod.eval_se_fusion = flag
        plans.append(prod._plan(x, kind, 1, T, x.shape[-2], x.shape[-1], need_grad))
    assert plans[1] is not plans[0] and not plans[1].eval_se_fusion
    for seg in plans[0].segs:
        assert _ops(plans[0], seg) == _ops(plans[1], seg), seg


def test_the_33_frame_tail_keeps_its_op_list():
    """stacks of 11 slices have no pooling depthwise kernel (mds_dw_fwd: kt == 3 pools at T == 5 only): nothing to hang the tail on"""
    prod = mds.MultiDimStacker(**dict(KW, num_frames=33)).eval()
    prod._lib = _emu()
    f = torch.rand(1, prod.num_stacks, prod.num_3d_features, 4, 6)
    with torch.no_grad():
        off = prod._plan(f, "tail", 1, 33, 4, 6, False)
        prod.eval_se_fusion = True
        on = prod._plan(f, "tail", 1, 33, 4, 6, False)
    assert on is not off and on.eval_se_fusion
    for seg in off.segs:
        assert _ops(off, seg) == _ops(on, seg), seg


def test_flag_survives_copies_and_is_not_state():
    m = mds.MultiDimStacker(**KW)
    assert m.eval_se_fusion is False
    m.eval_se_fusion = True
    assert copy.deepcopy(m).eval_se_fusion is True and copy.deepcopy(m).eval_fusion is False
    assert pickle.loads(pickle.dumps(m)).eval_se_fusion is True
    assert not any("fusion" in k for k in m.state_dict())


def test_a_refused_launch_zeroes_the_se_tickets():
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    prod.eval_se_fusion = True
    x = torch.rand(1, 3, 64, 96)
    with torch.no_grad():
        prod.forward_2d(x)
        plan = next(pl for p in prod._cache.plans.values() for pl in p if pl.eval_se_fusion)
    plan._se_ticket.tensor.fill_(3)          # what an interrupted launch could leave behind
    with pytest.raises(mds.cabi.MdsError):
        plan._failed(-1, "dw_fwd")
    assert int(plan._se_ticket.tensor.abs().sum()) == 0


def test_module_parity_emu():
    x = torch.rand(1, 15, 48, 40, generator=torch.Generator().manual_seed(1))      # odd sizes down the pyramid
    ref, prod = _conditioned_pair(x, "cpu", _emu())
    with torch.no_grad():
        want_l, want_f = ref(x), ref.forward_2d(x[:, :3])
        out = {}
        for a, se in COMBOS:
            _set(prod, a, se)
            out[a, se] = (prod(x), prod.forward_2d(x[:, :3]))
    for (a, se), (l, f) in out.items():
        assert relerr(l, want_l) < 1e-3 and relerr(f, want_f) < 1e-3, (a, se)        # the bar of test_eval_fusion.test_module_parity_emu
    for a in (False, True):
        dl, df = relerr(out[a, True][0], out[a, False][0]), relerr(out[a, True][1], out[a, False][1])
        print(f"[eval_se_fusion emu] eval_fusion={a}: logits {dl:.3e} features {df:.3e} against the plan without the tail")
        assert dl < 2e-4 and df < 2e-4
    plans = [pl for p in prod._cache.plans.values() for pl in p if pl.eval_se_fusion]
    assert any(kw.get("se") for pl in plans for name, kw in pl.segs["f2d"] if name == "dw_fwd")
    assert any(kw.get("se") for pl in plans for name, kw in pl.segs["f3d"] if name == "dw_fwd")


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
    sp = StreamPredictor(prod, frame_size=size, eval_se_fusion=True)
    prod.eval_se_fusion = True
    sm = StreamPredictor(prod, frame_size=size)                     # None: follows the module
    so = StreamPredictor(prod, frame_size=size, eval_se_fusion=False)
    refs, outs = [], []
    for index in range(30):
        frame = new_frame()
        pr, _ = rp.predict(frame, index)
        pp, _ = sp.predict(frame, index)
        pm, _ = sm.predict(frame, index)
        po, _ = so.predict(frame, index)
        assert (pr is None) == (pp is None)
        if pr is not None:
            refs.append(pr); outs.append(pp.float())
            assert torch.equal(pp, pm)
            assert (pp.float() - po.float()).abs().max().item() < 1e-5
    prod.eval_se_fusion = False
    assert len(refs) == 2
    lref, lg = torch.logit(torch.stack(refs).double()), torch.logit(torch.stack(outs).double())
    assert (lg - lref).abs().max().item() < 1e-3 * lref.abs().max().item() + 1e-4
    for p, want in ((sp, True), (sm, True), (so, False)):
        assert any(kw.get("se") for name, kw in p.plans[1]["p2d"][0].segs["f2d"] if name == "dw_fwd") is want
        assert any(kw.get("se") for name, kw in p.plans[1]["ptail"][0].segs["f3d"] if name == "dw_fwd") is want
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_module_parity_fullsize_gpu(dt):
    """one 15 x 736 x 1280 window, every flag combination: against the oracle (fp32) and against the plan without the tail"""
    torch.set_num_threads(min(32, torch.get_num_threads()))
    x = torch.rand(1, 15, 736, 1280, generator=torch.Generator().manual_seed(5))
    ref, prod = _conditioned_pair(x, "cuda:0")
    xd = x.cuda()
    out = {}
    with torch.no_grad():
        want = ref(x) if dt == "f32" else None
        prod.compute_dtype = "f32"
        lf, ff = prod(xd).clone(), prod.forward_2d(xd[:, :3]).clone()      # the plain fp32 plan
        prod.compute_dtype = dt
        for a, se in COMBOS:
            _set(prod, a, se)
            out[a, se] = (prod(xd).clone(), prod.forward_2d(xd[:, :3]).clone())
    torch.cuda.synchronize()
    l0, f0 = out[False, False]
    for a, se in COMBOS[1:]:
        l1, f1 = out[a, se]
        print(f"[eval_se_fusion gpu {dt}] eval_fusion={a} eval_se_fusion={se}: logits {relerr(l1, l0):.3e} features {relerr(f1, f0):.3e} "
              f"against the plain plan; tail alone: logits {relerr(l1, out[a, False][0]):.3e} features {relerr(f1, out[a, False][1]):.3e}")
        if dt == "f32":
            assert relerr(l1, want) < 1e-3
            assert relerr(l1, l0) < 2e-4 and relerr(f1, f0) < 2e-4
        else:
            assert relerr(l1, lf) <= 1.5 * relerr(l0, lf) + 5e-3, (relerr(l1, lf), relerr(l0, lf))
            assert relerr(f1, ff) <= 1.5 * relerr(f0, ff) + 5e-3, (relerr(f1, ff), relerr(f0, ff))


@pytest.mark.gpu
@pytest.mark.parametrize("a", [False, True])
@pytest.mark.parametrize("tta", [False, True])
def test_predictor_at_the_real_frame_size_gpu(tta, a):
    """720 x 1280 uint8 frames padded to 736 x 1280, fp32, eval_se_fusion=True with and without eval_fusion: frame by frame
    against the reference's predictor logic on the oracle, then predict_stream with 8 frames per pass and 3 lanes"""
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
    sp = StreamPredictor(prod, frame_size=size, tta=tta, eval_fusion=a, eval_se_fusion=True)
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
    ss = StreamPredictor(prod, frame_size=size, tta=tta, eval_fusion=a, eval_se_fusion=True)
    res = list(ss.predict_stream((f.cuda() for f in frames), 0, chunk=8, lanes=3))
    torch.cuda.synchronize()
    assert [pp is None for pp, _ in res] == [i < 28 for i in range(30)]
    ls = torch.logit(torch.stack([pp.float().cpu() for pp, _ in res[28:]]).double())
    err = (ls - lref).abs().max().item()
    assert err < 1e-3 * lref.abs().max().item() + 1e-4, ("predict_stream 8 x 3", err, lref)
    assert any(kw.get("se") for name, kw in sp.plans[1]["p2d"][0].segs["f2d"] if name == "dw_fwd")
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
    sp = StreamPredictor(prod, frame_size=(64, 32), use_graphs=False, eval_se_fusion=True)
    for i in range(30):
        p_old, _ = sp.predict(frames[i], i)
    assert p_old is not None
    prod.load_state_dict(other.state_dict())          # in place: data pointers unchanged, versions bumped
    p_new, _ = sp.predict(frames[30], 30)
    fresh = model(src.state_dict())
    sf = StreamPredictor(fresh, frame_size=(64, 32), use_graphs=False, eval_se_fusion=True)
    for i in range(30):
        sf.predict(frames[i], i)
    fresh.load_state_dict(other.state_dict())
    p_want, _ = sf.predict(frames[30], 30)
    assert not torch.equal(p_new.cpu(), p_old.cpu())
    assert torch.allclose(p_new.cpu().float(), p_want.cpu().float(), rtol=1e-5, atol=1e-6)
    # a write to one block's conv_expand alone shows in the next frame's new stack: the tail reads it through its packed [R][C]
    # copy only (no se_fc_fwd is left to read the parameter itself)
    with torch.no_grad():
        blk = next(b for b in prod.conv2d_encoder.modules() if hasattr(b, "se"))
        blk.se.conv_expand.weight.mul_(-3.0)
    p_flip, _ = sp.predict(frames[31], 31)
    p_keep, _ = sf.predict(frames[31], 31)
    assert not torch.equal(p_flip.cpu(), p_keep.cpu()), "a write to conv_expand between two frames was not picked up"
    sp.close(); sf.close()
