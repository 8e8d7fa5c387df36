"""MultiDimStacker.eval_er_fusion: in inference plans the four edge-residual blocks of the b0 encoder run their 3x3 expansion
and their 1x1 projection in ONE launch (mds_project_t, k_c3p.hip) - the mid-wide tensor between them is never stored and the
plan loses four pw_fwd launches.  Independent of eval_fusion and eval_se_fusion: all eight combinations are planned; the module
and the stream predictor stay on the oracle, and fused against unfused stays inside the bars eval_fusion is held to."""
import copy
import itertools
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

COMBOS = list(itertools.product((False, True), repeat=3))      # (eval_fusion, eval_se_fusion, eval_er_fusion)


@pytest.fixture(autouse=True, scope="module")
def _leave_the_allocator_as_found():
    """the GPU cases of this file allocate (and free) full-size tensors: give the blocks back to the driver afterwards"""
    yield
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _ops(plan, seg):
    return [(name, sorted(kw)) for name, kw in plan.segs[seg]]


def _set(m, a, se, er):
    m.eval_fusion, m.eval_se_fusion, m.eval_er_fusion = a, se, er


def _pairs(plan):
    """pw_fwd ops that read the mid-wide buffer a plain conv_fwd op wrote (the output of a launch with a projection tail is a
    block output: the next block's expansion may read it)"""
    conv_out = {id(kw["y"]) for name, kw in plan.segs["f2d"] if name == "conv_fwd" and not kw.get("project")}
    return [kw for name, kw in plan.segs["f2d"] if name == "pw_fwd" and id(kw["x"]) in conv_out]


def _fused(plan):
    return [kw for name, kw in plan.segs["f2d"] if name == "conv_fwd" and kw.get("project")]


def test_eval_plan_loses_the_four_projection_launches():
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    x = torch.rand(2, 3, 64, 96)
    plans = {}
    with torch.no_grad():
        for c in COMBOS:
            _set(prod, *c)
            plans[c] = prod._plan(x, "2d", 2, 3, 64, 96, False)
    assert len({id(p) for p in plans.values()}) == 8, "the flag is part of the plan-cache key"
    off, on = plans[False, False, False], plans[False, False, True]
    assert on.eval_er_fusion and not on.eval_fusion and not on.eval_se_fusion and not off.eval_er_fusion
    # 75 -> 71 launches per 2D pass; 59 -> 55 with either other switch, 43 -> 39 with both (one more op than launches in each
    # plan: the eval-BatchNorm table is part of the prefix, not of the segment)
    n = {c: len(p.segs["f2d"]) for c, p in plans.items()}
    for a, se in itertools.product((False, True), repeat=2):
        assert n[a, se, True] == n[a, se, False] - 4, (a, se)
        assert n[a, se, False] == n[False, False, False] - 16 * (int(a) + int(se))
    assert len(_pairs(off)) == 4 and not _fused(off)
    blocks = [b for b in prod.conv2d_encoder.modules() if hasattr(b, "conv_exp")]
    assert len(blocks) == 4
    for c, p in plans.items():
        if not c[2]:
            assert len(_pairs(p)) == 4 and not _fused(p), c
            continue
        f = _fused(p)
        assert len(f) == 4 and not _pairs(p), c
        for kw, blk in zip(f, blocks):
            assert kw["Cin"] == blk.cin and kw["Cout"] == blk.mid and kw["project"]["cout"] == blk.cout and kw["is"] == blk.stride
            assert (kw["residual"] is not None) == blk.has_skip and (kw["residual"] is None or kw["residual"] is kw["x"])
            assert kw["stats"] is None and kw["epi"]["mode"] == 2
        # the fused launch's output is what the next op reads: no buffer of the mid width is left between the two
        outs = {id(kw["y"]) for kw in f}
        read = {id(kw.get("x")) for name, kw in p.segs["f2d"]} | {id(kw["expand"]["x"]) for name, kw in p.segs["f2d"] if kw.get("expand")}
        assert outs <= read
    # the packed projection filters (and the 3x3 filters) are part of the weight-dependent prefix (refresh_weights / stale)
    ws = {id(b.conv_pwl.weight) for b in blocks} | {id(b.conv_exp.weight) for b in blocks}
    assert len({id(t) for t in on.weight_tensors()} & ws) == 8
    bns = {id(b.bn1.weight) for b in blocks} | {id(b.bn2.weight) for b in blocks}
    assert len({id(t) for t in on.weight_tensors()} & bns) == 8


@pytest.mark.parametrize("training,need_grad", [(True, True), (False, True), (True, False)])
def test_training_and_grad_plans_do_not_change(training, need_grad):
    prod = mds.MultiDimStacker(**KW).train(training)
    prod._lib = _emu()
    x = torch.rand(1, 3, 64, 96)
    plans = []
    for flag in (False, True):
        prod.eval_er_fusion = flag
        plans.append(prod._plan(x, "2d", 1, 3, 64, 96, need_grad))
    assert plans[1] is not plans[0] and not plans[1].eval_er_fusion
    for seg in plans[0].segs:
        assert _ops(plans[0], seg) == _ops(plans[1], seg), seg


def test_plans_without_output_transforms_do_not_change(monkeypatch):
    monkeypatch.setenv("MDS_EVAL_EPI", "0")
    prod = mds.MultiDimStacker(**KW).eval()
    prod._lib = _emu()
    x = torch.rand(1, 3, 64, 96)
    with torch.no_grad():
        off = prod._plan(x, "2d", 1, 3, 64, 96, False)
        prod.eval_er_fusion = True
        on = prod._plan(x, "2d", 1, 3, 64, 96, False)
    assert on is not off and not on.eval_er_fusion
    for seg in off.segs:
        assert _ops(off, seg) == _ops(on, seg), seg


def test_flag_survives_copies_and_is_not_state():
    m = mds.MultiDimStacker(**KW)
    assert m.eval_er_fusion is False
    m.eval_er_fusion = True
    c = copy.deepcopy(m)
    assert c.eval_er_fusion is True and c.eval_fusion is False and c.eval_se_fusion is False
    assert pickle.loads(pickle.dumps(m)).eval_er_fusion is True
    assert not any("fusion" in k for k in m.state_dict())
    old = pickle.loads(pickle.dumps(m))
    del old.__dict__["eval_er_fusion"]                 # a module pickled before the attribute existed: off
    old._lib = _emu()
    with torch.no_grad():
        assert not old.eval()._plan(torch.rand(1, 3, 64, 96), "2d", 1, 3, 64, 96, False).eval_er_fusion


def test_module_parity_emu():
    x = torch.rand(1, 15, 48, 40, generator=torch.Generator().manual_seed(1))      # odd sizes down the pyramid
    ref, prod = _conditioned_pair(x, "cpu", _emu())
    with torch.no_grad():
        want_l, want_f = ref(x), ref.forward_2d(x[:, :3])
        l0, f0 = prod(x), prod.forward_2d(x[:, :3])
        prod.eval_er_fusion = True
        l1, f1 = prod(x), prod.forward_2d(x[:, :3])
        _set(prod, True, True, True)
        l3, f3 = prod(x), prod.forward_2d(x[:, :3])
    print(f"[eval_er_fusion emu] oracle: logits {relerr(l1, want_l):.3e} features {relerr(f1, want_f):.3e}; unfused plan: logits "
          f"{relerr(l1, l0):.3e} features {relerr(f1, f0):.3e}; all three on, oracle: logits {relerr(l3, want_l):.3e} features {relerr(f3, want_f):.3e}")
    assert relerr(l1, want_l) < 1e-3 and relerr(f1, want_f) < 1e-3          # the bars eval_fusion is held to
    assert relerr(l1, l0) < 2e-4 and relerr(f1, f0) < 2e-4
    assert relerr(l3, want_l) < 1e-3 and relerr(f3, want_f) < 1e-3
    plans = [pl for p in prod._cache.plans.values() for pl in p if pl.eval_er_fusion]
    assert plans and all(len(_fused(pl)) == 4 for pl in plans if pl.kind in ("2d", "full"))


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
    sp = StreamPredictor(prod, frame_size=size, eval_er_fusion=True)
    prod.eval_er_fusion = True
    sm = StreamPredictor(prod, frame_size=size)                     # None: follows the module
    so = StreamPredictor(prod, frame_size=size, eval_er_fusion=False)
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
            assert (pp.float() - po.float()).abs().max().item() < 1e-3
    assert prod.eval_er_fusion is True                  # a predictor with its own setting restores the module's
    prod.eval_er_fusion = False
    assert len(refs) == 2
    lref, lg = torch.logit(torch.stack(refs).double()), torch.logit(torch.stack(outs).double())
    assert (lg - lref).abs().max().item() < 1e-3 * lref.abs().max().item() + 1e-4
    for p, want in ((sp, True), (sm, True), (so, False)):
        assert (len(_fused(p.plans[1]["p2d"][0])) == 4) is want
        p.close()
    sq = StreamPredictor(prod, frame_size=size, eval_er_fusion=True)
    sq.predict(new_frame(), 0)
    assert prod.eval_er_fusion is False                 # the predictor's setting does not leak into the module
    sq.close()


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
        prod.eval_er_fusion = True
        l1, f1 = prod(xd).clone(), prod.forward_2d(xd[:, :3]).clone()
        _set(prod, True, True, True)
        l3 = prod(xd).clone()
    torch.cuda.synchronize()
    print(f"[eval_er_fusion gpu {dt}] against the unfused plan: logits {relerr(l1, l0):.3e} features {relerr(f1, f0):.3e}; against the fp32 plan: "
          f"fused {relerr(l1, lf):.3e} / {relerr(f1, ff):.3e} unfused {relerr(l0, lf):.3e} / {relerr(f0, ff):.3e}")
    if dt == "f32":
        assert relerr(l1, want) < 1e-3 and relerr(l3, want) < 1e-3
        assert relerr(l1, l0) < 2e-4 and relerr(f1, f0) < 2e-4
    else:
        # bf16 storage: both forms round the activated expansion to bf16 once, but sum in different orders; against the fp32
        # plan the fused one must be as good as the unfused one
        assert relerr(l1, lf) <= 1.5 * relerr(l0, lf) + 5e-3, (relerr(l1, lf), relerr(l0, lf))
        assert relerr(f1, ff) <= 1.5 * relerr(f0, ff) + 5e-3, (relerr(f1, ff), relerr(f0, ff))
        assert relerr(l3, lf) <= 1.5 * relerr(l0, lf) + 5e-3, (relerr(l3, lf), relerr(l0, lf))


@pytest.mark.gpu
@pytest.mark.parametrize("tta", [False, True])
def test_predictor_at_the_real_frame_size_gpu(tta):
    """720 x 1280 uint8 frames padded to 736 x 1280, fp32, eval_er_fusion=True: frame by frame against the reference's predictor
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
    sp = StreamPredictor(prod, frame_size=size, tta=tta, eval_er_fusion=True)
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
    ss = StreamPredictor(prod, frame_size=size, tta=tta, eval_er_fusion=True)
    res = list(ss.predict_stream((f.cuda() for f in frames), 0, chunk=8, lanes=3))
    torch.cuda.synchronize()
    assert [pp is None for pp, _ in res] == [i < 28 for i in range(30)]
    ls = torch.logit(torch.stack([pp.float().cpu() for pp, _ in res[28:]]).double())
    err = (ls - lref).abs().max().item()
    assert err < 1e-3 * lref.abs().max().item() + 1e-4, ("predict_stream 8 x 3", err, lref)
    assert len(_fused(sp.plans[1]["p2d"][0])) == 4 and prod.eval_er_fusion is False
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
    sp = StreamPredictor(prod, frame_size=(64, 32), use_graphs=False, eval_er_fusion=True)
    for i in range(30):
        p_old, _ = sp.predict(frames[i], i)
    assert p_old is not None
    prod.load_state_dict(other.state_dict())          # in place: data pointers unchanged, versions bumped
    p_new, _ = sp.predict(frames[30], 30)
    # a fresh predictor on the new weights, fed the old-weight features of the four older stacks the same way
    fresh = model(src.state_dict())
    sf = StreamPredictor(fresh, frame_size=(64, 32), use_graphs=False, eval_er_fusion=True)
    for i in range(30):
        sf.predict(frames[i], i)
    fresh.load_state_dict(other.state_dict())
    p_want, _ = sf.predict(frames[30], 30)
    assert not torch.equal(p_new.cpu(), p_old.cpu())
    assert torch.allclose(p_new.cpu().float(), p_want.cpu().float(), rtol=1e-5, atol=1e-6)
    # a write to ONE projection filter of an edge-residual block alone (BatchNorms untouched) shows in the next frame's new
    # stack: the fused launch reads it through its packed copy
    with torch.no_grad():
        blk = next(b for b in prod.conv2d_encoder.modules() if hasattr(b, "conv_exp"))
        blk.conv_pwl.weight.mul_(-1.0)
    p_flip, _ = sp.predict(frames[31], 31)
    p_keep, _ = sf.predict(frames[31], 31)
    assert not torch.equal(p_flip.cpu(), p_keep.cpu()), "a write to a projection filter between two frames was not picked up"
    sp.close(); sf.close()
