"""x.grad from forward() / forward_2d(): the stem's data gradient wired through the planner and both ways into autograd (the registered
operator; the one autograd bridge, for forward() with MDS_CUSTOM_OP=0 and for forward_2d()), on the
kernel simulator (CPU) and - marked gpu - on the gfx950 library, against the float64 oracle."""
import copy
import os
import subprocess
import sys
import warnings

import pytest
import torch

from oracle import multidim_stacker_ref as orc
from det_init import fill_deterministic
import mds

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
SHAPE = {"emu": (1, 15, 48, 40), "gpu": (1, 15, 128, 128)}
KW0 = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
TGT = torch.tensor([[1.0, 0.0]])


@pytest.fixture(params=BACKENDS)
def bk(request):
    return request.param


def _dev(bk):
    return torch.device("cpu" if bk == "emu" else "cuda:0")


def _pair(bk, kw, seed=3, scale=0.05):
    ref = fill_deterministic(orc.MultiDimStacker(**kw), seed, scale=scale)
    prod = mds.MultiDimStacker(**kw)
    prod.load_state_dict(ref.state_dict())
    if bk == "emu":
        from hipemu.loader import load_emulator
        prod._lib = load_emulator()
    else:
        prod = prod.to("cuda:0")
    return ref, prod


def _x(bk, seed=1):
    return torch.rand(*SHAPE[bk], generator=torch.Generator().manual_seed(seed))


def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def _loss(logits, dev):
    return orc.sigmoid_focal_loss(logits, TGT.to(dev).to(logits.dtype), alpha=-1.0, gamma=1.2)


def _xgrad(model, x, autocast=None):
    """x.grad and the parameter gradients of one step"""
    model.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    ctx = torch.autocast(x.device.type, dtype=torch.bfloat16) if autocast else torch.autocast(x.device.type, enabled=False)
    with ctx:
        logits = model(x)
    _loss(logits.float() if autocast else logits, x.device).backward()
    return x.grad, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _force_masks(ref, prod, B, S, seed=5):
    """the same DropPath / dropout masks on both sides (tests/test_module_gpu.py, test_stochastic_layers_with_shared_masks_fp32)"""
    g = torch.Generator().manual_seed(seed)
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


def _realistic_running_stats(ref, prod, x):
    """eval mode on the deterministic fill's arbitrary running statistics blows up (tests/test_module_emu.py): take this batch's"""
    for bn in ref.modules():
        if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            bn.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(x)
    prod.load_state_dict(ref.state_dict())


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_input_grad_fp32_vs_float64_oracle(bk, mode):
    """bar: the one tests/test_module_gpu.py applies to parameter gradients, |err| <= 1e-3 * max|ref|"""
    kw = dict(orc.BASIC_CONFIG_KWARGS) if mode == "train" else KW0
    ref, prod = _pair(bk, kw)
    x = _x(bk)
    if mode == "train":
        ref.train(); prod.train()
        _force_masks(ref, prod, x.shape[0], x.shape[1] // 3)
    else:
        _realistic_running_stats(ref, prod, x)
        ref.eval(); prod.eval()
    ref64 = copy.deepcopy(ref).double()
    xr, _ = _xgrad(ref64, x.double())
    xg, gp = _xgrad(prod, x.to(_dev(bk)))
    assert xg is not None and xg.shape == x.shape and xg.dtype == torch.float32
    e = relerr(xg, xr)
    print(f"x.grad fp32 {mode} {bk}: rel err {e:.3e} (max |ref| {xr.abs().max().item():.3e})")
    assert e < 1e-3
    assert "conv2d_encoder.conv_stem.weight" in gp


def test_input_grad_bf16_within_2x_of_torch_bf16(bk):
    """the bar of a bf16 result is twice the error of torch's own bf16-autocast run of the oracle on that tensor"""
    ref, prod = _pair(bk, KW0, scale=0.03)
    ref.train(); prod.train()
    x = _x(bk, 2)
    x32, _ = _xgrad(copy.deepcopy(ref).double(), x.double())
    x16, _ = _xgrad(ref, x, autocast=True)
    xp, _ = _xgrad(prod, x.to(_dev(bk)), autocast=True)
    e_ref, e_prod = relerr(x16, x32), relerr(xp, x32)
    print(f"x.grad bf16 {bk}: rel err {e_prod:.3e}, torch bf16 autocast {e_ref:.3e}")
    assert e_prod <= 2 * e_ref, (e_prod, e_ref)


def test_forward_2d_alone_returns_the_input_gradient(bk):
    ref, prod = _pair(bk, KW0)
    ref.train(); prod.train()
    x = _x(bk, 7)
    ref64 = copy.deepcopy(ref).double()
    xr = x.double().requires_grad_(True)
    fr = ref64.forward_2d(xr)
    up = torch.randn(fr.shape, generator=torch.Generator().manual_seed(8))
    fr.backward(up.double())
    xp = x.to(_dev(bk)).requires_grad_(True)
    fp = prod.forward_2d(xp)
    fp.backward(up.to(_dev(bk)))
    assert xp.grad is not None and xp.grad.shape == x.shape
    e = relerr(xp.grad, xr.grad)
    print(f"forward_2d x.grad {bk}: rel err {e:.3e}")
    assert e < 1e-3


_CHILD = r"""
import sys, torch
sys.path[:0] = {path!r}
from oracle import multidim_stacker_ref as orc
from det_init import fill_deterministic
import mds
from mds import module
assert not module.USE_CUSTOM_OP
kw = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
ref = fill_deterministic(orc.MultiDimStacker(**kw), 3, scale=0.05)
prod = mds.MultiDimStacker(**kw)
prod.load_state_dict(ref.state_dict())
if {bk!r} == "emu":
    from hipemu.loader import load_emulator
    prod._lib = load_emulator()
    dev = "cpu"
else:
    prod = prod.to("cuda:0"); dev = "cuda:0"
prod.train()
x = torch.rand(*{shape!r}, generator=torch.Generator().manual_seed(1)).to(dev).requires_grad_(True)
orc.sigmoid_focal_loss(prod(x), torch.tensor([[1.0, 0.0]], device=dev), alpha=-1.0, gamma=1.2).backward()
torch.save(x.grad.cpu(), {out!r})
"""


def test_both_operator_paths_give_the_same_input_gradient(bk, tmp_path):
    """the registered operator here, torch.autograd.Function (MDS_CUSTOM_OP=0, read at import) in a fresh child process"""
    from mds import module
    assert module.USE_CUSTOM_OP
    _, prod = _pair(bk, KW0)
    prod.train()
    xg, _ = _xgrad(prod, _x(bk).to(_dev(bk)))
    out = str(tmp_path / "xg.pt")
    code = _CHILD.format(path=[p for p in sys.path if p], bk=bk, shape=SHAPE[bk], out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MDS_CUSTOM_OP="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    other = torch.load(out)
    # same plan, same launches; the statistics behind BatchNorm backward are summed by fp64 atomics (order-independent to 1e-16)
    assert relerr(other, xg) < 1e-5


@pytest.mark.parametrize("det", [True, False])
def test_parameter_gradients_do_not_depend_on_the_input_gradient(bk, det):
    _, prod = _pair(bk, KW0)
    prod.train()
    prod.deterministic = det
    state = copy.deepcopy(prod.state_dict())
    x = _x(bk, 4).to(_dev(bk))
    prod.zero_grad(set_to_none=True)
    _loss(prod(x), x.device).backward()
    g0 = {n: p.grad.detach().clone() for n, p in prod.named_parameters()}
    prod.load_state_dict(state)
    xg, g1 = _xgrad(prod, x)
    assert xg is not None
    for n in g0:
        if det:
            assert torch.equal(g1[n], g0[n]), n
        else:      # fp32 atomics on the weight gradients: equal up to the order of the sums
            assert (g1[n] - g0[n]).abs().max().item() <= 1e-4 * max(g0[n].abs().max().item(), 1e-6) + 1e-7, n


def test_plan_hygiene():
    """without x.requires_grad: the schedules of before, no stem_dgrad, no dx buffer; with it: exactly one more launch, its own cache key"""
    _, prod = _pair("emu", KW0)
    prod.train()
    x = torch.rand(1, 15, 32, 32)
    off = prod._plan(x, "full", 1, 15, 32, 32, True)
    on = prod._plan(x, "full", 1, 15, 32, 32, True, input_grad=True)
    assert on is not off and len(prod._cache.plans) == 2
    assert prod._plan(x, "full", 1, 15, 32, 32, True, input_grad=True) is on and prod._plan(x, "full", 1, 15, 32, 32, True) is off
    names = lambda p: {s: [n for n, _ in ops] for s, ops in p.segs.items()}
    a, b = names(off), names(on)
    assert not off.input_grad and off.dx is None and not any("stem_dgrad" in v for v in a.values())
    assert sum(v.count("stem_dgrad") for v in b.values()) == 1 and b["b2d"][-1] == "stem_dgrad"
    assert b["b2d"][:-1] == a["b2d"] and all(a[s] == b[s] for s in a if s != "b2d")
    assert on.nbytes - off.nbytes == 4 * x.numel()                 # the fp32 dx buffer, nothing else
    # a plan without a backward, or of a frozen encoder, never has it
    assert not prod._plan(x, "full", 1, 15, 32, 32, False, input_grad=True).input_grad
    cost = dict(zip(b["b2d"], on.costs["b2d"]))["stem_dgrad"]
    assert cost[0] == 4 * x.numel() + 4 * 5 * 16 * 16 * 32 and cost[1] == 2 * 27 * 32 * (x.numel() // 3) // 4


def test_frozen_encoder_warns_once_and_leaves_no_input_gradient(bk):
    _, prod = _pair(bk, KW0)
    prod.train()
    for p in prod.conv2d_encoder.parameters():
        p.requires_grad_(False)
    x = _x(bk).to(_dev(bk))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(2):
            xi = x.clone().requires_grad_(True)
            prod(xi).sum().backward()
            assert xi.grad is None
    hits = [w for w in rec if issubclass(w.category, RuntimeWarning) and "input gradient" in str(w.message)]
    assert len(hits) == 1, [str(w.message) for w in rec]
    assert prod.classifier.weight.grad is not None


def test_compile_fullgraph_with_input_grad():
    import torch._dynamo as dynamo
    _, prod = _pair("emu", KW0)
    prod.train()
    x = torch.rand(1, 15, 32, 64, generator=torch.Generator().manual_seed(21))
    state = copy.deepcopy(prod.state_dict())
    xe, ge = _xgrad(prod, x)
    prod.load_state_dict(state)
    dynamo.reset()
    cm = torch.compile(prod, fullgraph=True, backend="aot_eager")
    xc, gc = _xgrad(cm, x)
    assert xc is not None and torch.equal(xc, xe)
    for n in ge:
        assert torch.equal(gc[n if n in gc else "_orig_mod." + n], ge[n]), n
