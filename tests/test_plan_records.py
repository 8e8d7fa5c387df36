"""The planner's backward records (mds.engine.Bwd) and the rule they protect, on the host kernel simulator: a gradient bucket
that a cut hands to `cut_hook` (the data-parallel all-reduce) is final - no launch issued after the cut adds into it."""
import pytest
import torch

from oracle import multidim_stacker_ref as orc
import mds
from mds import cabi, engine
from mds.engine import Bwd, Lazy, Plan

BWD_SEGS = ("bhead", "b3d", "b2d")      # issue order
SHAPE = (1, 15, 48, 40)


@pytest.fixture(scope="module")
def lib():
    from hipemu.loader import load_emulator
    return load_emulator()


def _module(lib, frozen):
    m = mds.MultiDimStacker(**orc.BASIC_CONFIG_KWARGS)
    m._lib = lib
    for p in m.conv2d_encoder.parameters():
        p.requires_grad_(not frozen)
    return m.train()


def _arena_ranges(plan, kw):
    """[(lo, hi)] of every buffer of a record that lies in the gradient arena: nested dicts and the `_jobs` of a table launch included"""
    out = []
    for v in kw.values():
        if isinstance(v, dict):
            out += _arena_ranges(plan, v)
        elif isinstance(v, (list, tuple)):
            for e in v:
                if isinstance(e, dict):
                    out += _arena_ranges(plan, e)
        elif isinstance(v, Lazy):
            off, root = 0, v
            while root.kind == "sub":
                off, root = off + root.off, root.parent
            if root is plan.grad_arena:
                out.append((off, off + v.numel))
    return out


@pytest.mark.parametrize("bucket", [None, 200_000, 1])
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_cut_bucket_is_final(lib, monkeypatch, dt, frozen, bucket):
    if bucket is not None:
        monkeypatch.setattr(Plan, "BUCKET_ELEMS", bucket)
    m = _module(lib, frozen)
    plan = m._plan(torch.empty(0), "full", *SHAPE, True, code=cabi.MDS_BF16 if dt == "bf16" else cabi.MDS_F32)
    numel = plan.grad_arena.numel
    assert numel == sum(p.numel() for p in m.parameters())
    # the records of the backward pass in issue order, each with its (segment, position)
    issued = [(seg, k, name, kw) for seg in BWD_SEGS for k, (name, kw) in enumerate(plan.segs[seg])]
    touched = [(seg, k, name, r) for seg, k, name, kw in issued for r in _arena_ranges(plan, kw)]
    assert touched and {seg for seg, *_ in touched} == set(BWD_SEGS)
    cuts = sorted(plan.cuts.items(), key=lambda c: (BWD_SEGS.index(c[0][0]), c[0][1]))
    if bucket == 1:          # (the smallest setting that cuts in every backward segment)
        assert {seg for (seg, _), _ in cuts} == set(BWD_SEGS)
    # the cuts tile [grad_lo, numel) from the top down without gaps
    assert cuts and cuts[0][1][1] == numel and cuts[-1][1][0] == plan.grad_lo
    assert all(a[1][0] == b[1][1] for a, b in zip(cuts, cuts[1:])) and all(lo < hi for _, (lo, hi) in cuts)
    assert plan.grad_lo == (sum(p.numel() for p in m.conv2d_encoder.parameters()) if frozen else 0)
    # once a cut is taken, nothing issued at or after it carries a buffer of the arena above the cut's lower bound
    for (cseg, ck), (lo, hi) in cuts:
        for seg, k, name, (a, b) in touched:
            after = (BWD_SEGS.index(seg), k) >= (BWD_SEGS.index(cseg), ck)
            assert not after or b <= lo, f"{name} at {seg}[{k}] carries arena[{a}:{b}] after the cut at {cseg}[{ck}] handed out [{lo}:{hi})"
    # and no backward record writes below grad_lo
    assert all(a >= plan.grad_lo for *_, (a, b) in touched)


def _closure(seg, dout, nxt_head):
    return None


def test_a_backward_record_needs_its_lower_bound():
    with pytest.raises(TypeError):
        Bwd(_closure)
    for bad in (None, -1, 1.5, "0"):
        with pytest.raises((TypeError, ValueError)):
            Bwd(_closure, bad)
    rec = Bwd(_closure, 7)
    assert (rec.lo, rec.head) == (7, None) and rec("bhead", None, None) is None


def _head_plan_with(lib, register):
    """a head plan whose builder registers one more closure the way `register` does (the chain runs in reverse: it is issued after
    the head's own closure)"""
    class Extra(Plan):
        def _build_head(self, *a):
            super()._build_head(*a)
            self._recs["head"].insert(0, register(_closure))

    return Extra(_module(lib, False), lib, torch.device("cpu"), "head", 1, 15, 2, 2, cabi.MDS_F32, True, True, True)


@pytest.mark.parametrize("register", [lambda f: Bwd(f), lambda f: Bwd(f, None), lambda f: f], ids=["no lo", "lo None", "bare function"])
def test_a_closure_registered_without_lo_fails_the_plan_build(lib, register):
    with pytest.raises((TypeError, ValueError, AttributeError)):
        _head_plan_with(lib, register)


def test_a_closure_registered_with_lo_builds(lib):
    assert _head_plan_with(lib, lambda f: Bwd(f, 0)).cuts


def test_mode_constants_are_the_headers():
    assert engine.NO_PRO == dict(mode=cabi.MDS_PRO_NONE)
    assert not [n for n in vars(engine) if n.split("_")[0] in ("PRO", "G", "POST", "EPI")]
