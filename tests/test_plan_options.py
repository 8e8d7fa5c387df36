"""The host plumbing of the engine's switches, on the host kernel simulator: PlanOptions (the five user switches as one element
of the plan-cache key), DevSwitches (the MDS_* environment, read once per plan build) and the predictor's override helper."""
import copy
import dataclasses
import types

import pytest
import torch

from oracle import multidim_stacker_ref as orc
import mds
from mds.engine import DevSwitches, PlanOptions
from mds.predict import _overridden

USER = ("eval_fusion", "eval_se_fusion", "eval_er_fusion", "deterministic", "device_rng")
# variable, field, default, [(value, parsed)]: how engine.py parsed each variable where it used to read it
ENV = [("MDS_FUSE_BN_BWD", "fuse_bn_bwd", True, [("0", False), ("1", True), ("", True), ("2", True)]),
       ("MDS_EVAL_EPI", "eval_epi", True, [("0", False), ("1", True), ("", False), ("2", False)]),
       ("MDS_SE_PARAMS_TABLE", "se_params_table", True, [("0", False), ("1", True), ("", False)]),
       ("MDS_FUSE_CONV_POST", "fuse_conv_post", False, [("0", False), ("1", True), ("", False)]),
       ("MDS_FUSE_CONV_POST_SILU", "fuse_conv_post_silu", True, [("0", False), ("1", True), ("", False)]),
       ("MDS_EVAL_POOL", "eval_pool", True, [("0", False), ("1", True), ("", False)]),
       ("MDS_SE_ACT", "se_act", False, [("0", False), ("1", True), ("", False)]),
       ("MDS_STEM_DYP", "stem_dyp", True, [("0", False), ("1", True), ("", False)]),
       ("MDS_SIDE_STREAM", "side_stream", True, [("0", False), ("1", True), ("", True)]),
       ("MDS_SIDE_EVENTS", "stop_events", True, [("stop", True), ("record", False), ("", False)]),
       ("MDS_EVENT_FLAGS", "event_flags", 0x20000002, [("0", 0), ("0x2", 2), ("2", 2), ("0x20000002", 0x20000002)]),
       ("MDS_MEMSET", "hip_memset", True, [("hip", True), ("torch", False), ("", False)])]


@pytest.fixture(scope="module")
def base():
    from hipemu.loader import load_emulator
    m = mds.MultiDimStacker(**dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.2, drop_path_rate=0.2))
    m._lib = load_emulator()
    return m


@pytest.fixture
def clean_env(monkeypatch):
    for var, *_ in ENV:
        monkeypatch.delenv(var, raising=False)
    return monkeypatch


def _plan(m, need_grad):
    return m._plan(torch.rand(1, 15, 32, 32), "full", 1, 15, 32, 32, need_grad)


def test_options_of_a_module_pickled_before_the_switches_existed(base):
    assert [f.name for f in dataclasses.fields(PlanOptions)] == list(USER) and PlanOptions() == PlanOptions(*[False] * 5)
    old = copy.deepcopy(base)
    for name in USER:
        setattr(old, name, True)
    assert PlanOptions.of(old, True, True) == PlanOptions(*[True] * 5)
    for name in USER:
        del old.__dict__[name]
    assert PlanOptions.of(old, True, True) == PlanOptions()
    assert hash(PlanOptions.of(old, True, True)) == hash(PlanOptions())


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("need_grad", [False, True])
def test_gate_table(training, need_grad):
    m = types.SimpleNamespace(**dict.fromkeys(USER, 1))      # (of() only reads attributes; any truthy value: the record holds bools)
    o = PlanOptions.of(m, training, need_grad)
    assert all(type(v) is bool for v in dataclasses.astuple(o))
    assert o.deterministic is need_grad and o.device_rng is training
    assert o.eval_fusion and o.eval_se_fusion and o.eval_er_fusion       # ungated in the key: Plan gates them with eval_epilogues
    m.deterministic = m.device_rng = False
    assert PlanOptions.of(m, True, True) == PlanOptions(True, True, True, False, False)


def test_plan_cache_keys_on_the_effective_options(base, clean_env):
    m = copy.deepcopy(base).train()
    p = _plan(m, True)
    assert _plan(m, True) is p
    (key,) = m._cache.plans
    assert sum(isinstance(e, PlanOptions) for e in key) == 1 and not any(isinstance(e, DevSwitches) for e in key)
    assert (p.eval_fusion, p.eval_se_fusion, p.eval_er_fusion, p.deterministic, p.device_rng) == (False,) * 5
    # gated away: a forward-only plan of a training module ignores `deterministic`, a plan of an eval module ignores `device_rng`
    q = _plan(m, False)
    m.deterministic = True
    assert _plan(m, False) is q and not q.deterministic
    d = _plan(m, True)
    assert d is not p and d.deterministic and _plan(m, True) is d
    m.eval()
    e = _plan(m, False)
    m.device_rng = True
    assert _plan(m, False) is e and not e.device_rng
    m.train()
    r = _plan(m, True)
    assert r is not d and r.device_rng and r.deterministic
    # the eval_* switches key a new plan in every mode (as before), and only inference plans act on them
    m.eval_fusion = True
    t = _plan(m, True)
    assert t is not r and not t.eval_fusion
    m.eval()
    f = _plan(m, False)
    assert f is not e and f.eval_fusion and not f.eval_se_fusion and not f.deterministic and not f.device_rng


@pytest.mark.parametrize("var,field,default,cases", ENV, ids=[e[0] for e in ENV])
def test_dev_switches_parse(clean_env, var, field, default, cases):
    unset = DevSwitches.from_env()
    assert unset == DevSwitches() and getattr(unset, field) == default and type(getattr(unset, field)) is type(default)
    for value, want in cases:
        clean_env.setenv(var, value)
        got = DevSwitches.from_env()
        assert getattr(got, field) == want and type(getattr(got, field)) is type(default), (var, value)
        assert dataclasses.replace(got, **{field: default}) == unset, (var, value)      # no other field moved


def test_every_field_of_dev_switches_has_a_variable():
    assert [f.name for f in dataclasses.fields(DevSwitches)] == [e[1] for e in ENV]


def test_a_plan_keeps_the_environment_it_was_built_under(base, clean_env):
    clean_env.setenv("MDS_SE_ACT", "1")
    clean_env.setenv("MDS_SIDE_EVENTS", "record")
    clean_env.setenv("MDS_FUSE_BN_BWD", "0")
    m = copy.deepcopy(base).train()
    m.compute_dtype = "bf16"
    p = _plan(m, True)
    want = dataclasses.replace(DevSwitches(), se_act=True, stop_events=False, fuse_bn_bwd=False)
    assert p.dev == want and not p.fuse_bn_bwd
    clean_env.setenv("MDS_SE_ACT", "0")
    clean_env.setenv("MDS_SIDE_EVENTS", "stop")
    clean_env.setenv("MDS_SIDE_STREAM", "0")
    assert p.dev == want and p._ext_events() is None          # the launch path reads the record, not the environment
    assert _plan(m, True) is p                                # the developer switches are not part of the key ...
    m.clear_plans()
    assert _plan(m, True).dev == dataclasses.replace(DevSwitches(), se_act=False, side_stream=False, fuse_bn_bwd=False)     # ... a new plan reads them


def test_override_helper_restores_and_removes(base):
    m = copy.deepcopy(base)
    m.compute_dtype, m.eval_fusion = "auto", True
    del m.__dict__["eval_er_fusion"]                          # a module pickled before the switch existed
    over = dict(compute_dtype="bf16", eval_fusion=False, eval_se_fusion=None, eval_er_fusion=True)
    with _overridden(m, over):
        assert (m.compute_dtype, m.eval_fusion, m.eval_se_fusion, m.eval_er_fusion) == ("bf16", False, False, True)
        m.eval_se_fusion = True                               # not overridden (None): not the helper's to restore
    assert (m.compute_dtype, m.eval_fusion, m.eval_se_fusion) == ("auto", True, True)
    assert "eval_er_fusion" not in m.__dict__ and not hasattr(m, "eval_er_fusion")
    with pytest.raises(ZeroDivisionError):
        with _overridden(m, over):
            assert m.eval_er_fusion is True and m.compute_dtype == "bf16"
            1 / 0
    assert (m.compute_dtype, m.eval_fusion) == ("auto", True) and not hasattr(m, "eval_er_fusion")
    with _overridden(m, dict.fromkeys(over)):                 # nothing to override: nothing touched
        assert m.compute_dtype == "auto" and not hasattr(m, "eval_er_fusion")
