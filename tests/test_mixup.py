"""mds_mixup (csrc/k_mix.hip) and mds.augment.TimmMixup.

Three layers, each compared bit for bit (int32 views: a contracted multiply-add is a 1-ulp effect):
  1. the reference's own src/mixup.py, recorded in tests/golden/mixup_ref.npz (make_golden_mixup.py), pins the restatement in
     tests/mixup_host.py and - through the product's host-side job list - the numpy implementation of the header's arithmetic;
  2. the kernel against that numpy implementation, on the simulator and on the GPU, every buffer guard-banded;
  3. the class against the restatement under the same np.random seed: batch, target and the generator's state afterwards.
"""
import numpy as np
import pytest
import torch

import mixup_host as mh
from backends import be, knobs  # noqa: F401
from mds import cabi
from mds.augment import TimmMixup

F32 = np.float32
MODES = ("batch", "elem", "pair")


def bits(a):
    a = a.detach().cpu().contiguous() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=F32))
    assert a.dtype == torch.float32
    return a.view(torch.int32)


def assert_bits(got, want, msg=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (msg, g.shape, w.shape)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, f"{msg}: {bad.shape[0]} of {g.numel()} values differ in their bits, first at {bad[0].tolist()}"


def config_kwargs(row):
    ma, ca, lo, hi = (float(v) for v in row)
    return dict(mixup_alpha=ma, cutmix_alpha=ca, cutmix_minmax=None if np.isnan(lo) else (lo, hi))


CONFIGS = [(0.4, 0.0, None), (0.0, 1.0, None), (0.4, 1.0, None), (0.0, 0.0, (0.2, 0.6))]


def test_header_constants():
    assert (cabi.MDS_MIX_NONE, cabi.MDS_MIX_BLEND, cabi.MDS_MIX_CUT) == (mh.NONE, mh.BLEND, mh.CUT)
    assert cabi.MDS_MIX_MAX_PAIRS == 32 and cabi.MDS_VERSION >= 139
    assert ("mds_mixup", "const mds_mixup_args* a, mds_stream_t stream") in cabi.LONG_FUNCS


# ================================================================================================ 1. the recorded reference
def test_fixture_settings_are_the_tested_ones(golden):
    ref = golden("mixup_ref")
    assert [tuple(config_kwargs(r).values()) for r in ref["configs"]] == CONFIGS
    assert ref["x"].shape == (4, 3, 12, 16)


def test_restated_mixup_target_matches_the_reference(golden):
    ref = golden("mixup_ref")
    target = torch.from_numpy(ref["target"])
    assert_bits(mh.mixup_target(target, 2, float(ref["target.scalar.lam"]), 0.1), ref["target.scalar.out"], "scalar lam")
    assert_bits(mh.mixup_target(target, 2, torch.from_numpy(ref["target.column.lam"]), 0.1), ref["target.column.out"], "(B, 1) lam")
    # the header's target arithmetic: a Python-float lam gives oml = fl32(1. - lam), an fp32 lam gives oml = fl32(1) - lam
    lam = float(ref["target.scalar.lam"])
    jobs = [mh.job(mh.NONE, lam, 1. - lam)] * 4
    _, t = mh.apply_jobs(np.zeros((4, 1, 1, 1), F32), jobs, ref["target"], 0.1 / 2, 1. - 0.1 + 0.1 / 2)
    assert_bits(t, ref["target.scalar.out"], "numpy, scalar lam")
    col = ref["target.column.lam"][:, 0]
    jobs = [mh.job(mh.NONE, l, F32(1) - l) for l in col]
    _, t = mh.apply_jobs(np.zeros((4, 1, 1, 1), F32), jobs, ref["target"], 0.1 / 2, 1. - 0.1 + 0.1 / 2)
    assert_bits(t, ref["target.column.out"], "numpy, (B, 1) lam")


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_params_per_elem_draws_match_the_reference(golden, ci):
    ref = golden("mixup_ref")
    kw = dict(prob=0.7, switch_prob=0.5, mode="elem", **config_kwargs(ref["configs"][ci]))
    for cls in (mh.TimmMixup, TimmMixup):
        np.random.seed(100 + ci)
        lam, cut = cls(**kw)._params_per_elem(6)
        assert lam.dtype == np.float32 and np.array_equal(lam, ref[f"elem.{ci}.lam"]) and np.array_equal(cut, ref[f"elem.{ci}.cut"]), cls
        assert np.random.rand() == float(ref[f"elem.{ci}.next"]), f"{cls}: a different number of draws"


def class_jobs(mix, shape):
    """the product's host-side job list in the numpy implementation's form (no launch)"""
    return [mh.job(m, lam, oml, box) for m, lam, oml, box in mix._jobs(shape[0], shape[2], shape[3])]


@pytest.mark.parametrize("ci", range(4))
@pytest.mark.parametrize("mode", MODES)
def test_restatement_and_numpy_implementation_match_the_recorded_calls(golden, mode, ci):
    ref = golden("mixup_ref")
    kw = dict(prob=1.0, switch_prob=0.5, mode=mode, label_smoothing=0.1, num_classes=2, **config_kwargs(ref["configs"][ci]))
    key = f"call.{mode}.{ci}"
    seed = int(ref[key + ".seed"])
    np.random.seed(seed)
    x, t = mh.TimmMixup(**kw)(torch.from_numpy(ref["x"]).clone(), torch.from_numpy(ref["target"]).clone())
    assert_bits(x, ref[key + ".x"], "restatement, batch")
    assert_bits(t, ref[key + ".t"], "restatement, target")
    assert np.random.rand() == float(ref[key + ".next"])
    np.random.seed(seed)
    jobs = class_jobs(TimmMixup(**kw), ref["x"].shape)
    assert np.random.rand() == float(ref[key + ".next"])
    xn, tn = mh.apply_jobs(ref["x"], jobs, ref["target"], 0.1 / 2, 1. - 0.1 + 0.1 / 2)
    assert_bits(xn, ref[key + ".x"], "numpy implementation, batch")
    assert_bits(tn, ref[key + ".t"], "numpy implementation, target")


# ================================================================================================ 2. the kernel
TOUT_FILL = -7.0      # what target_out holds before a launch: rows the launch does not own keep it


def make_args(be, xbuf, jobs, tbuf=None, obuf=None, C=0, off_value=0.0, on_value=1.0, pair0=0, npairs=None, **over):
    B, T, H, W = xbuf.shape if xbuf is not None else over.pop("shape")
    npairs = B // 2 - pair0 if npairs is None else npairs
    kw = dict(B=B, T=T, H=H, W=W, x=xbuf, pair0=pair0, npairs=npairs, target=tbuf, target_out=obuf, C=C, off_value=off_value, on_value=on_value)
    kw.update(over)
    args = cabi.make("mds_mixup_args", **kw)
    for k in range(max(0, min(npairs, cabi.MDS_MIX_MAX_PAIRS))):
        for slot, s in ((args.lo[k], pair0 + k), (args.hi[k], B - 1 - (pair0 + k))):
            if 0 <= s < len(jobs):
                jb = jobs[s]
                slot.mode, slot.lam, slot.oml = jb["mode"], float(jb["lam"]), float(jb["oml"])
                slot.yl, slot.yh, slot.xl, slot.xh = jb["box"]
    return args


def data(shape, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    target = torch.rand(shape[0], C, generator=g) if C else None
    if C:
        target[:, 0] = (target[:, 0] < 0.5).float()       # hard labels next to soft ones
    return x, target


def run_kernel(be, shape, jobs, C=2, smoothing=0.1, num_classes=2, arena=False, launches=None):
    """one or more launches over guarded buffers; every intermediate state is compared with the numpy implementation"""
    x0, target = data(shape, C)
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    names = ("x", "target", "target_out") if C else ("x",)
    with be.arena(*names) if arena else _Null():
        xbuf = be.out(shape, fill=x0, name="x")
        tbuf = be.t(target, name="target") if C else None
        obuf = be.out((shape[0], C), fill=TOUT_FILL, name="target_out") if C else None
    assert xbuf.data_ptr() % 32 == 16 or (arena and xbuf.data_ptr() % 16 == 4)
    xn, tn = x0.numpy(), (np.full((shape[0], C), TOUT_FILL, F32) if C else None)
    for pair0, npairs in launches or [(0, shape[0] // 2)]:
        be.call("mixup", make_args(be, xbuf, jobs, tbuf, obuf, C, off_value, on_value, pair0, npairs))
        be.sync()
        xn, tn = mh.apply_jobs(xn, jobs, target.numpy() if C else None, off_value, on_value, pair0, npairs, target_out=tn)
        assert_bits(xbuf, xn, f"batch after pairs {pair0}..{pair0 + npairs - 1}")
        if C:
            assert_bits(obuf, tn, f"target after pairs {pair0}..{pair0 + npairs - 1}")
            assert_bits(tbuf, target, "the input target changed")
    return x0, xbuf


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def blend(lam):
    return mh.job(mh.BLEND, lam, F32(1) - F32(lam))


def cut(box, lam=0.62):
    return mh.job(mh.CUT, lam, F32(1) - F32(lam), box)


NOJOB = mh.job()


def scenarios(H, W):
    """name -> jobs of samples 0..3; the pairs are (0, 3) and (1, 2)"""
    return {
        "blend_blend": [blend(0.3), blend(0.55), blend(0.1), blend(0.8)],
        "none_blend": [NOJOB, blend(0.37), NOJOB, blend(0.9)],
        "none_none": [NOJOB] * 4,
        "blend_cut": [blend(0.3), cut((0, H, 0, W), 0.0), blend(0.45), cut((2, 7, 3, 13))],
        "cut_interior_odd_edges": [cut((1, 9, 3, 13)), cut((3, 4, 5, 6)), cut((2, 8, 1, W - 1)), cut((1, 9, 3, 13))],
        "cut_whole_image": [cut((0, H, 0, W), 0.0)] * 4,
        "cut_empty": [cut((4, 4, 2, 9), 1.0), cut((0, 0, 0, 0), 1.0), cut((H, H, W, W), 1.0), cut((2, 5, 7, 7), 1.0)],
        "cut_borders": [cut((0, 3, 5, 11)), cut((2, 8, 0, 5)), cut((1, H - 1, W - 3, W)), cut((H - 2, H, 1, W - 1))],
        "cut_disjoint_boxes": [cut((0, 2, 0, 3)), NOJOB, cut((5, 6, 8, 12)), cut((H - 3, H, W - 5, W))],
    }


SCENARIOS = list(scenarios(10, 20))


@pytest.mark.parametrize("place", ["w20", "w20_arena", "w18", "w18_arena"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_kernel_matches_the_header_arithmetic(be, name, place):
    """B=4, T=3, H=10: W=20 takes 16-byte vectors (payload at 16 mod 32), the arena placement (4 mod 16) and W=18 (rows that
    are no 16-byte multiples) take the guarded scalar path; box edges off the 4-column grid take it inside a vector launch"""
    W = 20 if place.startswith("w20") else 18
    shape = (4, 3, 10, W)
    jobs = scenarios(10, W)[name]
    x0, xbuf = run_kernel(be, shape, jobs, arena=place.endswith("arena"))
    for s, jb in enumerate(jobs):       # (what the numpy comparison already implies, said once more in the issue's words)
        if jb["mode"] == mh.NONE or name == "cut_empty":
            assert_bits(xbuf[s], x0[s], f"sample {s} has nothing to do and must keep its bits")
    if name == "none_blend":
        assert_bits(xbuf[1], x0[1] * F32(0.37) + x0[2] * (F32(1) - F32(0.37)), "the partner of an untouched sample mixes its original values")


@pytest.mark.parametrize("C", [2, 15])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_kernel_targets(be, C, smoothing):
    run_kernel(be, (4, 3, 10, 20), scenarios(10, 20)["blend_cut"], C=C, smoothing=smoothing, num_classes=C)


def test_kernel_targets_of_untouched_images(be):
    """every job NONE (a batch-mode draw of lam = 1): no image is touched, the target rows are still smoothed"""
    run_kernel(be, (4, 3, 10, 20), [NOJOB] * 4, C=2, smoothing=0.1)


def test_kernel_without_target(be):
    run_kernel(be, (4, 3, 10, 20), scenarios(10, 20)["blend_cut"], C=0)


def test_kernel_one_pair(be):
    run_kernel(be, (2, 3, 10, 20), [blend(0.7), cut((1, 9, 3, 13))])


def test_kernel_two_launches_leave_each_others_pairs_alone(be):
    """B=6: pairs 0, 1 first, pair 2 second; run_kernel compares the whole batch and the whole target_out after each launch,
    the rows of the other launch's pairs included"""
    jobs = [blend(0.2), cut((1, 9, 3, 13)), blend(0.6), blend(0.35), blend(0.5), cut((0, 10, 4, 8))]
    run_kernel(be, (6, 3, 10, 20), jobs, launches=[(0, 2), (2, 1)])


@pytest.mark.parametrize("T", [3, 7])
def test_kernel_grid_stride_loop(be, T):
    """MDS_KNOB_STREAM_BLOCKS = 1: one block per pair; at T=7 a pair has 350 four-column items for 256 threads, so the stride
    loop takes a second trip"""
    with knobs(be, {cabi.MDS_KNOB_STREAM_BLOCKS: 1}):
        run_kernel(be, (4, T, 10, 20), scenarios(10, 20)["blend_blend"])
        ls = be.launches("mixup_kernel")
        assert ls is None or [(l.gx, l.gy) for l in ls] == [(1, 2)], ls


def test_kernel_refusals(be):
    shape = (4, 3, 10, 20)
    x0, target = data(shape, 2)
    xbuf, tbuf, obuf = be.out(shape, fill=x0), be.t(target), be.out((4, 2), fill=TOUT_FILL)
    jobs = scenarios(10, 20)["blend_cut"]
    ok = dict(tbuf=tbuf, obuf=obuf, C=2)

    def refused(args, word):
        assert be.rc("mixup", args) == cabi.MDS_ERR_BAD_ARG
        assert word in be.lib.dll.mds_last_error().decode(), be.lib.dll.mds_last_error()

    refused(make_args(be, xbuf, jobs, **ok, B=3), "B = 3")
    refused(make_args(be, xbuf, jobs, **ok, B=0), "B = 0")
    refused(make_args(be, xbuf, jobs, **ok, npairs=0), "npairs")
    refused(make_args(be, xbuf, jobs, **ok, B=128, npairs=cabi.MDS_MIX_MAX_PAIRS + 1), "npairs")
    refused(make_args(be, xbuf, jobs, **ok, pair0=1, npairs=2), "pairs")
    refused(make_args(be, xbuf, jobs, **ok, pair0=-1, npairs=1), "pairs")
    for box in [(0, 11, 0, 20), (0, 10, 0, 21), (-1, 4, 0, 4), (0, 4, -1, 4), (5, 4, 0, 4), (0, 4, 9, 8)]:
        refused(make_args(be, xbuf, [cut(box)] + jobs[1:], **ok), "box")
    refused(make_args(be, xbuf, jobs[:3] + [mh.job(3)], **ok), "mode")
    refused(make_args(be, xbuf, [mh.job(-1)] + jobs[1:], **ok), "mode")
    refused(make_args(be, None, jobs, **ok, shape=shape), "null")
    refused(make_args(be, xbuf, jobs, tbuf=tbuf, obuf=None, C=2), "target")
    refused(make_args(be, xbuf, jobs, tbuf=tbuf, obuf=obuf, C=0), "target")
    refused(make_args(be, xbuf, jobs, tbuf=tbuf, obuf=tbuf, C=2), "overlaps")
    be.sync()
    assert_bits(xbuf, x0, "a refused call launched something")
    assert_bits(obuf, np.full((4, 2), TOUT_FILL, F32), "a refused call launched something")


# ================================================================================================ 3. the class
SHAPE = (4, 3, 12, 16)


def run_class(be, kw, seed, shape=SHAPE, C=2):
    """the restatement on the CPU and the class on the backend under the same seed -> (input, restated, got) + checks"""
    x0, target = data(shape, C, seed=3)
    target = target.view(shape[0], C)
    np.random.seed(seed)
    xr, tr = mh.TimmMixup(**kw)(x0.clone(), target.clone())
    state_r = np.random.get_state()
    xbuf, tbuf = be.out(shape, fill=x0, name="x"), be.t(target, name="target")
    mix = TimmMixup(**kw)
    if be.name == "emu":
        mix._lib = be.lib
    np.random.seed(seed)
    xg, tg = mix(xbuf, tbuf)
    state_g = np.random.get_state()
    be.sync()
    assert xg is xbuf, "the batch is mixed in place and handed back"
    assert_bits(xg, xr, "batch")
    assert tg.shape == target.shape and tg.data_ptr() != tbuf.data_ptr()
    assert_bits(tg, tr, "target")
    assert_bits(tbuf, target, "the caller's target changed")
    assert state_r[0] == state_g[0] and np.array_equal(state_r[1], state_g[1]) and state_r[2:] == state_g[2:], "np.random advanced differently"
    return x0, xr


@pytest.mark.parametrize("cfg", CONFIGS, ids=["mixup", "cutmix", "both", "minmax"])
@pytest.mark.parametrize("mode", MODES)
def test_class_matches_the_restatement(be, mode, cfg):
    kw = dict(mixup_alpha=cfg[0], cutmix_alpha=cfg[1], cutmix_minmax=cfg[2], prob=1.0, switch_prob=0.5, mode=mode, label_smoothing=0.1, num_classes=2)
    x0, xr = run_class(be, kw, seed=11)
    assert not torch.equal(x0, xr), "prob = 1: this draw mixes"


# prob = 0.5, settings "both": the samples that a seed leaves UNMIXED (lam == 1), from the restatement's draws.  batch mode draws
# once for the whole batch: seeds 0 and 3 give a non-mixing draw, seeds 1, 2 and 5 a mixing one.  elem draws per sample, pair per
# pair (mirrored onto the upper half): most of their seeds hold both kinds within one batch.
PROB_HALF = {
    "batch": {0: [0, 1, 2, 3], 1: [], 2: [], 3: [0, 1, 2, 3], 5: []},
    "elem": {0: [0, 1], 1: [1], 2: [3], 3: [2, 3], 5: [1, 2]},
    "pair": {0: [1, 2], 1: [1, 2], 2: [0, 1, 2, 3], 3: [0, 3], 5: []},
}


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("mode", MODES)
def test_class_with_prob_one_half(be, mode, seed):
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.5, switch_prob=0.5, mode=mode, label_smoothing=0.1, num_classes=2)
    x0, xr = run_class(be, kw, seed)
    unmixed = [s for s in range(4) if torch.equal(x0[s], xr[s])]
    assert unmixed == PROB_HALF[mode][seed], (mode, seed, unmixed)


def test_prob_one_half_seeds_hold_both_kinds():
    for mode, table in PROB_HALF.items():
        assert any(len(v) > 0 for v in table.values()) and any(len(v) < 4 for v in table.values()), mode       # unmixed and mixed samples
    for mode in ("batch", "pair"):      # (whole batches of either kind as well)
        assert any(len(v) == 4 for v in PROB_HALF[mode].values()) and any(len(v) == 0 for v in PROB_HALF[mode].values()), mode


def test_class_targets_keep_the_callers_shape(be):
    """target (B, 3, 5): flattened to (B, 15) for the launch, handed back as (B, 3, 5); batch mode, whose scalar lam lets the
    reference take a target of any rank"""
    x0, target = data(SHAPE, 15, seed=5)
    target = target.view(4, 3, 5)
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, mode="batch", label_smoothing=0.1, num_classes=15)
    np.random.seed(21)
    xr, tr = mh.TimmMixup(**kw)(x0.clone(), target.clone())
    mix = TimmMixup(**kw)
    if be.name == "emu":
        mix._lib = be.lib
    np.random.seed(21)
    xg, tg = mix(be.out(SHAPE, fill=x0), be.t(target))
    be.sync()
    assert tg.shape == (4, 3, 5)
    assert_bits(xg, xr, "batch")
    assert_bits(tg, tr, "target")


def test_class_rng_argument_leaves_the_global_generator_alone(be):
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, mode="pair", label_smoothing=0.1, num_classes=2)
    x0, target = data(SHAPE, 2, seed=3)
    np.random.seed(33)
    xr, tr = mh.TimmMixup(**kw)(x0.clone(), target.clone())
    np.random.seed(1)
    before = np.random.get_state()
    mix = TimmMixup(rng=np.random.RandomState(33), **kw)
    if be.name == "emu":
        mix._lib = be.lib
    xg, tg = mix(be.out(SHAPE, fill=x0), be.t(target))
    be.sync()
    assert np.array_equal(before[1], np.random.get_state()[1]) and before[2] == np.random.get_state()[2]
    assert_bits(xg, xr, "batch")
    assert_bits(tg, tr, "target")


def test_class_more_than_64_samples_takes_one_launch_per_32_pairs(be):
    shape = (66, 1, 2, 8)
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=2)
    be.reset_launches()
    run_class(be, kw, seed=4, shape=shape)
    ls = be.launches("mixup_kernel")
    assert ls is None or [l.gy for l in ls] == [32, 1], ls


def test_class_refuses_what_it_cannot_mix_in_place(be):
    mix = TimmMixup(mixup_alpha=0.4)
    mix._lib = be.lib if be.name == "emu" else None
    dev = be.device
    x, t = torch.zeros(4, 3, 12, 16, device=dev), torch.zeros(4, 2, device=dev)
    with pytest.raises(AssertionError, match="Batch size should be even"):
        mix(x[:3].contiguous(), t[:3])
    with pytest.raises(cabi.MdsError):
        mix(x.double(), t)
    with pytest.raises(cabi.MdsError):
        mix(x[:, :, :, ::2], t)
    with pytest.raises(cabi.MdsError):
        mix(x[:, 0], t)
    with pytest.raises(cabi.MdsError):
        TimmMixup(mixup_alpha=0.4)(torch.zeros(4, 3, 12, 16), torch.zeros(4, 2))       # a CPU batch without the simulator: no eager fallback
    with pytest.raises(AssertionError):
        TimmMixup(cutmix_minmax=(0.2, 0.4, 0.6))


def test_class_keeps_timms_attribute_names():
    m = TimmMixup(mixup_alpha=0.3, cutmix_alpha=0.0, cutmix_minmax=(0.2, 0.6), prob=0.9, switch_prob=0.4, mode="pair", correct_lam=False,
                  label_smoothing=0.05, num_classes=7)
    got = (m.mixup_alpha, m.cutmix_alpha, m.cutmix_minmax, m.mix_prob, m.switch_prob, m.label_smoothing, m.num_classes, m.mode, m.correct_lam, m.mixup_enabled)
    assert got == (0.3, 1.0, (0.2, 0.6), 0.9, 0.4, 0.05, 7, "pair", False, True)
    d = TimmMixup()
    assert (d.mixup_alpha, d.cutmix_alpha, d.cutmix_minmax, d.mix_prob, d.switch_prob, d.mode, d.correct_lam, d.label_smoothing, d.num_classes) == \
        (1., 0., None, 1.0, 0.5, "batch", True, 0.1, 1000)
