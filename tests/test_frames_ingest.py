"""Training ingest: the frames processor (mds.frames.PadNormalizeFramesProcessor / mds_pad_normalize) and the raw uint8 source
of the augmentation pass (mds_aug_raw_t; TrainAugmentations(..., frames_processor=p)).

References, in the order of their authority:
  - tests/golden/frames_ref.npz: what the reference's own src/frames.py returns (tests/golden/make_golden_frames.py);
  - the torch expression of that file, F.pad(x, ...).to(float32) / 255.0, for the geometries the fixture does not hold;
  - the SAME launch fed buf[0] = pad + / 255 of the raw batch: existing code, held to the oracle by tests/test_augment.py.
Every comparison of a raw launch with its fp32 twin is bit for bit: the conversion is one correctly rounded division, and
everything after the load is the same code.  Inputs sit in guarded buffers whose integer guards are 0xA5 bytes: an over-read
of the raw source that is used shows up as 165 / 255 in the result.

The tile of the pass is 8 rows x 128 columns; its vector paths depend on W % 4, src_w % 4 and pad_left % 4."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backends import be  # noqa: F401
from oracle import augment_ref as aug
from mds import augment, cabi, frames

B, T = 2, 3
# name -> (h, w, H, W, fill)
GEOMS = {
    "odd_two_tiles": (21, 131, 24, 140, 0),      # pads top 1 / bottom 2, left 4 / right 5; unaligned source rows; second column tile partial
    "pad_left_2": (20, 36, 24, 40, 0),           # 4-byte groups straddle the pad edge
    "no_pad": (16, 256, 16, 256, 0),             # full vector path
    "top_only": (16, 128, 24, 128, 0),           # the real case's pattern: top 8, left 0
    "ragged": (10, 30, 13, 34, 0),               # W % 4 != 0: scalar store path
    "fill_37": (21, 131, 24, 140, 37),           # a visible pad band
}

# copied from tests/test_augment.py
STAGES = {
    "identity": dict(),
    "camera": dict(camera=dict(angle=[1.9, -2.2], translations=[[2.5, -1.0], [-3.0, 0.8]], center=[[19.5, 11.5]] * 2, scale=[[0.96, 0.96], [1.04, 1.04]])),
    "rotation": dict(rotation=-2.3),
    "crop": dict(crop=(3, 2, 33, 20)),
    "flip": dict(flip=True),
    "sharpness": dict(sharpness=0.35),
    "motion_blur": dict(motion_blur=dict(ksize=11, angle=5.5, direction=0.6)),
    "brightness": dict(brightness=1.17),
    "contrast": dict(contrast=0.83),
    "posterize": dict(posterize=3),
    "noise": dict(noise=dict(std=0.05, mean=0.0, seed=7)),
}


def _t(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.float32)


def _oracle_params(s):
    s = dict(s)
    if "camera" in s:
        s["camera"] = {k: _t(v) for k, v in s["camera"].items()}
    return s


def _pads(h, w, H, W):
    top, left = (H - h) // 2, (W - w) // 2
    return top, left, H - h - top, W - w - left


def torch_ref(x, H, W, fill=0):
    """src/frames.py as a torch expression"""
    top, left, bottom, right = _pads(x.shape[-2], x.shape[-1], H, W)
    return F.pad(x, [left, right, top, bottom], mode="constant", value=fill).to(torch.float32) / 255.0


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


_RAW = {}


def raw_batch(geom):
    """the (B, T, h, w) uint8 batch of a geometry: computed once, shared, never modified.  Every byte value occurs."""
    if geom not in _RAW:
        h, w = GEOMS[geom][:2]
        x = torch.randint(0, 256, (B, T, h, w), generator=torch.Generator().manual_seed(71), dtype=torch.uint8)
        x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
        _RAW[geom] = (x, torch_ref(x, *GEOMS[geom][2:]))
    return _RAW[geom]


def processor(be, geom, **kw):
    _, _, H, W, fill = GEOMS[geom]
    p = frames.PadNormalizeFramesProcessor((W, H), fill_value=fill, **kw)
    p._lib = be.lib if be.name == "emu" else None
    return p


# ------------------------------------------------------------------------------------------------ the stand-alone processor
def test_processor_is_bit_identical_to_the_reference_fixture(be, golden):
    g = golden("frames_ref")
    assert list(g["names"]) == ["bytes", "odd", "fill", "bytes_fill"]
    assert sorted(set(g["bytes.x"].flatten().tolist())) == list(range(256)) and int(g["fill.fill"]) == 37
    for name in g["names"]:
        x, y = torch.from_numpy(g[f"{name}.x"]), torch.from_numpy(g[f"{name}.y"])
        p = frames.get_frames_processor("pad_normalize", dict(size=tuple(int(v) for v in g[f"{name}.size"]), pad_mode="constant",
                                                             fill_value=int(g[f"{name}.fill"])))
        p._lib = be.lib if be.name == "emu" else None
        out = p(be.t(x))
        be.sync()
        assert same_bits(out, y), name
        assert same_bits(torch_ref(x, y.shape[-2], y.shape[-1], int(g[f"{name}.fill"])), y), name      # the restatement used below


def test_a_multiply_by_the_reciprocal_is_a_different_function(golden):
    """guards the fixture test against proving nothing: x * (1 / 255) in fp32 is NOT what the reference computes"""
    g = golden("frames_ref")
    x, y = torch.from_numpy(g["bytes.x"]), torch.from_numpy(g["bytes.y"])
    wrong = x.to(torch.float32) * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert not same_bits(wrong, y)
    assert int((wrong != y).sum()) == 126
    assert float((wrong - y).abs().max()) < 1e-7      # one ulp: invisible to a tolerance, visible to a bit compare


@pytest.mark.parametrize("geom", list(GEOMS))
def test_processor_equals_the_torch_expression(be, geom):
    x, ref = raw_batch(geom)
    p = processor(be, geom)
    out = p(be.t(x))                                        # (B, T, h, w): two leading dimensions
    one = p(be.t(x[1, 2]))                                  # a single (h, w) frame
    five = p(be.t(x.reshape(1, B, T, *x.shape[-2:])))       # three leading dimensions
    be.sync()
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert same_bits(out, ref) and same_bits(one, ref[1, 2]) and same_bits(five, ref[None])


def test_registry_and_signatures_follow_the_reference():
    assert list(inspect.signature(frames.PadNormalizeFramesProcessor.__init__).parameters) == ["self", "size", "pad_mode", "fill_value"]
    sig = inspect.signature(frames.PadNormalizeFramesProcessor.__init__).parameters
    assert sig["pad_mode"].default == "constant" and sig["fill_value"].default == 0
    assert list(inspect.signature(frames.get_frames_processor).parameters) == ["name", "processor_params"]
    p = frames.get_frames_processor("pad_normalize", dict(size=(40, 24)))
    assert isinstance(p, frames.PadNormalizeFramesProcessor) and (p.size, p.pad_mode, p.fill_value) == ((40, 24), "constant", 0)
    with pytest.raises(AssertionError):
        frames.get_frames_processor("resize", dict(size=(40, 24)))


# ------------------------------------------------------------------------------------------------ mds_pad_normalize, directly
def _pad_normalize_args(be, src_t, dst_t, geom, **over):
    h, w, H, W, fill = GEOMS[geom]
    top, left, _, _ = _pads(h, w, H, W)
    kw = dict(src=src_t, dst=dst_t, n=B * T, src_h=h, src_w=w, H=H, W=W, pad_top=top, pad_left=left, fill=fill)
    kw.update(over)
    return cabi.make("mds_pad_normalize_args", **kw)


@pytest.mark.parametrize("placement", ["aligned", "arena"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_pad_normalize_entry_point(be, geom, placement):
    x, ref = raw_batch(geom)
    _, _, H, W, _ = GEOMS[geom]
    if placement == "arena":          # raw batch and output at 4-byte-only addresses: byte loads / scalar stores where alignment is lost
        with be.arena("raw", "dst"):
            xs, dst = be.t(x, name="raw"), be.out((B, T, H, W), fill=-1.0, name="dst")
    else:
        xs, dst = be.t(x, name="raw"), be.out((B, T, H, W), fill=-1.0, name="dst")
    be.call("pad_normalize", _pad_normalize_args(be, xs, dst, geom))
    be.sync()
    assert same_bits(dst, ref)


# ------------------------------------------------------------------------------------------------ mds_aug_pass with a raw source
def _jobs(be, jobs):
    Job = cabi.STRUCTS["mds_aug_job"]
    arr = (Job * len(jobs))()
    for jb, d in zip(arr, jobs):
        jb.active, jb.src, jb.dst, jb.point = 1, 0, 1, 1
        for k, v in d.items():
            if isinstance(v, (list, tuple)):
                for i, e in enumerate(v):
                    getattr(jb, k)[i] = e
            else:
                setattr(jb, k, v)
    return be.t(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))


def _taps(angle, direction, stretch=1):
    """a motion-blur job; stretch = 2 spreads the taps beyond the staged halo (|dx| <= 8, |dy| <= 5): direct gathers"""
    ker = augment.motion_kernel(11, angle, direction)
    ys, xs = np.nonzero(ker)
    return dict(mode=cabi.MDS_AUG_TAPS, ntaps=len(ys), tap_dx=[(int(v) - 5) * stretch for v in xs], tap_dy=[int(v) - 5 for v in ys],
                tap_w=[float(ker[a, b]) for a, b in zip(ys, xs)])


def _mode_jobs(mode, H, W):
    """(two jobs - one per sample, both of the mode under test -, (B, T, 6) maps)"""
    maps = np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (B, T, 1))
    point = dict(bright_on=1, bright_add=0.07, contrast_on=1, contrast_mul=0.9, posterize_bits=5)
    if mode == "copy":
        return [dict(mode=cabi.MDS_AUG_COPY), dict(mode=cabi.MDS_AUG_COPY, **point)], maps
    if mode in ("warp", "warp_far"):
        # a rotation about the centre: the corners sample the pad band and beyond the frame; 45 degrees = a source box that no
        # longer fits the staging tile wherever the frame is large enough for that (direct gathers)
        deg = (7.0, -4.0) if mode == "warp" else (45.0, -40.0)
        for i in range(B):
            maps[i] = augment.TrainAugmentations.frame_maps(dict(rotation=deg[i]), T, H, W)[0]
        return [dict(mode=cabi.MDS_AUG_WARP), dict(mode=cabi.MDS_AUG_WARP, **point)], maps
    if mode == "sharp":
        return [dict(mode=cabi.MDS_AUG_SHARP, sharp_factor=0.35), dict(mode=cabi.MDS_AUG_SHARP, sharp_factor=0.8, **point)], maps
    if mode == "taps":
        return [_taps(5.5, 0.6), dict(_taps(-7.0, -1.0), **point)], maps
    assert mode == "taps_far"
    return [_taps(5.5, 0.6, stretch=2), dict(_taps(-7.0, -1.0, stretch=2), **point)], maps


def _aug_launch(be, geom_hw, jobs, maps, xf=None, raw=None):
    H, W = geom_hw
    out = be.out((B, T, H, W), fill=-1.0, name="out")      # (buf[] are activations: 16-byte aligned by the header's contract)
    jt, mp = _jobs(be, jobs), be.t(torch.from_numpy(maps))
    kw = dict(B=B, T=T, H=H, W=W, buf=[be.ptr(xf) if xf is not None else 0, be.ptr(out), 0, 0], jobs=jt, maps=mp, noise=None)
    if raw is not None:
        kw["raw"] = raw
    be.call("aug_pass", cabi.make("mds_aug_args", **kw))
    be.sync()
    return out.cpu()


def _raw_t(x, geom, **over):
    h, w, H, W, fill = GEOMS[geom]
    top, left, _, _ = _pads(h, w, H, W)
    kw = dict(u8=x, src_h=h, src_w=w, pad_top=top, pad_left=left, fill=fill)
    kw.update(over)
    return cabi.make("mds_aug_raw_t", **kw)


@pytest.mark.parametrize("mode", ["copy", "warp", "sharp", "taps", "taps_far"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_aug_pass_from_raw_equals_the_pass_from_the_padded_batch(be, geom, mode):
    x, ref = raw_batch(geom)
    H, W = GEOMS[geom][2:4]
    jobs, maps = _mode_jobs(mode, H, W)
    want = _aug_launch(be, (H, W), jobs, maps, xf=be.t(ref))                      # existing code: fp32 source
    got = _aug_launch(be, (H, W), jobs, maps, raw=_raw_t(be.t(x), geom))          # buf[0] = NULL
    assert same_bits(got, want)
    if mode == "copy":
        assert same_bits(got[0], ref[0]), "COPY without point operations is the plain pad + normalize"
    else:
        assert not same_bits(got[0], ref[0])
    # once more with the raw batch where the engine's arenas would put it: at a 4-byte-only address
    with be.arena("raw"):
        xs = be.t(x, name="raw")
    assert same_bits(_aug_launch(be, (H, W), jobs, maps, raw=_raw_t(xs, geom)), want)
    # buf[0] set as well: the jobs with src 0 still read the raw batch
    assert same_bits(_aug_launch(be, (H, W), jobs, maps, xf=be.t(torch.full_like(ref, 0.5)), raw=_raw_t(be.t(x), geom)), want)


def test_aug_pass_from_raw_with_a_source_box_beyond_the_staging_tile(be):
    """a 45-degree rotation of a 96 x 140 frame: the affine image of an 8 x 128 tile is about 100 x 100 source pixels, more than
    the 7168-float tile holds - the pass gathers directly (px), where the raw source converts per sample"""
    h, w, H, W, fill = 90, 131, 96, 140, 37
    GEOMS["far"] = (h, w, H, W, fill)
    try:
        x = torch.randint(0, 256, (B, T, h, w), generator=torch.Generator().manual_seed(72), dtype=torch.uint8)
        ref = torch_ref(x, H, W, fill)
        jobs, maps = _mode_jobs("warp_far", H, W)
        want = _aug_launch(be, (H, W), jobs, maps, xf=be.t(ref))
        assert same_bits(_aug_launch(be, (H, W), jobs, maps, raw=_raw_t(be.t(x), "far")), want)
        assert float(want[0, 0, H // 2, W // 2 - 8:W // 2 + 8].abs().max()) > 0 and float(want[0, 0, 0, 0]) == 0.0      # picture in the middle, nothing in the corner
    finally:
        del GEOMS["far"]


# ------------------------------------------------------------------------------------------------ TrainAugmentations on the raw batch
def _modules(be, geom, compose):
    _, _, H, W, _ = GEOMS[geom]
    p = processor(be, geom)
    fused = augment.TrainAugmentations((W, H), compose_geometric=compose, frames_processor=p)
    plain = augment.get_train_augmentations((W, H), compose_geometric=compose)
    for m in (fused, plain):
        m._lib = be.lib if be.name == "emu" else None
    return p, fused, plain


@pytest.mark.parametrize("compose", [False, True])
@pytest.mark.parametrize("stage", list(STAGES))
def test_every_stage_from_the_raw_batch(be, stage, compose):
    geom = "odd_two_tiles"
    x, ref = raw_batch(geom)
    _, _, H, W, _ = GEOMS[geom]
    noise = torch.randn(B, T, H, W, generator=torch.Generator().manual_seed(11))
    params = [STAGES[stage], dict()]                                  # the second sample stays untouched
    p, fused, plain = _modules(be, geom, compose)
    out = fused(be.t(x), params=params, noise=be.t(noise))
    xf = p(be.t(x))
    two_step = plain(xf, params=params, noise=be.t(noise))
    be.sync()
    assert out.shape == (B, T, H, W) and out.dtype == torch.float32
    assert same_bits(xf, ref)
    assert same_bits(out, two_step)
    assert same_bits(out[1], ref[1]), "a sample no stage fires for is the plain pad + normalize"
    want = aug.apply_reference_order(ref, [_oracle_params(s) for s in params], noise)
    if stage in ("identity", "flip", "posterize", "brightness", "contrast"):
        torch.testing.assert_close(out.cpu(), want, rtol=0, atol=1e-7)
    else:
        torch.testing.assert_close(out.cpu(), want, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("compose", [False, True])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_stage_chains_from_the_raw_batch(be, geom, compose):
    """several passes per sample (resampling slots, sharpness and motion blur through scratch), the noise generated in the kernel
    (its counter is the output element), prepared= : only the first pass of a chain reads the raw batch"""
    x, ref = raw_batch(geom)
    _, _, H, W, _ = GEOMS[geom]
    params = [dict(rotation=2.0, crop=(1, 1, W - 3, H - 2), flip=True, sharpness=0.5, brightness=0.9, noise=dict(std=0.05, mean=0.0, seed=1)),
              dict(sharpness=0.7, motion_blur=dict(ksize=11, angle=-3.0, direction=0.2), contrast=1.1, posterize=6)]
    p, fused, plain = _modules(be, geom, compose)
    out = fused(be.t(x), params=params)
    two_step = plain(p(be.t(x)), params=params)
    again = fused(be.t(x), prepared=fused.prepare(params, T, H, W, out.device))
    be.sync()
    assert same_bits(out, two_step) and same_bits(again, out)
    assert not same_bits(out, ref)
    # fp32 input behaves exactly as without a processor
    assert same_bits(fused(be.t(ref), params=params), two_step)
    be.sync()


# ------------------------------------------------------------------------------------------------ refusals
BAD_GEOMETRY = [dict(src_h=0), dict(src_w=0), dict(src_h=-3), dict(pad_top=-1), dict(pad_left=-1), dict(pad_top=4), dict(pad_left=10),
                dict(src_h=25, pad_top=0), dict(src_w=141, pad_left=0), dict(fill=-1), dict(fill=256)]


def test_aug_pass_refuses_a_bad_raw_source(be):
    geom = "odd_two_tiles"      # 21 x 131 at (1, 4) of 24 x 140
    x, ref = raw_batch(geom)
    H, W = GEOMS[geom][2:4]
    jobs, maps = [dict(mode=cabi.MDS_AUG_COPY)] * B, np.zeros((B, T, 6), dtype=np.float32)
    xs, out, jt, mp = be.t(x), be.out((B, T, H, W)), _jobs(be, jobs), be.t(torch.from_numpy(maps))

    def rc(buf0, raw):
        kw = dict(B=B, T=T, H=H, W=W, buf=[buf0, be.ptr(out), 0, 0], jobs=jt, maps=mp, noise=None)
        if raw is not None:
            kw["raw"] = raw
        return be.rc("aug_pass", cabi.make("mds_aug_args", **kw))
    assert rc(0, None) == cabi.MDS_ERR_BAD_ARG                                    # neither an fp32 nor a raw source
    assert rc(0, _raw_t(None, geom)) == cabi.MDS_ERR_BAD_ARG                      # geometry without a pointer is not a source
    for over in BAD_GEOMETRY:
        assert rc(0, _raw_t(xs, geom, **over)) == cabi.MDS_ERR_BAD_ARG, over
        assert b"aug_pass" in be.lib.dll.mds_last_error()
    assert rc(0, _raw_t(xs, geom)) == 0                                           # and the good one runs
    be.sync()
    assert same_bits(out, ref)


def test_pad_normalize_refuses_bad_arguments(be):
    geom = "odd_two_tiles"
    x, ref = raw_batch(geom)
    H, W = GEOMS[geom][2:4]
    xs, dst = be.t(x), be.out((B, T, H, W))
    for over in BAD_GEOMETRY + [dict(src=None), dict(dst=None), dict(n=0), dict(H=0, src_h=1, pad_top=0), dict(W=-1)]:
        assert be.rc("pad_normalize", _pad_normalize_args(be, xs, dst, geom, **over)) == cabi.MDS_ERR_BAD_ARG, over
        assert b"pad_normalize" in be.lib.dll.mds_last_error()
    assert be.rc("pad_normalize", _pad_normalize_args(be, xs, dst, geom)) == 0
    be.sync()
    assert same_bits(dst, ref)


def test_python_level_errors(be):
    geom = "pad_left_2"
    x, _ = raw_batch(geom)
    _, _, H, W, _ = GEOMS[geom]
    p = processor(be, geom)
    with pytest.raises(cabi.MdsError, match="uint8"):
        p(be.t(x).to(torch.float32))                                    # no eager path for other types
    with pytest.raises(cabi.MdsError, match="contiguous"):
        p(be.t(x)[..., ::2])
    with pytest.raises(NotImplementedError, match="pad_mode"):
        processor(be, geom, pad_mode="reflect")(be.t(x))
    with pytest.raises(AssertionError):
        frames.PadNormalizeFramesProcessor((W - 8, H))(be.t(x))         # the frame does not fit
    with pytest.raises(cabi.MdsError, match="fill_value"):
        frames.PadNormalizeFramesProcessor((W, H), fill_value=300)(be.t(x))
    if be.name == "emu":
        with pytest.raises(cabi.MdsError, match="cuda"):
            frames.PadNormalizeFramesProcessor((W, H))(x)               # a CPU tensor without the injected simulator
    _, fused, plain = _modules(be, geom, False)
    with pytest.raises(cabi.MdsError, match="frames_processor"):
        plain(be.t(x))                                                  # uint8 without a processor
    with pytest.raises(cabi.MdsError, match="contiguous"):
        fused(be.t(x).transpose(0, 1))
    with pytest.raises(AssertionError):
        fused(be.t(x).to(torch.float64))                                # as before: fp32 (or, now, uint8) only
    with pytest.raises(cabi.MdsError, match="pads to"):
        augment.TrainAugmentations((W + 4, H), frames_processor=p)      # the two sizes must agree
    with pytest.raises(cabi.MdsError, match="PadNormalizeFramesProcessor"):
        augment.TrainAugmentations((W, H), frames_processor=lambda f: f)
    edge = augment.TrainAugmentations((W, H), frames_processor=processor(be, geom, pad_mode="edge"))
    edge._lib = fused._lib
    with pytest.raises(NotImplementedError, match="pad_mode"):
        edge(be.t(x))
    be.sync()


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_140():
    assert cabi.MDS_VERSION >= 140
    assert "mds_pad_normalize" in [n for n, _ in cabi.LONG_FUNCS]
    assert "mds_pad_normalize" not in [n for n, _ in cabi.FUNCS]
    raw = dict(cabi.STRUCTS["mds_aug_raw_t"]._fields_)
    assert list(raw) == ["u8", "src_h", "src_w", "pad_top", "pad_left", "fill"] and raw["u8"] is ctypes.c_void_p
    assert dict(cabi.STRUCTS["mds_aug_args"]._fields_)["raw"] is cabi.STRUCTS["mds_aug_raw_t"]
    zero = cabi.make("mds_aug_args")
    assert not zero.raw.u8 and zero.raw.src_h == 0 and zero.raw.fill == 0      # all-zero = the fp32 source
