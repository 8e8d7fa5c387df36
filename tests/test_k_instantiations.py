"""A ledger of the template instantiations of the convolution and GEMM kernels, one numeric case per instantiation
(tools/kernel_census.py lists what is compiled; tests/test_zz_kernel_census.py fails when an instantiation has no case).

Where a family is a product of template values (conv_wgrad_kernel, conv_fwd_q_kernel, conv_fwd_kernel, pwk8_kernel) the case table
is the WHOLE product, so that it can be read against the launcher: about 66 of its 297 cases (about 10 conv_wgrad, 24 conv_fwd_q, 8
conv_fwd, 24 pwk8) name an instantiation that a shape of test_k_conv.py / test_k_pw.py reaches as well, and deleting one of those
leaves the census passing.  Every other case here is the only launch of its instantiation: deleting it makes the census fail and
name it.  The other families list only what the rest of the suite does not launch.

A case names the instantiation it is for, picks the smallest arguments that route to it - read off the launcher: what selects the
tile shape, the prologue, the ragged tail, the residual / post form, the patch-vector count - with a few output rows, a width that
is no multiple of the tile, an interior and an edge, runs on both backends, and on the simulator asserts that the launch hit the
instantiation it names (the same host routing code runs on the GPU).

References: the cases written here (convolutions by tap list, the depthwise tail, the multi-tensor and table kernels) compare with
float64 torch on the operands as stored.  The cases that reuse a neighbour's check run that neighbour's reference: float64 in
test_pw_fwd, _run_pw_plain's statistics, test_c3_filter_in_registers and test_conv_project's `reference`; float32 torch (K <= 448,
against the same tol(dt)) in test_pw_fwd_output_transform, test_pw_fwd_split_k and the elementwise part of test_c3_post_statistics."""
import pytest
import torch
import torch.nn.functional as F

from backends import be, DT, ABS, assert_close, assert_sum_close, assert_stats_close, knobs, pro_operand  # noqa: F401
from mds import cabi, geometry as geo

TYPES = {"f32": "float", "bf16": "unsigned short"}


def gen(s):
    return torch.Generator().manual_seed(s)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def hit(be, inst):
    """simulator: the last launch is the instantiation the case names"""
    rec = be.launches()
    if rec is not None:
        assert rec[-1].inst == inst, f"the case routed to {rec[-1].inst}, not to {inst}"


def hit_among(be, inst):
    """simulator: a case of several launches (a yardstick launch beside the one under test) made the instantiation it names"""
    rec = be.launches()
    if rec is not None:
        assert inst in {l.inst for l in rec}, f"the case routed to {sorted({l.inst for l in rec})}, not to {inst}"


# ------------------------------------------------------------------------------------------------ convolutions by tap list
def taps3x3(pt=1, pl=1, dil=1):
    """the nine taps of a 3x3 filter with dilation `dil`: input offset (dy, dx) of tap (ky, kx), filter slot 3 ky + kx"""
    return ([dil * ky - pt for ky in range(3) for _ in range(3)], [dil * kx - pl for _ in range(3) for kx in range(3)], list(range(9)))


def tap_conv(a, w, taps, stride, OH, OW):
    """float64 convolution by tap list: y[n][o][oy][ox] = sum_t sum_i a[n][i][oy * stride + dy[t]][ox * stride + dx[t]] * w[o][i][wi[t]],
    zero outside the image (a: [N][I][H][W], w: [O][I][wtaps]) - what mds_conv_fwd / mds_conv_wgrad define, without torch's padding rules"""
    dy, dx, wi = taps
    H, W = a.shape[2:]
    top, left = max(0, -min(dy)), max(0, -min(dx))
    bot = max(0, (OH - 1) * stride + max(dy) - (H - 1))
    right = max(0, (OW - 1) * stride + max(dx) - (W - 1))
    ap = F.pad(a, (left, right, top, bot))
    y = 0
    for t in range(len(dy)):
        y0, x0 = top + dy[t], left + dx[t]
        patch = ap[:, :, y0:y0 + (OH - 1) * stride + 1:stride, x0:x0 + (OW - 1) * stride + 1:stride]
        y = y + torch.einsum("nihw,oi->nohw", patch, w[:, :, wi[t]])
    return y


def tap_wgrad(a, dyt, shape, taps, stride):
    """float64 autograd of tap_conv's filter ([O][I][wtaps])"""
    ww = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    tap_conv(a, ww, taps, stride, dyt.shape[2], dyt.shape[3]).backward(dyt)
    return ww.grad


def conv_pro(x, mode, scale, shift, dt):
    xq = x.double()
    if not mode:
        return xq, None
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    return pro_operand(xq * sc + sh, (xq * sc).abs() + sh.abs(), mode == 2, dt)


# ------------------------------------------------------------------------------------------------ conv_wgrad_kernel<T, PRO, CI, CO, XL>
# k_conv.hip, mds_conv_wgrad: CI = Cin / 16; CO = 1 for Cout == 16, else 4 (64-channel slices, the last one ragged at Cout = 80);
# XL = 3 / 5 / 9 covers ceil(TH * TW * (Cin / 8) / 256) patch vectors per thread, TH x TW = (7 stride + extent) x (15 stride + extent)
# the input patch of an 8 x 16 output tile.  Geometry that reaches each XL at each Cin (stride, dilation, taps):
WGRAD_GEOMETRY = {
    (1, 3): (1, 1, 9),      # 10 x 18 x 2 = 360 vectors
    (1, 5): (2, 1, 9),      # 17 x 33 x 2 = 1122: the stride-2 layers
    (1, 9): (3, 1, 9),      # 24 x 48 x 2 = 2304: input stride 3, the largest patch the staging registers take
    (2, 3): (1, 1, 9),      # 10 x 18 x 4 = 720
    (2, 5): (1, 2, 9),      # 12 x 20 x 4 = 960: dilation 2
    (2, 9): (2, 1, 9),      # 17 x 33 x 4 = 2244
    (3, 3): (1, 1, 1),      # 8 x 16 x 6 = 768: a one-tap list (a 1x1 filter: wtaps = 1)
    (3, 5): (1, 1, 9),      # 10 x 18 x 6 = 1080
    (3, 9): (1, 2, 9),      # 12 x 20 x 6 = 1440
}


@pytest.mark.parametrize("xl", [3, 5, 9])
@pytest.mark.parametrize("co", [1, 4])
@pytest.mark.parametrize("ci", [1, 2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_conv_wgrad_instantiation(be, dt, mode, ci, co, xl):
    """two images of 9 x 21 outputs: 2 x 2 tiles of 8 x 16 each, ragged in both directions; Cout = 80 is a full and a quarter slice"""
    code, tdt = DT[dt]
    stride, dil, ntaps = WGRAD_GEOMETRY[ci, xl]
    N, OH, OW, Cin, Cout = 2, 9, 21, 16 * ci, 16 if co == 1 else 80
    H, W = OH * stride - (stride - 1) // 2, OW * stride - (stride // 2)       # the last tile's patch ends past the image on both axes
    taps = taps3x3(dil, dil, dil) if ntaps == 9 else ([0], [0], [0])
    g = gen(1000 * ci + 100 * co + 10 * xl + mode)
    x = torch.randn(N, Cin, H, W, generator=g).to(tdt)
    scale = 1 + 0.2 * torch.randn(Cin, generator=g); shift = 0.3 * torch.randn(Cin, generator=g)
    dyt = torch.randn(N, Cout, OH, OW, generator=g).to(tdt)
    a, aerr = conv_pro(x, mode, scale, shift, dt)
    shape, dy64, cnt = (Cout, Cin, ntaps), dyt.double(), N * OH * OW
    want = tap_wgrad(a, dy64, shape, taps, stride)
    parts = [(cnt, tap_wgrad(a.abs(), dy64.abs(), shape, taps, stride))] + ([(ABS, tap_wgrad(aerr, dy64.abs(), shape, taps, stride))] if mode else [])
    cut = dy64.clone(); cut[:, :, :, -1] = 0
    probes = [("last output column left out", tap_wgrad(a, cut, shape, taps, stride)), ("last image left out", tap_wgrad(a[:-1], dy64[:-1], shape, taps, stride))]
    if ntaps == 9:
        probes.append(("ky / kx transposed", want.view(Cout, Cin, 3, 3).transpose(2, 3).reshape(shape)))
    dw = be.out(shape, torch.float32, 0, name="dw")
    be.reset_launches()
    be.call("conv_wgrad", cabi.make("mds_conv_wgrad_args", dtype=code, N=N, IH=H, IW=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, **{"is": stride},
                                    ntaps=ntaps, dy=taps[0], dx=taps[1], wi=taps[2], wtaps=ntaps, x=be.t(nhwc(x)), dyt=be.t(nhwc(dyt)), dw=dw,
                                    pro=cabi.pro(mode, be.t(scale), be.t(shift))))
    be.sync()
    hit(be, f"conv_wgrad_kernel<{TYPES[dt]}, {mode}, {ci}, {co}, {xl}>")
    assert_sum_close(dw, want, parts, "dw", probes, cap=(dt, cnt ** 0.5))


def test_conv_wgrad_refuses_a_tap_list_that_leaves_filter_slots_out(be):
    """every block adds all Cin x wtaps values of its output channels from a staging that only the launch's taps fill: with one tap
    of a nine-slot filter the other eight slots received stale staging contents (found by the one-tap case above when it passed
    wtaps = 9).  Such a list is an argument error now; the same tap as a one-slot filter is the case above.  Two taps that name one
    slot are refused too: their units write the same staging address and one contribution would be lost."""
    N, H, W, Cin, Cout = 1, 8, 16, 48, 16
    x, dyt = be.t(torch.zeros(N, H, W, Cin)), be.t(torch.zeros(N, H, W, Cout))
    dw = be.out((Cout, Cin, 9), torch.float32, 0)
    for ntaps, wi in ((1, [4]), (9, [0, 1, 2, 3, 4, 5, 6, 7, 9]), (8, list(range(8))), (9, [0, 1, 2, 3, 4, 5, 6, 7, 7])):
        args = cabi.make("mds_conv_wgrad_args", dtype=0, N=N, IH=H, IW=W, Cin=Cin, OH=H, OW=W, Cout=Cout, **{"is": 1}, ntaps=ntaps,
                         dy=[0] * ntaps, dx=[0] * ntaps, wi=wi, wtaps=9, x=x, dyt=dyt, dw=dw, pro=cabi.pro(0))
        assert be.rc("conv_wgrad", args) == cabi.MDS_ERR_BAD_ARG
        assert b"filter slot" in be.lib.dll.mds_last_error()
    be.sync()
    assert not dw.any()


# ------------------------------------------------------------------------------------------------ mds_conv_fwd by tap list
ROW3 = ([0, 0, 0], [-1, 0, 1], [0, 1, 2])        # a 1 x 3 filter: three taps in a row (wtaps = 3)


def run_conv_fwd(be, dt, N, H, W, Cin, Cout, stride, mode, taps=None, res=False, emode=0, stats=False, seed=0):
    """one mds_conv_fwd launch over the whole output against tap_conv in float64: y elementwise, forward statistics as sums"""
    code, tdt = DT[dt]
    g = gen(seed + 31 * H + W + Cin + 7 * Cout)
    if taps is None:
        OH, OW, pt, pl = geo.conv_geometry(H, W, stride)
        taps = taps3x3(pt, pl)
    else:
        OH, OW = -(-H // stride), -(-W // stride)
    wtaps = max(taps[2]) + 1
    x = torch.randn(N, Cin, H, W, generator=g).to(tdt)
    w = (torch.randn(Cout, Cin, wtaps, generator=g) / (len(taps[0]) * Cin) ** 0.5).to(tdt)
    scale = 1 + 0.2 * torch.randn(Cin, generator=g); shift = 0.3 * torch.randn(Cin, generator=g)
    esc = 1 + 0.3 * torch.randn(Cout, generator=g); esh = 0.4 * torch.randn(Cout, generator=g)
    r = torch.randn(N, OH, OW, Cout, generator=g).to(tdt) if res else None
    y = be.out((N, OH, OW, Cout), tdt, float("nan"))
    st = be.out((cabi.MDS_STAT_SLOTS, 2, Cout), torch.float64, 0) if stats else None
    kw = dict(epi=cabi.make("mds_epi_t", mode=emode, scale=be.t(esc), shift=be.t(esh))) if emode else {}
    be.reset_launches()
    be.call("conv_fwd", cabi.make("mds_conv_fwd_args", dtype=code, N=N, IH=H, IW=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, A=OH, B=OW, oy0=0, ox0=0,
                                  os=1, **{"is": stride}, ntaps=len(taps[0]), dy=taps[0], dx=taps[1], wi=taps[2], wtaps=wtaps, x=be.t(nhwc(x)),
                                  w=be.t(w.permute(0, 2, 1).contiguous()), y=y, pro=cabi.pro(mode, be.t(scale), be.t(shift)),
                                  residual=be.t(r) if res else None, stats=st, **kw))
    be.sync()
    a, aerr = conv_pro(x, mode, scale, shift, dt)
    w64 = w.double()
    v = nhwc(tap_conv(a, w64, taps, stride, OH, OW))
    ref = v
    if emode:
        ref = ref * esc.double() + esh.double()
        ref = F.silu(ref) if emode == 2 else ref
    if res:
        ref = ref + r.double()
    assert_close(y, ref, dt, msg="y")
    if stats:       # sums of the fp32 accumulators, before the store rounds them
        vabs = nhwc(tap_conv(a.abs(), w64.abs(), taps, stride, OH, OW))
        verr = nhwc(tap_conv(aerr, w64.abs(), taps, stride, OH, OW)) if mode else None
        cnt = N * OH * OW
        nc = OW % 16 or max(1, OW // 8)      # the ragged last 16-column tile (one column of a K = 1152 layer is below the resolution of `sumsq`)
        probes = [(f"last {nc} columns left out", lambda t: t[:, :, :-nc]), ("last image left out", lambda t: t[:-1]) if N > 1 else ("last row left out", lambda t: t[:, :-1])]
        # one row of OH: `sumsq`'s bound is (2 K + 2) U sum vabs^2, and sum vabs^2 ~ 0.4 K sum v^2 for zero-mean operands - a share
        # K^2 x 1e-7 of the sum, 13 % at K = 1152 and 3 % at K = 576: the row probe only where it is above that
        if len(taps[0]) * Cin <= 576:
            probes.append(("row 0 counted twice", lambda t: torch.cat([t, t[:, :1]], 1)))
        assert_stats_close(st.sum(0), v, vabs, len(taps[0]) * Cin, cnt, (dt, cnt ** 0.5), verr, probes)


# ------------------------------------------------------------------------------------------------ c3_kernel / c3s_kernel (k_c3.hip)
# c3_kernel<CIN, NF, NSPL, SPW, NPW, NSW, RES, STATS, MASKED, POST, ONE, NTW>: the instance follows (Cin, Cout) of the launch (c3_fwd_route),
# RES / POST / STATS the operands, MASKED a width that is no multiple of the band (32 columns; 64 for 16 -> 32 and behind the prologue).
# MDS_KNOB_C3 = 2 lifts the size bar.  Five rows: more than the ring's three-row batch, so a band has an interior and both edges.
C3_INSTANCE = {(128, 32): "128, 1, 2, 1, 3, 1", (16, 32): "16, 2, 1, 1, 2, 2", (32, 128): "32, 2, 4, 2, 2, 2", (48, 192): "48, 2, 2, 1, 2, 2"}
C3_BAND = {(128, 32): 32, (16, 32): 64, (32, 128): 32, (48, 192): 32}
C3_FORMS = [  # Cin, Cout of the launch, residual, statistics, ragged width, post statistics
    (128, 32, False, False, False, False), (128, 32, False, False, False, True), (128, 32, False, True, False, False),
    (128, 32, False, True, True, False), (128, 32, True, False, False, False),
    (16, 32, False, False, False, False), (16, 32, False, True, False, False), (16, 32, False, True, True, False),
    (16, 32, True, False, False, False), (16, 32, True, False, False, True),
    (32, 128, False, False, False, False), (32, 128, False, False, False, True), (32, 128, False, False, True, False),
    (32, 128, False, False, True, True), (32, 128, True, False, False, False), (32, 128, True, False, True, False),
    (48, 192, False, False, False, False), (48, 192, False, False, False, True), (48, 192, False, False, True, False),
    (48, 192, False, False, True, True), (48, 192, False, True, False, False), (48, 192, True, False, False, False),
    (48, 192, True, False, False, True), (48, 192, True, False, True, False), (48, 192, True, False, True, True),
]


def flag(b):
    return "true" if b else "false"


@pytest.mark.parametrize("Cin,Cout,res,stats,ragged,post", C3_FORMS)
def test_c3_instantiation(be, Cin, Cout, res, stats, ragged, post):
    import test_k_conv as tc
    band = C3_BAND[Cin, Cout]
    N, H, W = (2, 5, band + 5) if ragged else (1, 5, 2 * band)
    be.reset_launches()
    if post:      # the data gradient of the forward layer Cout -> Cin with the BatchNorm-backward sums of the layer below
        tc.test_c3_post_statistics(be, 1, N, H, W, 0, False, Cout, Cin, with_res=res)
    else:
        tc.test_c3_filter_in_registers(be, N, H, W, Cin, Cout, res, stats, 0)
    hit(be, f"c3_kernel<{C3_INSTANCE[Cin, Cout]}, {flag(res)}, {flag(stats)}, {flag(ragged)}, {flag(post)}, false, 0>")


@pytest.mark.parametrize("ragged", [False, True])
def test_c3_instantiation_prologue_without_statistics(be, ragged):
    """the first 3x3 layer's instance (32 -> 16 behind BatchNorm + SiLU, transform waves) in its two forms without forward statistics"""
    with knobs(be, {cabi.MDS_KNOB_C3: 2}):
        run_conv_fwd(be, "bf16", *((2, 5, 70) if ragged else (1, 5, 128)), 32, 16, 1, 2)
        hit(be, f"c3_kernel<32, 1, 1, 1, 1, 1, false, false, {flag(ragged)}, false, false, 8>")


def test_c3_instantiation_one_tap_with_residual(be):
    """a prologue-free 32 -> 64 1x1 launch with a residual operand as one-tap 'images' (c3_pw_try)"""
    import test_k_pw as tp
    with knobs(be, {cabi.MDS_KNOB_C3: 2}):
        tp.test_pw_fwd(be, "bf16", 96 * 5, 32, 64, 0, True, False)
        hit(be, "c3_kernel<32, 2, 2, 1, 1, 3, true, false, false, false, true, 0>")


@pytest.mark.parametrize("Cin,Cout,mode,W,inst", [
    (32, 128, 0, 128, "32, 2, 4, 2, 2, 2, false, false, 0"), (32, 128, 0, 40, "32, 2, 4, 2, 2, 2, false, true, 0"),      # 32-column output bands
    (16, 64, 0, 256, "16, 2, 2, 2, 2, 2, false, false, 0"), (16, 64, 0, 70, "16, 2, 2, 2, 2, 2, false, true, 0"),      # 64-column bands
    (16, 64, 2, 256, "16, 1, 4, 4, 1, 1, false, false, 6"),                                                            # behind the prologue: whole bands only
])
def test_c3s_instantiation_without_statistics(be, Cin, Cout, mode, W, inst):
    """the stride-2 forward kernel's forms without forward statistics (the suite's other cases all ask for them); six input rows
    = three output rows: one batch of four input rows and a partial one"""
    with knobs(be, {cabi.MDS_KNOB_C3: 2}):
        run_conv_fwd(be, "bf16", 2, 6, W, Cin, Cout, 2, mode)
        hit(be, f"c3s_kernel<{inst}>")


# ------------------------------------------------------------------------------------------------ conv_fwd_q_kernel<T, HASPRO, IS, MF, NF, X3>
# k_conv.hip's persistent kernel: mds_conv_fwd takes the first (NF, MF) - tried in the order NF = 4, 2, 1 (what Cout / 16 allows) by
# MF = 4, 2, 1 (stride 2: 2, 1) - whose input patch ((4 MF - 1) stride + extent) x (15 stride + extent) x Cin / 8 stays within 1536
# vectors and fits 76 KiB of LDS together with the 16 NF x K filter slab.  So Cin picks MF (a taller patch no longer fits), and Cin
# x taps picks NF (a wider slab no longer fits); a 1 x 3 tap list shortens K where nine taps would push NF further down.
# (taps, Cin, Cout) that reach each (IS, MF, NF), per type (the slab is twice as large in fp32):
CVQ_SHAPES = {
    "f32": {(1, 1, 1): ("3x3", 64, 16), (1, 1, 2): ("3x3", 40, 32), (1, 1, 4): ("1x3", 64, 48), (1, 2, 1): ("3x3", 40, 16), (1, 2, 2): ("3x3", 32, 32),
            (1, 2, 4): ("1x3", 40, 48), (1, 4, 1): ("3x3", 8, 16), (1, 4, 2): ("3x3", 8, 32), (1, 4, 4): ("3x3", 8, 48), (2, 1, 1): ("3x3", 32, 16),
            (2, 1, 2): ("1x3", 32, 32), (2, 1, 4): ("3x3", 16, 48), (2, 2, 1): ("3x3", 8, 16), (2, 2, 2): ("3x3", 8, 32), (2, 2, 4): ("3x3", 8, 48)},
    "bf16": {(1, 1, 1): ("3x3", 96, 16), (1, 1, 2): ("1x3", 96, 32), (1, 1, 4): ("3x3", 48, 48), (1, 2, 1): ("3x3", 40, 16), (1, 2, 2): ("3x3", 40, 32),
             (1, 2, 4): ("3x3", 40, 48), (1, 4, 1): ("3x3", 8, 16), (1, 4, 2): ("3x3", 8, 32), (1, 4, 4): ("3x3", 8, 48), (2, 1, 1): ("3x3", 32, 16),
             (2, 1, 2): ("3x3", 32, 32), (2, 1, 4): ("3x3", 32, 48), (2, 2, 1): ("3x3", 8, 16), (2, 2, 2): ("3x3", 8, 32), (2, 2, 4): ("3x3", 8, 48)},
}
CVQ_CASES = [(dt, hp, key, x3) for dt in ("f32", "bf16") for hp in (False, True) for key in sorted(CVQ_SHAPES[dt]) for x3 in ((False, True) if dt == "f32" else (False,))]


@pytest.mark.parametrize("dt,hp,key,x3", CVQ_CASES)
def test_conv_fwd_q_instantiation(be, dt, hp, key, x3):
    """two images of (4 MF + 3) x 21 outputs: two row tiles and two column tiles, both ragged.  X3 - fp32 operands as split-bf16
    products - is what an fp32 launch with an output transform takes; without one the case checks the forward statistics"""
    stride, mf, nf = key
    taps, Cin, Cout = CVQ_SHAPES[dt][key]
    OH, OW = 4 * mf + 3, 21
    run_conv_fwd(be, dt, 2, OH * stride, OW * stride - (stride - 1), Cin, Cout, stride, (1 if x3 else 2) if hp else 0,
                 ROW3 if taps == "1x3" else None, emode=2 if x3 else 0, stats=not x3)
    hit(be, f"conv_fwd_q_kernel<{TYPES[dt]}, {flag(hp)}, {stride}, {mf}, {nf}, {flag(x3)}>")


# ------------------------------------------------------------------------------------------------ conv_fwd_kernel<T, PRO, IS, NF>
# k_conv.hip's tiled kernel takes what the persistent one does not: a launch with a residual operand, or a patch / slab that fits no
# (NF, MF) - Cin = 128 (K = 1152) at any stride.  NF = Cout / 16 up to 64 channels per pass.  At Cin = 128 the taps no longer fit
# LDS together and are staged in barrier groups (the chunked-K form).
@pytest.mark.parametrize("nf", [1, 2, 3, 4])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_conv_fwd_tiled_instantiation(be, dt, mode, stride, nf):
    """two images of 19 x 21 outputs (tiles of 16 x 16 at stride 1, 8 x 16 at stride 2).  Without a prologue: Cin = 8 (a quarter of a
    k-step) with a residual operand; behind the affine prologue: Cin = 128, chunked K, forward statistics; behind BatchNorm + SiLU:
    Cin = 40 (one k-step and a quarter) with a residual operand"""
    Cin, res = {0: (8, True), 1: (128, False), 2: (40, True)}[mode]
    OH, OW = 19, 21
    run_conv_fwd(be, dt, 2, OH * stride, OW * stride - (stride - 1), Cin, 16 * nf, stride, mode, res=res, stats=not res)
    hit(be, f"conv_fwd_kernel<{TYPES[dt]}, {mode}, {stride}, {nf}>")


# ------------------------------------------------------------------------------------------------ pw_fwd_kernel<T, PRO, WN, BM, TAIL, SPLIT, DEEP>
# k_pw.hip, mds_pw_fwd: WN = 1 (128 x 64 tiles) for N <= 64 unless split, else 2; BM = 64 below 400 000 rows; TAIL = 2 with an output
# transform, 1 with post statistics; SPLIT with args.split > 1; DEEP (two K chunks in flight) for fp32 launches with an output transform
# or split-K that walk three or more 32-wide chunks.  The cases reuse tests/test_k_pw.py's checks at (prologue, N, epi, split) the
# suite's own shapes do not combine.
PW_PLAIN = [  # M, K, N, prologue, residual, statistics -> PRO, WN, BM
    (200, 48, 144, 1, False, True, "1, 2, 64, 0"),       # affine prologue on a two-n-tile layer (128 + 16 columns), K tail
    (200, 48, 48, 2, True, True, "2, 1, 128, 0"),        # BatchNorm + SiLU on a narrow projection: 128 x 64 tiles, ragged second row tile
    (200, 112, 144, 3, False, True, "3, 2, 64, 0"),      # BatchNorm + SiLU + gate, gate boundaries inside a tile (50 rows per group)
    (200, 112, 48, 4, True, False, "4, 1, 128, 0"),      # gate only, narrow
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,K,N,mode,res,stats,inst", PW_PLAIN)
def test_pw_fwd_instantiation(be, dt, M, K, N, mode, res, stats, inst):
    import test_k_pw as tp
    be.reset_launches()
    tp.test_pw_fwd(be, dt, M, K, N, mode, res, stats)
    hit(be, f"pw_fwd_kernel<{TYPES[dt]}, {inst}, false, false>")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,res,inst", [(48, False, "2, 1, 128, 2"), (144, True, "2, 2, 64, 2")])
def test_pw_fwd_instantiation_bn_silu_with_output_transform(be, dt, N, res, inst):
    import test_k_pw as tp
    be.reset_launches()
    tp.test_pw_fwd_output_transform(be, dt, 200, 48, N, 2, 2 if res else 1, res)
    hit(be, f"pw_fwd_kernel<{TYPES[dt]}, {inst}, false, false>")


@pytest.mark.parametrize("dt,K,N,pmode,emode,res,split,inst", [
    ("f32", 64, 48, 0, 0, False, 2, "0, 2, 64, 0, true, false"),       # one 32-wide chunk per split: below the three that DEEP needs
    ("f32", 64, 144, 0, 2, False, 2, "0, 2, 64, 2, true, false"),
    ("f32", 64, 48, 4, 0, True, 2, "4, 2, 64, 0, true, false"),
    ("bf16", 64, 48, 4, 0, True, 2, "4, 2, 64, 0, true, false"),
    ("f32", 448, 144, 4, 0, False, 3, "4, 2, 64, 0, true, true"),      # five chunks per split: DEEP
    ("f32", 64, 144, 4, 1, True, 2, "4, 2, 64, 2, true, false"),
])
def test_pw_fwd_instantiation_split_k(be, dt, K, N, pmode, emode, res, split, inst):
    """(split launch twice, then the unsplit yardstick: the instantiation is among the launches)"""
    import test_k_pw as tp
    be.reset_launches()
    tp.test_pw_fwd_split_k(be, dt, 130, K, N, pmode, emode, res, split)
    hit_among(be, f"pw_fwd_kernel<{TYPES[dt]}, {inst}>")


# ------------------------------------------------------------------------------------------------ pw_fwd_wres_kernel<T, 0, NF, KS, RING>
# k_pwr.hip: NF = 3 (96-column tiles) where N is a multiple of 96 and not of 128, else 4; KS = ceil(K / 32) in {3, 4, 6}; RING = 2 row
# tiles in flight for fp32 at KS = 6, else 3.  MDS_KNOB_PW_WRES = 2 takes the kernel at any M.  An fp32 filter tile of K > 96 leaves one
# block per CU, which is why the suite's own fp32 cases stop at K = 96 - the launcher still takes the kernel there.
@pytest.mark.parametrize("dt,K,N,inst", [
    ("f32", 80, 192, "3, 3, 3"), ("f32", 112, 192, "3, 4, 3"), ("f32", 176, 192, "3, 6, 2"), ("f32", 128, 144, "4, 4, 3"), ("f32", 192, 144, "4, 6, 2"),
    ("bf16", 96, 192, "3, 3, 3"), ("bf16", 192, 192, "3, 6, 3"), ("bf16", 128, 256, "4, 4, 3"),
])
def test_pw_fwd_wres_instantiation(be, dt, K, N, inst):
    """650 rows = 11 row tiles over 8 blocks: one and two tiles per block, the last tile ragged; N = 144: a ragged n-tile"""
    import test_k_pw as tp
    with knobs(be, {cabi.MDS_KNOB_PW_WRES: 2}):
        tp._run_pw_plain(be, dt, 650, K, N, False, True, 0, True)
        hit(be, f"pw_fwd_wres_kernel<{TYPES[dt]}, 0, {inst}>")


# ------------------------------------------------------------------------------------------------ conv_project_kernel<T, IS, MF, CF, X3>
# k_c3p.hip: CF = project.cout / 16; the tile height 4 MF is the tallest that still gives each of the 256 CUs a tile, otherwise the
# smallest (conv_fwd_project's score) - so a tall tile needs 256 tiles.  The widths below are the narrowest that reach it with two
# ragged row tiles: 19 rows x 2 x 64 column tiles of 16 (MF = 4); 24 rows, where three 8-row tiles x 2 x 44 pass 256 and two 16-row
# tiles do not (MF = 2); stride 2: 11 output rows x 2 x 64 (MF = 2).  8 -> 16 channels inside: a quarter k-step per tap, half a chunk.
CP_SHAPES = {(1, 1): (2, 9, 21), (1, 2): (2, 24, 16 * 43 + 5), (1, 4): (2, 19, 16 * 63 + 5), (2, 1): (2, 13, 41), (2, 2): (2, 22, 2 * (16 * 63 + 5))}
CP_CASES = [("f32", 1, 2, 1), ("f32", 1, 2, 2), ("f32", 1, 2, 3), ("f32", 1, 4, 1), ("f32", 1, 4, 2), ("f32", 1, 4, 3), ("f32", 2, 1, 1),
            ("f32", 2, 2, 1), ("f32", 2, 2, 2), ("f32", 2, 2, 3), ("bf16", 1, 1, 1), ("bf16", 1, 2, 1), ("bf16", 1, 2, 2), ("bf16", 1, 2, 3),
            ("bf16", 1, 4, 1), ("bf16", 1, 4, 2), ("bf16", 1, 4, 3), ("bf16", 2, 1, 1), ("bf16", 2, 2, 1), ("bf16", 2, 2, 2), ("bf16", 2, 2, 3)]


@pytest.mark.parametrize("dt,stride,mf,cf", CP_CASES)
def test_conv_project_instantiation(be, dt, stride, mf, cf):
    """(the fused launch, then the two launches it is measured against: the instantiation is among the launches)"""
    import test_k_conv_project as tcp
    N, H, W = CP_SHAPES[stride, mf]
    be.reset_launches()
    tcp.check(be, dt, N, H, W, 8, 16, 16 * cf, stride, stride == 1, seed=mf + cf)
    hit_among(be, f"conv_project_kernel<{TYPES[dt]}, {stride}, {mf}, {cf}, {flag(dt == 'f32')}>")


# ------------------------------------------------------------------------------------------------ dw2_fwd_kernel<T, 6, 2>
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dw2_fwd_six_row_bands_with_the_squeeze_excite_tail(be, dt):
    """the 3x3 stride-1 depthwise forward in six-row bands (what a launch of 256 blocks or more takes; MDS_KNOB_DW2_R = 1 keeps them
    at a small size) with output transform, pooling and the squeeze-excite tail: y, the pooled means, hidden and gate against float64.
    13 x 11 pixels: two whole bands and a one-row band, an 8-column strip and a 3-column one; 192 channels: three chunks of 64"""
    import test_k_dw_se_tail as ts
    code, tdt = DT[dt]
    N, H, W, C, R = 3, 13, 11, 192, 12
    g = gen(77)
    x = torch.randn(N, 1, H, W, C, generator=g).to(tdt)
    w = torch.randn(C, 9, generator=g) * 0.3
    esc, esh = 1 + 0.3 * torch.randn(C, generator=g), 0.4 * torch.randn(C, generator=g)
    w1, b1 = torch.randn(R, C, generator=g) * 0.3, torch.randn(R, generator=g) * 0.1
    w2, b2 = torch.randn(C, R, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1
    kw = dict(dtype=code, N=N, T=1, IH=H, IW=W, C=C, OH=H, OW=W, stride=1, pad_t=1, pad_l=1, kt=1, w=be.t(w), pro=cabi.pro(0), stats=None,
              epi=cabi.make("mds_epi_t", mode=2, scale=be.t(esc), shift=be.t(esh)), pool_inv=1.0 / (H * W), x=be.t(x))
    se = dict(R=R, w1=be.t(w1), b1=be.t(b1), w2=be.t(w2), w2t=be.t(w2.t()), b2=be.t(b2))
    with knobs(be, {cabi.MDS_KNOB_DW2_R: 1}):
        y, pooled, hidden, gate = ts.launch(be, kw, (N, 1, H, W, C, tdt), se, be.out(N, torch.int32, 0))
        hit(be, f"dw2_fwd_kernel<{TYPES[dt]}, 6, 2>")
    z = F.conv2d(x[:, 0].double().permute(0, 3, 1, 2), w.double().view(C, 1, 3, 3), None, 1, 1, 1, C) * esc.double().view(1, -1, 1, 1) + esh.double().view(1, -1, 1, 1)
    y64 = nhwc(F.silu(z))
    assert_close(y[:, 0], y64, dt, msg="y")
    # the means are taken of the STORED outputs (k_dw.hip, dw_pool_flush: what mds_se_pool would read back): H x W terms, fp64 slots
    ys = y[:, 0].double().cpu()
    assert_sum_close(pooled, ys.mean((1, 2)), [(H * W, ys.abs().mean((1, 2)))], "pooled", [("last row left out", ys[:, :-1].sum((1, 2)) / (H * W)),
                                                                                            ("last column left out", ys[:, :, :-1].sum((1, 2)) / (H * W))])
    pk = pooled.cpu().float().double()      # the tail reads the means as fp32
    h64 = pk @ w1.double().t() + b1.double()
    g64 = torch.sigmoid(F.silu(h64) @ w2.double().t() + b2.double())
    assert_close(hidden, h64, "f32", msg="hidden")
    assert_close(gate, g64, "f32", msg="gate")


# ------------------------------------------------------------------------------------------------ adamw / sgd / ema / bn_eval_table
# The multi-tensor kernels and the eval-table kernel are launched by mds.train / the plans on torch's own parameters; here on guarded
# buffers, against float64.  Three tensors: one chunk and a ragged second (5000 = 4096 + 904), exactly one chunk, a tiny one.
OPT_NUMELS = [5000, 4096, 37]


def opt_tables(be, params, grads, soffs):
    """(table, chunks, nchunks): mds_opt_tensor rows with the parameters' addresses, gradient offsets into the flat buffer `grads`"""
    T = cabi.STRUCTS["mds_opt_tensor"]
    arr = (T * len(params))()
    goff, rows = 0, []
    for k, p in enumerate(params):
        arr[k].p, arr[k].goff, arr[k].soff, arr[k].n = be.ptr(p), goff, soffs[k], p.numel()
        rows += [(k, c) for c in range(-(-p.numel() // cabi.MDS_OPT_CHUNK))]
        goff += p.numel()
    assert goff == grads.numel()
    return be.t(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)), be.t(torch.tensor(rows, dtype=torch.int32)), len(rows)


def opt_setup(be, seed):
    g = gen(seed)
    p0 = [torch.randn(n, generator=g) for n in OPT_NUMELS]
    gr = [torch.randn(n, generator=g) * 3 for n in OPT_NUMELS]
    soffs, off = [], 0
    for n in OPT_NUMELS:
        soffs.append(off); off += (n + 3) // 4 * 4
    params = [be.out(n, torch.float32, t, name=f"p{k}") for k, (n, t) in enumerate(zip(OPT_NUMELS, p0))]
    grads = be.t(torch.cat(gr))
    return g, p0, gr, soffs, off, params, grads


def test_multi_adamw_on_guarded_buffers(be):
    g, p0, gr, soffs, nstate, params, grads = opt_setup(be, 5)
    m0, v0 = torch.randn(nstate, generator=g) * 0.1, torch.rand(nstate, generator=g) * 0.1
    m, v = be.out(nstate, torch.float32, m0), be.out(nstate, torch.float32, v0)
    table, chunks, nchunks = opt_tables(be, params, grads, soffs)
    lr, b1, b2, eps, wd, scale, t_in = 3e-3, 0.9, 0.99, 1e-7, 0.05, 4.0, 2.0
    steps = be.out(2, torch.float32, torch.tensor([t_in, -1.0]))
    be.reset_launches()
    be.call("multi_adamw", cabi.make("mds_adamw_args", table=table, chunks=chunks, nchunks=nchunks, gbase=grads, exp_avg=m, exp_avg_sq=v, lr=lr,
                                     beta1=b1, beta2=b2, eps=eps, weight_decay=wd, bias1=0.0, bias2=0.0, found_inf=None, grad_scale=be.t(torch.tensor([scale])),
                                     step_in=steps[0:1], step_out=steps[1:2], beta1_d=b1, beta2_d=b2))
    be.sync()
    hit(be, "adamw_kernel")
    t = t_in + 1
    assert float(steps[1]) == t
    for k, n in enumerate(OPT_NUMELS):
        gd, o = gr[k].double() / scale, soffs[k]
        m64 = b1 * m0[o:o + n].double() + (1 - b1) * gd
        v64 = b2 * v0[o:o + n].double() + (1 - b2) * gd * gd
        p64 = p0[k].double() * (1 - lr * wd) - lr / (1 - b1 ** t) * m64 / (v64.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        assert_close(m[o:o + n], m64, "f32", msg=f"exp_avg {k}")
        assert_close(v[o:o + n], v64, "f32", msg=f"exp_avg_sq {k}")
        assert_close(params[k], p64, "f32", msg=f"p {k}")
        assert not torch.equal(params[k].cpu(), p0[k]), "the parameter moved"


def test_multi_sgd_on_guarded_buffers(be):
    g, p0, gr, soffs, nstate, params, grads = opt_setup(be, 6)
    buf0 = torch.randn(nstate, generator=g)
    buf = be.out(nstate, torch.float32, buf0)
    table, chunks, nchunks = opt_tables(be, params, grads, soffs)
    lr, mom, wd = 1e-2, 0.9, 0.01
    steps = be.out(2, torch.float32, torch.tensor([1.0, -1.0]))      # not the first step: the buffer is blended, not initialised
    be.reset_launches()
    be.call("multi_sgd", cabi.make("mds_sgd_args", table=table, chunks=chunks, nchunks=nchunks, gbase=grads, momentum_buf=buf, lr=lr, momentum=mom,
                                   dampening=0.0, weight_decay=wd, nesterov=1, first=0, found_inf=None, grad_scale=None, step_in=steps[0:1], step_out=steps[1:2]))
    be.sync()
    hit(be, "sgd_kernel")
    assert float(steps[1]) == 2.0
    for k, n in enumerate(OPT_NUMELS):
        o = soffs[k]
        g64 = gr[k].double() + wd * p0[k].double()
        b64 = mom * buf0[o:o + n].double() + g64
        assert_close(buf[o:o + n], b64, "f32", msg=f"momentum_buffer {k}")
        assert_close(params[k], p0[k].double() - lr * (g64 + mom * b64), "f32", msg=f"p {k}")


def test_multi_ema_on_guarded_buffers(be):
    g, e0, model, soffs, _, ema, flat = opt_setup(be, 7)
    table, chunks, nchunks = opt_tables(be, ema, flat, soffs)
    decay = 0.99
    be.reset_launches()
    be.call("multi_ema", cabi.make("mds_ema_args", table=table, chunks=chunks, nchunks=nchunks, gbase=flat, decay=decay))
    be.sync()
    hit(be, "ema_kernel")
    for k in range(len(OPT_NUMELS)):
        assert_close(ema[k], decay * e0[k].double() + (1 - decay) * model[k].double(), "f32", msg=f"ema {k}")
        assert not torch.equal(ema[k].cpu(), e0[k])


def test_bn_eval_table_on_guarded_buffers(be):
    """two layers in one launch, 40 and 300 channels (two blocks of 256 along x, the first layer idle in the second):
    out = [4][C] {scale, shift, mean, rstd} from the running statistics"""
    g = gen(8)
    Job = cabi.STRUCTS["mds_bn_eval_job"]
    Cs, eps = [40, 300], [1e-5, 1e-3]
    jobs, held = (Job * 2)(), []
    for j, C in enumerate(Cs):
        gamma, beta, mean, var = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g), 0.2 + torch.rand(C, generator=g)
        out = be.out((4, C), torch.float32, float("nan"))
        dev = [be.t(v) for v in (gamma, beta, mean, var)]
        jobs[j].gamma, jobs[j].beta, jobs[j].running_mean, jobs[j].running_var = (be.ptr(v) for v in dev)
        jobs[j].out, jobs[j].eps, jobs[j].C = be.ptr(out), eps[j], C
        held.append((gamma, beta, mean, var, out, dev))
    be.reset_launches()
    be.call_raw("bn_eval_table", jobs, 2, max(Cs))
    be.sync()
    hit(be, "bn_eval_table_kernel")
    for j, (gamma, beta, mean, var, out, _) in enumerate(held):
        rstd = 1 / (var.double() + eps[j]).sqrt()
        scale = gamma.double() * rstd
        assert_close(out, torch.stack([scale, beta.double() - mean.double() * scale, mean.double(), rstd]), "f32", msg=f"layer {j}")


# ------------------------------------------------------------------------------------------------ pwk8_kernel<MFW, WM, NFW, WN, DX, PRO, TAIL>
# k_pwk8.hip (bf16, fragment-major filter copy; MDS_KNOB_PWK = 2 takes it at any size): the column shape follows N - 192-column tiles
# (NFW, WN = 3, 4) above 128, 128-column tiles (2, 4) above 96, else the 96-column shape <3, 2, 3, 2> of 96 rows; MFW = tile rows / 16
# = 4 / 5 / 6 / 8 (MDS_KNOB_PWK_BM picks what the rounds-of-the-chip rule picks at training sizes); PRO the prologue, with a ring one
# stage deeper (DX = 7) behind one; TAIL = 1 the data-gradient form (64 / 80 rows; 96 at 128 columns).
PWK_N = {0: 176, 1: 112, 2: 80}      # 176: not a multiple of 48; 112: a 128-column tile with 16 padding columns; 80: a padding fragment
PWK_FWD = [(shape, bm, mode) for mode in range(5) for shape, bms in ((0, (64, 80, 96, 128)), (1, (64, 80, 96, 128)), (2, (96,))) for bm in bms]
PWK_DG = [(0, 64), (1, 64), (0, 80), (1, 80), (1, 96), (2, 96)]


def pwk_inst(shape, bm, dx, mode, tail):
    return f"pwk8_kernel<{'3, 2, 3, 2' if shape == 2 else f'{bm // 16}, 1, {3 if shape == 0 else 2}, 4'}, {dx}, {mode}, {tail}>"


@pytest.mark.parametrize("shape,bm,mode", PWK_FWD)
def test_pwk8_forward_instantiation(be, shape, bm, mode):
    """170 rows: two or three row tiles, the last ragged, a gate boundary (150 rows per group) inside a tile; K = 96: one and a half stages"""
    import test_k_pw as tp
    with knobs(be, {cabi.MDS_KNOB_PWK: 2, cabi.MDS_KNOB_PWK_BM: 0 if shape == 2 else bm}):
        tp._kstream_case(be, 170, 96, PWK_N[shape], mode, True)
        hit(be, pwk_inst(shape, bm, 7 if mode else 6, mode, 0))


@pytest.mark.parametrize("shape,bm", PWK_DG)
def test_pwk8_data_gradient_instantiation(be, shape, bm):
    """residual + PLAIN post statistics of the layer below, 170 rows, K = 96"""
    import test_k_pw as tp
    with knobs(be, {cabi.MDS_KNOB_PWK: 2, cabi.MDS_KNOB_PWK_BM: 0 if shape == 2 else bm}):
        tp._run_pw_plain(be, "bf16", 170, 96, PWK_N[shape], True, False, 1, False, frag=True)
        hit(be, pwk_inst(shape, bm, 6, 0, 1))
