"""Depthwise (2D/3D) and stem kernels against torch conv / autograd references."""
import pytest
import torch
import torch.nn.functional as F

from backends import be, DT, ABS, U, bf16_ulp, assert_close, assert_sum_close, assert_stats_close, assert_post_close, pro_operand  # noqa: F401
from mds import cabi, geometry as geo

SLOTS = cabi.MDS_STAT_SLOTS


def gen(s):
    return torch.Generator().manual_seed(s)


def to_rows(x):   # (N,C,T,H,W) -> [N][T][H][W][C]
    return x.permute(0, 2, 3, 4, 1).contiguous()


def dw_ref(a, w, stride, kt, pads):
    """a: (N,C,T,H,W) activated input, w: (C,1,kt,3,3)."""
    (pt, pb), (pl, pr) = pads
    tp = 1 if kt == 3 else 0
    a = F.pad(a, (pl, pr, pt, pb, tp, tp))
    return F.conv3d(a, w, None, (1, stride, stride), 0, 1, a.shape[1])


DW_CASES = [  # N,T,H,W,C,stride,kt
    (2, 1, 9, 13, 48, 1, 1),
    (1, 1, 14, 37, 72, 1, 1),     # several bands/segments, half-filled channel chunk
    (3, 1, 5, 8, 136, 1, 1),
    (1, 1, 12, 18, 16, 2, 1),     # even: pad 0/1
    (2, 1, 11, 15, 24, 2, 1),     # odd: pad 1/1
    (1, 1, 12, 15, 16, 2, 1),     # mixed: pad_t 0, pad_l 1
    (1, 1, 11, 38, 72, 2, 1),     # mixed: pad_t 1, pad_l 0; several segments
    (2, 3, 5, 7, 24, 1, 3),
    (1, 5, 6, 9, 576, 1, 3),
    (2, 11, 6, 13, 72, 1, 3),     # the 33-frame configuration's stack length: time chunks of 4 / 4 / 3 slices (dw3g_*)
    (1, 4, 5, 9, 24, 1, 3),       # exactly one chunk
    (1, 9, 7, 8, 136, 1, 3),      # 4 / 4 / 1
    (3, 2, 5, 6, 16, 1, 3),
    (2, 1, 23, 37, 72, 1, 1),     # two images, ragged last strip, several strips per block at once
    # the LDS-tiled kernels (3x3x3, T != 5) past one 8 x 16 tile:
    (1, 3, 9, 37, 24, 1, 3),      # three column tiles (the backward walks two per block: grid.x = 2, the second block's walk ends early), two row bands - the second ragged -, a partly filled channel slab
    (2, 1, 5, 7, 24, 1, 3),       # T = 1: a slice ring without a prefetch, both time neighbours out of range
]
DW_TILED_WIDE = DW_CASES[-2]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,T,H,W,C,stride,kt", DW_CASES)
def test_dw_fwd_bwd(be, dt, N, T, H, W, C, stride, kt):
    _dw_fwd_bwd(be, dt, N, T, H, W, C, stride, kt)


@pytest.mark.parametrize("length", [5, 7, 13])
@pytest.mark.parametrize("N,T,H,W,C,stride,kt", [(1, 1, 14, 37, 72, 1, 1), (2, 5, 6, 23, 136, 1, 3)])
def test_dw_strip_lengths(be, length, N, T, H, W, C, stride, kt):
    """the launchers pick the strip length from the block count (dw2_len / dw3_len); any length gives the same result:
    forced lengths with ragged last segments, several segments per row"""
    knob = cabi.MDS_KNOB_DW2_L if kt == 1 else cabi.MDS_KNOB_DW3_L
    be.lib.check(be.lib.fn["dev_set"](knob, length), "dev_set")
    try:
        _dw_fwd_bwd(be, "bf16", N, T, H, W, C, stride, kt)
    finally:
        be.lib.fn["dev_set"](knob, 0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,T,H,W,C,stride,kt", [c for c in DW_CASES if c[5] == 1 and c[6] == 1])
def test_dw_fwd_six_row_bands(be, dt, N, T, H, W, C, stride, kt):
    """small launches take two-row bands (dw2_fwd_kernel<T, 2>); the six-row form that every training layer uses is forced here"""
    be.lib.check(be.lib.fn["dev_set"](cabi.MDS_KNOB_DW2_R, 1), "dev_set")
    try:
        _dw_fwd_bwd(be, dt, N, T, H, W, C, stride, kt)
        test_dw_fwd_output_transform(be, dt, N, T, H, W, C, stride, kt)
    finally:
        be.lib.fn["dev_set"](cabi.MDS_KNOB_DW2_R, 0)


def _cut(t, dim):
    """t without its last index along dim"""
    return t.narrow(dim, 0, t.shape[dim] - 1)


def _pix_probes(v):
    """wrong sums over [N][T][H][W][C] (or [N][H][W][C]) at the strip kernels' seams: the strip end, a band's row, the image"""
    h = v.dim() - 3
    pr = [("last column left out", lambda t: _cut(t, h + 1)), ("row 0 counted twice", lambda t: torch.cat([t, t.narrow(h, 0, 1)], h))]
    return pr + [("last image left out", lambda t: t[:-1]) if v.shape[0] > 1 else ("last row left out", lambda t: _cut(t, h))]


def _dw_fwd_bwd(be, dt, N, T, H, W, C, stride, kt, act_rounded=False):
    """The reference is float64.  What k_dw.hip sums (read in the kernels, all of them alike):
    the activation silu(x * scale + shift) stays in fp32 registers - it is NOT rounded to the storage type on its way into the
    products - and the forward statistics, the weight gradient and sum g / sum g * xhat are taken of the fp32 register values
    (acc before the store, gv before the store).  The reference is fed the same: x rounded to the storage type, the fp32 tables
    the kernel is handed, an un-rounded activation.  The one exception is the LDS-tiled bf16 FORWARD dw_fwd_kernel<bf16_t>,
    which bf16 launches reach only under MDS_KNOB_DW3G = 1: its tile holds the activation in the storage type (act_rounded)."""
    rd = torch.float64
    code, tdt = DT[dt]
    g = gen(H * W + C + kt)
    x = (torch.randn(N, C, T, H, W, generator=g) * 1.3).to(tdt)
    w = torch.randn(C, 1, kt, 3, 3, generator=g) * 0.3
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(rd); beta = (0.2 * torch.randn(C, generator=g)).to(rd)
    eps = 1e-3
    OH, OW, pt, pl = geo.conv_geometry(H, W, stride)
    pads = (geo.same_pad(H, stride), geo.same_pad(W, stride)) if stride == 2 else ((1, 1), (1, 1))
    # reference: a = silu(bn(x)) with the batch statistics held constant (the fp32 tables the kernels read); y = dw(a)
    xf = x.to(rd)
    wf = w.to(rd).requires_grad_(True)
    mean = xf.mean((0, 2, 3, 4)); var = xf.var((0, 2, 3, 4), unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    scale = gamma * rstd; shift = beta - mean * scale
    scale, shift, mean, rstd = (t.float().to(rd) for t in (scale, shift, mean, rstd))
    cv = lambda t: t.view(1, -1, 1, 1, 1)      # noqa: E731
    z = (xf * cv(scale) + cv(shift)).requires_grad_(True)
    a = F.silu(z)
    yref = dw_ref(a, wf, stride, kt, pads)
    dyt = torch.randn(yref.shape, generator=g).to(tdt)
    yref.backward(dyt.to(rd))
    zmag_ = (xf * cv(scale)).abs() + cv(shift).abs()
    if act_rounded:     # the forward's own operand: rounded to bf16, one ulp of doubt on the near-tie elements
        aq, aqerr = pro_operand(z.detach(), zmag_, True, "bf16")
        yfwd = dw_ref(aq, w.to(rd), stride, kt, pads)
    # magnitudes: the same products on absolute values, and on the bound of the fp32 activation's own error
    # (the training-size cases of tests/test_deterministic_kernels.py: the magnitudes need percent accuracy - float32 on the device;
    # no probes there: a bound that grows like the square of the pixel count no longer resolves a column)
    big = be.name != "emu" and x.numel() > 4_000_000
    md = dict(device=be.device, dtype=torch.float32) if big else dict(device=x.device, dtype=rd)
    zd, zmag_ = z.detach().to(md["device"]), zmag_.to(md["device"])
    aerr = pro_operand(zd, zmag_, True, "f32")[1].to(**md)
    a_m, dy_m, wabs = F.silu(zd).to(**md), dyt.to(**md), w.to(**md).abs()

    def grads(act, dyv):
        """(d/d act, d/d w) of sum(dw(act, w) * dyv) at w = |w|: the data- and weight-gradient products on given magnitudes"""
        act = act.detach().clone().requires_grad_(True); ww = wabs.clone().requires_grad_(True)
        dw_ref(act, ww, stride, kt, pads).backward(dyv)
        return act.grad, ww.grad

    def grads_w(dyv):
        return grads(a_m, dyv)[1]       # (linear in w: the same at any w)
    vabs = to_rows(dw_ref(a_m.abs(), wabs, stride, kt, pads)).double().cpu()
    verr = to_rows(dw_ref(aqerr if act_rounded else aerr, wabs, stride, kt, pads)).double().cpu()
    damag, dwmag = grads(a_m.abs(), dy_m.abs())
    dwerr = grads(aerr, dy_m.abs())[1]
    # forward kernel
    xd = be.t(to_rows(x)); wd = be.t(w.view(C, kt * 9))
    scd, shd = be.t(scale.float()), be.t(shift.float())
    y = be.out((N, T, OH, OW, C), tdt, float("nan"))
    st = be.out((SLOTS, 2, C), torch.float64, 0)
    pro = cabi.pro(2, scd, shd)
    be.call("dw_fwd", cabi.make("mds_dw_fwd_args", dtype=code, N=N, T=T, IH=H, IW=W, C=C, OH=OH, OW=OW, stride=stride,
                                pad_t=pt, pad_l=pl, kt=kt, x=xd, w=wd, y=y, pro=pro, stats=st))
    be.sync()
    yr = to_rows(yfwd if act_rounded else yref.detach())
    assert_close(y, yr, dt, msg="y")
    cnt = N * T * OH * OW
    assert_stats_close(st.sum(0), yr, vabs, 9 * kt, cnt, (dt, cnt ** 0.5), verr, () if big else _pix_probes(yr))
    # backward kernel
    gout = be.out((N, T, H, W, C), tdt, float("nan"))
    dw = be.out((C, kt * 9), torch.float32, 0, name="dw")
    st2 = be.out((SLOTS, 2, C), torch.float64, 0)     # backward sums: fp64 slots
    be.call("dw_bwd", cabi.make("mds_dw_bwd_args", dtype=code, N=N, T=T, IH=H, IW=W, C=C, OH=OH, OW=OW, stride=stride,
                                pad_t=pt, pad_l=pl, kt=kt, x=xd, dy=be.t(to_rows(dyt)), w=wd, g=gout, dw=dw, pro=pro,
                                mean=be.t(mean.float()), rstd=be.t(rstd.float()), stats=st2))
    be.sync()
    gref = to_rows(z.grad)
    assert_close(gout, gref, dt, msg="g")
    dcut = dy_m.clone(); dcut[..., -1] = 0
    probes = [] if big else [("last output column left out", grads_w(dcut)), ("ky / kx transposed", wf.grad.transpose(3, 4))]
    assert_sum_close(dw, wf.grad.view(C, kt * 9), [(cnt, dwmag.view(C, kt * 9)), (ABS, dwerr.view(C, kt * 9))], "dw",
                     [(n, p.reshape(C, kt * 9)) for n, p in probes], cap=(dt, cnt ** 0.5))
    # sum g, sum g * xhat: of gv = (sum dy * w) * silu'(z) as the registers hold it.  Its own error: the 9 kt products' sum,
    # silu' = s (1 + z (1 - s)) through v_exp / v_rcp (as pro_operand: (|z| + 12) U of its magnitude), z's rounding through |silu''| <= 1/2
    sg = torch.sigmoid(zd)
    gerr = (U * damag.double() * ((9 * kt + zd.abs() + 12) * sg * (1 + zd.abs() * (1 - sg)) + 0.5 * zmag_)).cpu()
    xhat, xmag = to_rows((xf - cv(mean)) * cv(rstd)), to_rows((xf.abs() + cv(mean).abs()) * cv(rstd))
    cin = N * T * H * W
    assert_post_close(st2.sum(0), gref, xhat, xmag, (dt, cin ** 0.5), () if big else _pix_probes(gref), gerr=to_rows(gerr))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,T,H,W,C,stride,kt", [c for c in DW_CASES if c[6] == 1 or c[1] == 5])
def test_dw_fwd_output_transform(be, dt, N, T, H, W, C, stride, kt):
    """inference form: the input already is an activation (no prologue), the output is stored as silu(bn(y)) (mds_epi_t)"""
    code, tdt = DT[dt]
    g = gen(H * W + C + kt + 7)
    x = torch.randn(N, C, T, H, W, generator=g).to(tdt)
    w = torch.randn(C, 1, kt, 3, 3, generator=g) * 0.3
    esc = 1 + 0.3 * torch.randn(C, generator=g); esh = 0.4 * torch.randn(C, generator=g)
    OH, OW, pt, pl = geo.conv_geometry(H, W, stride)
    pads = (geo.same_pad(H, stride), geo.same_pad(W, stride)) if stride == 2 else ((1, 1), (1, 1))
    ref = F.silu(dw_ref(x.float(), w, stride, kt, pads) * esc.view(1, -1, 1, 1, 1) + esh.view(1, -1, 1, 1, 1))
    y = be.out((N, T, OH, OW, C), tdt, float("nan"))
    # (kt == 1: T == 1 in every case; the pooled means of the STORED output come out of the same pass - mds_dw_fwd_args.pool)
    pool = be.out((N, C), torch.float64, 0)
    be.call("dw_fwd", cabi.make("mds_dw_fwd_args", dtype=code, N=N, T=T, IH=H, IW=W, C=C, OH=OH, OW=OW, stride=stride, pad_t=pt,
                                pad_l=pl, kt=kt, x=be.t(to_rows(x)), w=be.t(w.view(C, kt * 9)), y=y, pro=cabi.pro(0), stats=None,
                                epi=cabi.make("mds_epi_t", mode=2, scale=be.t(esc), shift=be.t(esh)),
                                pool=pool, pool_inv=1.0 / (T * OH * OW)))
    be.sync()
    assert_close(y, to_rows(ref), dt, msg="y")
    want = y.float().cpu().double().mean((1, 2, 3))
    assert (pool.cpu() - want).abs().max() <= 2e-6 * max(1.0, float(want.abs().max())), "pooled means of the stored output"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,H,W", [(2, 20, 36), (1, 17, 23), (3, 6, 70), (2, 40, 150)])      # (the last: 3 x 3 tiles of the tiled kernels per image)
def test_stem_fwd_wgrad(be, dt, N, H, W):
    """the reference is float64"""
    rd = torch.float64
    code, tdt = DT[dt]
    g = gen(H * W)
    x = torch.rand(N, 3, H, W, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g) * 0.3
    OH, OW, pt, pl = geo.conv_geometry(H, W, 2)
    (pt_, pb), (pl_, pr) = geo.same_pad(H, 2), geo.same_pad(W, 2)
    xq = x.to(tdt).to(rd)
    wq = w.to(tdt).to(rd).requires_grad_(True)
    yref = F.conv2d(F.pad(xq, (pl_, pr, pt_, pb)), wq, None, 2)
    dyt = torch.randn(yref.shape, generator=g).to(tdt)
    yref.backward(dyt.to(rd))
    wp = torch.zeros(32, 32); wp[:, :27] = w.view(32, 27)
    y = be.out((N, OH, OW, 32), tdt, float("nan"))
    st = be.out((SLOTS, 2, 32), torch.float64, 0)
    xd = be.t(x)
    be.call("stem_fwd", cabi.make("mds_stem_fwd_args", dtype=code, N=N, H=H, W=W, OH=OH, OW=OW, Cout=32, pad_t=pt, pad_l=pl,
                                  x=xd, w=be.t(wp.to(tdt)), y=y, stats=st))
    dw = be.out((32, 3, 3, 3), torch.float32, 0, name="dw")
    be.call("stem_wgrad", cabi.make("mds_stem_wgrad_args", dtype=code, N=N, H=H, W=W, OH=OH, OW=OW, Cout=32, pad_t=pt,
                                    pad_l=pl, x=xd, dy=be.t(dyt.permute(0, 2, 3, 1)), dw=dw))
    be.sync()
    yr = yref.detach().permute(0, 2, 3, 1)
    assert_close(y, yr, dt, msg="y")
    cnt = N * OH * OW
    # (the training-size case of tests/test_deterministic_kernels.py: magnitudes in float32 on the device, no probes - as _dw_fwd_bwd)
    big = be.name != "emu" and x.numel() > 4_000_000
    md = dict(device=be.device, dtype=torch.float32) if big else dict(device=x.device, dtype=rd)
    vabs = F.conv2d(F.pad(xq.to(**md), (pl_, pr, pt_, pb)), wq.detach().to(**md).abs(), None, 2).permute(0, 2, 3, 1).double().cpu()      # (x >= 0)
    assert_stats_close(st.sum(0), yr, vabs, 27, cnt, (dt, cnt ** 0.5), None, () if big else _pix_probes(yr))
    d64 = dyt.to(rd)
    probes = []
    if not big:
        dcut = d64.clone(); dcut[..., -1] = 0
        probes = [("last output column left out", stem_wgrad64(xq, dcut)), ("ky / kx transposed", wq.grad.transpose(2, 3))]
        if N > 1:
            probes.append(("last image left out", stem_wgrad64(xq[:-1], d64[:-1])))
    assert_sum_close(dw, wq.grad, [(cnt, stem_wgrad64(xq.to(**md), d64.to(**md).abs()))], "dw", probes, cap=(dt, cnt ** 0.5))


def stem_wgrad64(x, dyt):
    """filter gradient of the stem's 3x3 stride-2 TF-SAME convolution (x: [N][3][H][W], dyt: [N][32][OH][OW]) in dyt's type
    (float64 everywhere but for the training-size magnitudes) on dyt's device"""
    (pt_, pb), (pl_, pr) = geo.same_pad(x.shape[2], 2), geo.same_pad(x.shape[3], 2)
    ww = torch.zeros(dyt.shape[1], 3, 3, 3, dtype=dyt.dtype, device=dyt.device, requires_grad=True)
    F.conv2d(F.pad(x.to(dyt.dtype), (pl_, pr, pt_, pb)), ww, None, 2).backward(dyt)
    return ww.grad


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stem_fwd_output_transform(be, dt):
    code, tdt = DT[dt]
    N, H, W = 2, 18, 30
    g = gen(5)
    x = torch.rand(N, 3, H, W, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g) * 0.3
    esc = 1 + 0.3 * torch.randn(32, generator=g); esh = 0.4 * torch.randn(32, generator=g)
    OH, OW, pt, pl = geo.conv_geometry(H, W, 2)
    (pt_, pb), (pl_, pr) = geo.same_pad(H, 2), geo.same_pad(W, 2)
    ref = F.silu(F.conv2d(F.pad(x.to(tdt).float(), (pl_, pr, pt_, pb)), w.to(tdt).float(), None, 2).permute(0, 2, 3, 1) * esc + esh)
    wp = torch.zeros(32, 32); wp[:, :27] = w.view(32, 27)
    y = be.out((N, OH, OW, 32), tdt, float("nan"))
    be.call("stem_fwd", cabi.make("mds_stem_fwd_args", dtype=code, N=N, H=H, W=W, OH=OH, OW=OW, Cout=32, pad_t=pt, pad_l=pl,
                                  x=be.t(x), w=be.t(wp.to(tdt)), y=y, stats=None,
                                  epi=cabi.make("mds_epi_t", mode=2, scale=be.t(esc), shift=be.t(esh))))
    be.sync()
    assert_close(y, ref, dt, msg="y")


@pytest.mark.parametrize("gmode", [cabi.MDS_G_PLAIN, cabi.MDS_G_SILU])
@pytest.mark.parametrize("N,H,W", [(2, 20, 36), (1, 17, 70)])
def test_stem_wgrad_forms_dy_on_load(be, gmode, N, H, W):
    """mds_stem_wgrad with a dy prologue (dy = A*g + B*y + D, g = u or u*silu'(y*scale + shift)) against the same kernel
    fed the materialised dy (what mds_bn_bwd_apply would have written)"""
    code, tdt = DT["bf16"]
    g = gen(H * W + gmode)
    OH, OW, pt, pl = geo.conv_geometry(H, W, 2)
    x = torch.rand(N, 3, H, W, generator=g)
    u = torch.randn(N, OH, OW, 32, generator=g).to(tdt)
    y = torch.randn(N, OH, OW, 32, generator=g).to(tdt)
    bn = torch.randn(4, 32, generator=g) * 0.5
    lin = torch.randn(3, 32, generator=g) * 0.5
    z = y.float() * bn[0] + bn[1]
    sg = torch.sigmoid(z)
    gg = u.float() * (sg * (1 + z * (1 - sg))) if gmode == cabi.MDS_G_SILU else u.float()
    dy = (lin[0] * gg + lin[1] * y.float() + lin[2]).to(tdt)
    xd = be.t(x)
    out = []
    for fused in (False, True):
        dw = be.out((32, 3, 3, 3), torch.float32, 0, name="dw")
        kw = dict(dtype=code, N=N, H=H, W=W, OH=OH, OW=OW, Cout=32, pad_t=pt, pad_l=pl, x=xd, dw=dw)
        if fused:
            kw.update(dy=None, dyp=cabi.make("mds_dyp_t", mode=1, g=cabi.gsrc(gmode, be.t(u)), y=be.t(y), bn=be.t(bn), lin=be.t(lin)))
        else:
            kw.update(dy=be.t(dy))
        be.call("stem_wgrad", cabi.make("mds_stem_wgrad_args", **kw))
        be.sync()
        out.append(dw.cpu())
    # the fused path multiplies the fp32 dy it forms, the other one the bf16-rounded dy: they differ by the rounding of dy.  The
    # rounded dy handed to the materialised launch comes from torch's float32 evaluation, the error model from float64: where the
    # two fall on different sides of a rounding boundary the stored value is up to a whole bf16 ulp from the float64 dy, elsewhere
    # half of one.  The near-tie set of a three-term fp32 expression is not worked out here: one whole ulp is charged everywhere,
    # which is at most twice the half-ulp model and stays a valid bound -
    # by the fp32 roundings of A*g + B*y + D ((|z| + 12) U as in pro_operand for the SiLU factor), and by two summation orders
    cnt, xq = N * OH * OW, x.to(tdt).double()
    l64 = lin.double()
    dy64 = l64[0] * gg.double() + l64[1] * y.double() + l64[2]
    dymag = (l64[0] * gg.double()).abs() * (1 + (z.double().abs() + 12) * U) + (l64[1] * y.double()).abs() + l64[2].abs()
    nchw = lambda t: t.permute(0, 3, 1, 2)      # noqa: E731
    mag = stem_wgrad64(xq, nchw(dy64.abs()))
    parts = [(cnt, mag), (cnt, mag), (ABS, stem_wgrad64(xq, nchw(bf16_ulp(dy64) + (z.double().abs() + 20) * U * dymag)))]
    last = torch.zeros_like(dy64); last[:, :, -1] = dy.double()[:, :, -1]
    probes = [("last output column left out", out[0].double() - stem_wgrad64(xq, nchw(last))), ("ky / kx transposed", out[0].double().transpose(2, 3))]
    assert_sum_close(out[1], out[0], parts, "dw", probes, cap=("bf16", cnt ** 0.5))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stem_fwd_uint8_ingest(be, dt):
    """raw uint8 frames -> constant pad (src/frames.py:12-31) -> /255 -> kornia hflip for the TTA copies, all
    inside the stem's gather, against the reference's pipeline followed by the convolution."""
    code, tdt = DT[dt]
    g = gen(77)
    nsrc, sh, sw, H, W = 2, 21, 38, 26, 44                      # padded size larger than the frames in both directions
    u8 = torch.randint(0, 256, (nsrc, 3, sh, sw), generator=g, dtype=torch.uint8)
    w = torch.randn(32, 3, 3, 3, generator=g) * 0.3
    hp, wp_ = H - sh, W - sw
    fr = F.pad(u8, [wp_ // 2, wp_ - wp_ // 2, hp // 2, hp - hp // 2], mode="constant", value=0).to(torch.float32) / 255.0
    x = torch.cat([fr, torch.flip(fr, dims=[-1])], dim=0)         # images 0..nsrc-1, then their mirrored copies
    N = 2 * nsrc
    OH, OW, pt, pl = geo.conv_geometry(H, W, 2)
    (pt_, pb), (pl_, pr) = geo.same_pad(H, 2), geo.same_pad(W, 2)
    yref = F.conv2d(F.pad(x.to(tdt).float(), (pl_, pr, pt_, pb)), w.to(tdt).float(), None, 2).permute(0, 2, 3, 1)
    wp = torch.zeros(32, 32); wp[:, :27] = w.view(32, 27)
    y = be.out((N, OH, OW, 32), tdt, float("nan"))
    ing = cabi.make("mds_ingest_t", u8=be.t(u8), nsrc=nsrc, src_h=sh, src_w=sw, pad_top=hp // 2, pad_left=wp_ // 2, scale=1.0 / 255.0)
    be.call("stem_fwd", cabi.make("mds_stem_fwd_args", dtype=code, N=N, H=H, W=W, OH=OH, OW=OW, Cout=32, pad_t=pt, pad_l=pl,
                                  x=None, w=be.t(wp.to(tdt)), y=y, stats=None, ingest=ing))
    be.sync()
    assert_close(y, yref, dt, msg="y")
