"""mds_dw_fwd with an expansion prologue (mds_expand_t, k_dwx.hip): 1x1 expansion + BN1 + SiLU computed in the depthwise
launch, against torch: conv1x1 -> affine -> SiLU -> zero pad -> depthwise 3x3 -> affine -> SiLU, plus the per-image means."""
import pytest
import torch
import torch.nn.functional as F

from backends import be, be_gpu, DT, assert_close  # noqa: F401
from mds import cabi, geometry as geo


def run_case(be, dt, N, H, W, cin, mid, stride, shift1=0.3, emode=2, pool=True, seed=0):
    code, tdt = DT[dt]
    g = torch.Generator().manual_seed(seed + 1000 * stride + H * W + cin + mid + N)
    x = (torch.randn(N, cin, H, W, generator=g) * 0.5).to(tdt).float()           # the activated block input
    w1 = torch.randn(mid, cin, generator=g) / cin ** 0.5
    s1 = 1 + 0.2 * torch.randn(mid, generator=g)
    b1 = shift1 + 0.3 * torch.randn(mid, generator=g)
    wd = torch.randn(mid, 1, 3, 3, generator=g) * 0.3
    s2 = 1 + 0.3 * torch.randn(mid, generator=g)
    b2 = 0.4 * torch.randn(mid, generator=g)
    OH, OW, pt, pl = geo.conv_geometry(H, W, stride)
    (ptt, pbb), (pll, prr) = ((geo.same_pad(H, stride), geo.same_pad(W, stride)) if stride == 2 else ((1, 1), (1, 1)))
    assert (ptt, pll) == (pt, pl)
    w1q = w1.to(tdt).float()                         # the kernel reads the packed (storage-dtype) filter
    y1 = F.silu(F.conv2d(x, w1q.view(mid, cin, 1, 1)) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))
    z = F.conv2d(F.pad(y1, (pll, prr, ptt, pbb)), wd, None, stride, 0, 1, mid)
    z = z * s2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)
    ref = F.silu(z) if emode == 2 else z
    ref = ref.permute(0, 2, 3, 1).contiguous()
    y = be.out((N, OH, OW, mid), tdt, float("nan"))
    pooled = be.out((N, mid), torch.float64, 0)
    exp = cabi.make("mds_expand_t", x=be.t(x.permute(0, 2, 3, 1), tdt), w=be.t(w1, tdt), cin=cin, scale=be.t(s1), shift=be.t(b1))
    be.call("dw_fwd", cabi.make("mds_dw_fwd_args", dtype=code, N=N, T=1, IH=H, IW=W, C=mid, OH=OH, OW=OW, stride=stride, pad_t=pt,
                                pad_l=pl, kt=1, x=None, w=be.t(wd.view(mid, 9)), y=y, pro=cabi.pro(0), stats=None,
                                epi=cabi.make("mds_epi_t", mode=emode, scale=be.t(s2), shift=be.t(b2)),
                                pool=pooled if pool else None, pool_inv=1.0 / (OH * OW) if pool else 0.0, expand=exp))
    be.sync()
    return y, ref, pooled


# (N, H, W, cin, mid, stride): odd / even sizes, both stride-2 pad patterns, every (cin, mid) pair of the b0 encoder's 2D blocks
EMU_CASES = [
    (1, 9, 13, 48, 192, 2),      # odd: pad 1/1
    (2, 12, 20, 48, 192, 2),     # even: pad 0/1
    (1, 12, 13, 112, 672, 2),    # mixed: pad_t 0, pad_l 1; a half-filled last channel chunk (672 = 10.5 x 64)
    (3, 9, 13, 96, 384, 1),
    (1, 12, 20, 96, 576, 1),
    (2, 9, 13, 112, 672, 1),
    (1, 12, 20, 192, 1152, 1),
    (1, 5, 3, 48, 192, 1),       # smaller than one tile
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,H,W,cin,mid,stride", EMU_CASES)
def test_dw_fwd_expand(be, dt, N, H, W, cin, mid, stride):
    y, ref, pooled = run_case(be, dt, N, H, W, cin, mid, stride)
    assert_close(y, ref, dt, msg="y")
    want = y.float().cpu().double().mean((1, 2))
    assert (pooled.cpu() - want).abs().max() <= 2e-6 * max(1.0, float(want.abs().max())), "pooled means of the stored output"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
def test_dw_fwd_expand_pads_the_activation(be, dt, stride):
    """a large BN1 shift: silu(shift) is far from 0, so a kernel that padded x (or y1 before its activation) instead of the
    activated y1 is off at every border pixel"""
    y, ref, _ = run_case(be, dt, 1, 9, 12, 48, 192, stride, shift1=3.0, pool=False, seed=5)
    assert_close(y, ref, dt, msg="y")


def test_dw_fwd_expand_affine_output(be):
    y, ref, _ = run_case(be, "f32", 2, 7, 10, 96, 384, 1, emode=1, pool=False, seed=9)
    assert_close(y, ref, "f32", msg="y")


def test_dw_fwd_expand_rejects_unsupported(be):
    """3D, a prologue or statistics with the expansion are errors, not silent fallbacks"""
    code, tdt = DT["f32"]
    z = lambda n: be.out(n, torch.float32, 0)
    exp = cabi.make("mds_expand_t", x=z(2 * 4 * 4 * 48), w=z(192 * 48), cin=48, scale=z(192), shift=z(192))
    epi = cabi.make("mds_epi_t", mode=2, scale=z(192), shift=z(192))
    base = dict(dtype=code, N=1, IH=4, IW=4, C=192, OH=4, OW=4, stride=1, pad_t=1, pad_l=1, x=None, w=z(192 * 27), y=z(16 * 192),
                stats=None, epi=epi, pool=None, pool_inv=0.0, expand=exp)
    for bad in (dict(T=2, kt=3, pro=cabi.pro(0)), dict(T=1, kt=1, pro=cabi.pro(2, z(192), z(192)))):
        a = cabi.make("mds_dw_fwd_args", **{**base, **bad})
        rc = be.rc("dw_fwd", a)
        assert rc == cabi.MDS_ERR_BAD_ARG


# one real-size case per stage of the 736 x 1280 encoder (stride-2 stage 3.0, stage 4, stage 5)
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,H,W,cin,mid,stride", [(1, 92, 160, 48, 192, 2), (2, 46, 80, 112, 672, 1), (1, 23, 40, 192, 1152, 1),
                                                  (2, 46, 80, 112, 672, 2)])
def test_dw_fwd_expand_fullsize(be_gpu, dt, N, H, W, cin, mid, stride):
    y, ref, pooled = run_case(be_gpu, dt, N, H, W, cin, mid, stride)
    assert_close(y, ref, dt, msg="y")
    want = y.float().cpu().double().mean((1, 2))
    assert (pooled.cpu() - want).abs().max() <= 2e-6 * max(1.0, float(want.abs().max())), "pooled means of the stored output"
