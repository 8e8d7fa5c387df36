"""mds_stem_dgrad (the stem's data gradient: transposed 3x3 stride-2 TF-SAME convolution, 32 -> 3) through the C ABI, on
the simulator and on the gfx950 library, against float64 autograd through F.conv2d."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from backends import be, DT, assert_close  # noqa: F401
from mds import cabi, geometry as geo


def gen(s):
    return torch.Generator().manual_seed(s)


def _case(N, H, W, Cout, dt, seed):
    """rounded operands + the float64 reference dx (N, 3, H, W)"""
    code, tdt = DT[dt]
    g = gen(seed)
    OH, OW, pt, pl = geo.conv_geometry(H, W, 2)
    (pt_, pb), (pl_, pr) = geo.same_pad(H, 2), geo.same_pad(W, 2)
    assert (pt_, pl_) == (pt, pl)
    w = (torch.randn(Cout, 3, 3, 3, generator=g) * 0.3).to(tdt)
    dy = torch.randn(N, OH, OW, Cout, generator=g).to(tdt)            # channels-last, as the kernel reads it
    x = torch.zeros(N, 3, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (pl_, pr, pt_, pb)), w.double(), None, 2)
    assert y.shape == (N, Cout, OH, OW)
    y.backward(dy.double().permute(0, 3, 1, 2))
    wp = torch.zeros(Cout, 32)
    wp[:, :27] = w.float().view(Cout, 27)                             # MDS_PACK_STEM: k = plane*9 + ky*3 + kx, zero padded to 32
    return dict(code=code, tdt=tdt, OH=OH, OW=OW, pt=pt, pl=pl, w=wp.to(tdt), dy=dy, ref=x.grad)


def _launch(be, c, N, H, W, Cout, **kw):
    dx = be.out((N, 3, H, W), torch.float32, float("nan"))
    be.call("stem_dgrad", cabi.make("mds_stem_dgrad_args", dtype=c["code"], N=N, H=H, W=W, OH=c["OH"], OW=c["OW"], Cout=Cout,
                                    pad_t=c["pt"], pad_l=c["pl"], w=be.t(c["w"]), dx=dx, **kw))
    be.sync()
    return dx


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,H,W", [(2, 20, 36), (1, 17, 23), (3, 6, 70), (2, 40, 150)])
def test_stem_dgrad(be, dt, N, H, W):
    c = _case(N, H, W, 32, dt, H * W)
    dx = _launch(be, c, N, H, W, 32, dy=be.t(c["dy"]))
    assert not torch.isnan(dx).any(), "an element of dx was not written"
    assert_close(dx, c["ref"], dt, msg="dx")
    again = _launch(be, c, N, H, W, 32, dy=be.t(c["dy"]))
    assert torch.equal(dx, again), "two launches differ"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stem_dgrad_cout16(be, dt):
    N, H, W = 2, 17, 36                       # odd H (pad 1), W a multiple of 4 (vector stores)
    c = _case(N, H, W, 16, dt, 161)
    dx = _launch(be, c, N, H, W, 16, dy=be.t(c["dy"]))
    assert not torch.isnan(dx).any()
    assert_close(dx, c["ref"], dt, msg="dx")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("gmode", [cabi.MDS_G_PLAIN, cabi.MDS_G_SILU])
@pytest.mark.parametrize("N,H,W", [(2, 20, 36), (1, 17, 70)])
def test_stem_dgrad_forms_dy_on_load(be, dt, gmode, N, H, W):
    """dy = A*g + B*y + D, g = u or u*silu'(y*scale + shift), formed while staging - against the same launch fed the materialised dy
    (what mds_bn_bwd_apply would have written, rounded to the storage type)"""
    c = _case(N, H, W, 32, dt, H * W + gmode)
    tdt = c["tdt"]
    g = gen(H * W + gmode + 1)
    OH, OW = c["OH"], c["OW"]
    u = torch.randn(N, OH, OW, 32, generator=g).to(tdt)
    y = torch.randn(N, OH, OW, 32, generator=g).to(tdt)
    bn = torch.randn(4, 32, generator=g) * 0.5
    lin = torch.randn(3, 32, generator=g) * 0.5
    z = y.float() * bn[0] + bn[1]
    sg = torch.sigmoid(z)
    gg = u.float() * (sg * (1 + z * (1 - sg))) if gmode == cabi.MDS_G_SILU else u.float()
    dy = (lin[0] * gg + lin[1] * y.float() + lin[2]).to(tdt)
    mat = _launch(be, c, N, H, W, 32, dy=be.t(dy))
    fused = _launch(be, c, N, H, W, 32, dy=None,
                    dyp=cabi.make("mds_dyp_t", mode=1, g=cabi.gsrc(gmode, be.t(u)), y=be.t(y), bn=be.t(bn), lin=be.t(lin)))
    assert not torch.isnan(fused).any()
    # both round dy to the storage type before the products; the formed value comes from hardware exp / rcp: a storage-type ulp
    assert_close(fused, mat, dt, msg="dx")


def test_stem_dgrad_bad_arguments_are_codes(be):
    c = _case(1, 8, 8, 32, "f32", 3)
    dx = be.out((1, 3, 8, 8), torch.float32, 0)
    base = dict(dtype=c["code"], N=1, H=8, W=8, OH=c["OH"], OW=c["OW"], Cout=32, pad_t=c["pt"], pad_l=c["pl"], w=be.t(c["w"]),
                dy=be.t(c["dy"]), dx=dx)
    for bad in (dict(Cout=24), dict(dy=None), dict(dx=None), dict(pad_l=2), dict(N=0)):
        a = cabi.make("mds_stem_dgrad_args", **dict(base, **bad))
        rc = be.rc("stem_dgrad", a)
        assert rc == cabi.MDS_ERR_BAD_ARG and b"stem_dgrad" in be.lib.dll.mds_last_error(), bad
