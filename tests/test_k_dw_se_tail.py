"""mds_dw_fwd with the squeeze-excite tail (mds_se_tail_t, csrc/se_tail.h): the block that completes an image's pooled means
also computes its gate.  y and pooled must be bit-identical to the launch without the tail; gate and hidden are compared with
mds_se_fc_fwd on the same pooled row (same backend) and with a float64 torch evaluation of the formula, both at the bar
tests/test_k_elem.py::test_se_forward_backward applies to mds_se_fc_fwd's gate (backends.tol("f32"): the FCs are fp32 whatever
the storage dtype).

Observed maxima over every case below: simulator - gate and hidden equal mds_se_fc_fwd's bit for bit, gate 5.6e-7 and hidden
8.1e-7 against float64 (fp32 rounding of sums of up to 1152 terms); MI355X - bit for bit as well against
mds_se_fc_fwd, gate 5.9e-7 and hidden 9.9e-7 against float64."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from backends import be, DT, assert_close  # noqa: F401
from mds import cabi, geometry as geo

# what output buffers hold before a launch: every element is compared with a reference afterwards, so an element the kernel
# did not write fails its comparison.  (Finite on purpose: freed NaN-filled blocks go back to torch's caching allocator and
# later tests' torch.empty buffers start from them.)
UNWRITTEN = -77.0


@pytest.fixture(autouse=True, scope="module")
def _leave_the_allocator_as_found():
    """the GPU cases of this file allocate (and free) full-size tensors: give the blocks back to the driver afterwards, so
    that later test files start from the caching allocator they would have had without this one"""
    yield
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def build(be, dt, N, H, W, mid, R, stride, kt, cin, seed=0):
    """arguments of one pooling launch (every tensor on the backend's device) without the tail, and the tail's struct fields"""
    code, tdt = DT[dt]
    g = torch.Generator().manual_seed(seed + 7 * mid + R + 100 * stride + H * W + N + kt)
    T = 5 if kt == 3 else 1
    OH, OW, pt, pl = geo.conv_geometry(H, W, stride)
    kw = dict(dtype=code, N=N, T=T, IH=H, IW=W, C=mid, OH=OH, OW=OW, stride=stride, pad_t=pt, pad_l=pl, kt=kt,
              w=be.t(torch.randn(mid, kt * 9, generator=g) * 0.3), pro=cabi.pro(0), stats=None,
              epi=cabi.make("mds_epi_t", mode=2, scale=be.t(1 + 0.3 * torch.randn(mid, generator=g)),
                            shift=be.t(0.4 * torch.randn(mid, generator=g))),
              pool_inv=1.0 / (T * OH * OW))
    if cin:
        x = (torch.randn(N, H, W, cin, generator=g) * 0.5)
        kw.update(x=None, expand=cabi.make("mds_expand_t", x=be.t(x, tdt), w=be.t(torch.randn(mid, cin, generator=g) / cin ** 0.5, tdt),
                                           cin=cin, scale=be.t(1 + 0.2 * torch.randn(mid, generator=g)),
                                           shift=be.t(0.3 + 0.3 * torch.randn(mid, generator=g))))
    else:
        kw.update(x=be.t(torch.randn(N, T, H, W, mid, generator=g), tdt))
    w2 = torch.randn(mid, R, generator=g) * 0.3
    se = dict(R=R, w1=be.t(torch.randn(R, mid, generator=g) * 0.3), b1=be.t(torch.randn(R, generator=g) * 0.1),
              w2=be.t(w2), w2t=be.t(w2.t()), b2=be.t(torch.randn(mid, generator=g) * 0.1))
    return kw, se, (N, T, OH, OW, mid, tdt)


def launch(be, kw, shape, se=None, ticket=None):
    N, T, OH, OW, mid, tdt = shape
    y = be.out((N, T, OH, OW, mid), tdt, UNWRITTEN)
    pooled = be.out((N, mid), torch.float64, 0)
    out = {}
    extra = {}
    if se is not None:
        out = dict(hidden=be.out((N, se["R"]), torch.float32, UNWRITTEN), gate=be.out((N, mid), torch.float32, UNWRITTEN))
        extra["se"] = cabi.make("mds_se_tail_t", R=se["R"], w1=se["w1"], b1=se["b1"], w2t=se["w2t"], b2=se["b2"], ticket=ticket, **out)
    be.call("dw_fwd", cabi.make("mds_dw_fwd_args", y=y, pool=pooled, **kw, **extra))
    be.sync()
    return y, pooled, out.get("hidden"), out.get("gate")


def se_fc(be, se, pooled):
    N, mid = pooled.shape
    hidden = be.out((N, se["R"]), torch.float32, float("nan"))
    gate = be.out((N, mid), torch.float32, float("nan"))
    be.call("se_fc_fwd", cabi.make("mds_se_fc_fwd_args", groups=N, C=mid, R=se["R"], pooled=pooled, w1=se["w1"], b1=se["b1"],
                                   w2=se["w2"], b2=se["b2"], hidden=hidden, gate=gate, w2t=se["w2t"]))
    be.sync()
    return hidden, gate


# (N, H, W, mid, R, stride, kt, cin): (mid, R) pairs of the b0 encoder's inverted-residual blocks (mds/structure.py: 192/12, 384/24,
# 576/24, 672/28, 1152/48) and of the basic configuration's 3D blocks (256 x 3 = 768 / 32); cin != 0: with the expansion prologue
# (k_dwx.hip)
CASES = [
    (3, 9, 13, 192, 12, 2, 1, 0),
    (1, 12, 20, 384, 24, 1, 1, 0),
    (3, 7, 10, 576, 24, 1, 1, 0),
    (1, 12, 13, 672, 28, 2, 1, 0),     # a half-filled last channel chunk
    (3, 6, 9, 1152, 48, 1, 1, 0),      # the widest block
    (3, 2, 8, 64, 16, 1, 1, 0),        # one block per launch: its 8 strips straddle all three images
    (3, 9, 13, 192, 12, 2, 1, 48),
    (1, 12, 20, 384, 24, 1, 1, 96),
    (3, 8, 8, 64, 16, 1, 1, 16),       # expansion: a single block per image (one 8 x 8 tile, one channel chunk)
    (1, 6, 9, 1152, 48, 1, 1, 192),
    (3, 5, 6, 672, 28, 2, 1, 112),
    (3, 4, 6, 192, 48, 1, 3, 0),       # 3x3x3, T = 5
    (1, 5, 7, 768, 32, 1, 3, 0),
    (3, 1, 5, 64, 16, 1, 3, 0),        # 3x3x3: one block, three images
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,H,W,mid,R,stride,kt,cin", CASES)
def test_tail_matches_se_fc_fwd(be, dt, N, H, W, mid, R, stride, kt, cin):
    kw, se, shape = build(be, dt, N, H, W, mid, R, stride, kt, cin)
    y0, p0, _, _ = launch(be, kw, shape)
    ticket = be.out(N, torch.int32, 0)
    y1, p1, hidden, gate = launch(be, kw, shape, se, ticket)
    # the tail only adds work after y and pooled (fp64 sums: order-independent to 1e-16, and the flush order is the launch's own)
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(y1.cpu().view(bits), y0.cpu().view(bits)), "y changed"
    if be.name == "emu":          # blocks run in one order: the atomic sums are bit-identical too
        assert torch.equal(p1.cpu(), p0.cpu())
    else:                         # fp64 atomics in a run-dependent order: identical to the last bits of a double
        assert (p1 - p0).abs().max().item() <= 1e-13 * max(1.0, p0.abs().max().item())
    assert int(ticket.abs().sum()) == 0, "tickets reset themselves"
    h_fc, g_fc = se_fc(be, se, p1)
    eg, eh = (gate - g_fc).abs().max().item(), (hidden - h_fc).abs().max().item()
    p64 = p1.cpu()
    h64 = p64.float().double() @ se["w1"].cpu().double().t() + se["b1"].cpu().double()
    g64 = torch.sigmoid(F.silu(h64) @ se["w2"].cpu().double().t() + se["b2"].cpu().double())
    print(f"[se tail {be.name} {dt} {(N, H, W, mid, R, stride, kt, cin)}] vs se_fc_fwd: gate {eg:.3e} hidden {eh:.3e}; "
          f"vs float64: gate {(gate.cpu().double() - g64).abs().max().item():.3e} hidden {(hidden.cpu().double() - h64).abs().max().item():.3e}")
    assert_close(gate, g_fc, "f32", msg="gate vs se_fc_fwd")
    assert_close(hidden, h_fc, "f32", msg="hidden vs se_fc_fwd")
    assert_close(gate, g64, "f32", msg="gate vs float64")
    assert_close(hidden, h64, "f32", msg="hidden vs float64")


@pytest.mark.parametrize("N,H,W,mid,R,stride,kt,cin", [(3, 9, 13, 192, 12, 2, 1, 0), (3, 7, 10, 576, 24, 1, 1, 0),
                                                      (3, 9, 13, 192, 12, 2, 1, 48), (3, 4, 6, 192, 48, 1, 3, 0)])
def test_relaunch_gives_the_same_gate(be, N, H, W, mid, R, stride, kt, cin):
    """the same arguments three times on one stream, pooled re-zeroed between launches as the plan does: the ticket resets itself"""
    kw, se, shape = build(be, "f32", N, H, W, mid, R, stride, kt, cin, seed=3)
    ticket = be.out(N, torch.int32, 0)
    _, T, OH, OW, _, tdt = shape
    y = be.out((N, T, OH, OW, mid), tdt, float("nan"))
    pooled = be.out((N, mid), torch.float64, 0)
    hidden, gate = be.out((N, R), torch.float32, float("nan")), be.out((N, mid), torch.float32, float("nan"))
    args = cabi.make("mds_dw_fwd_args", y=y, pool=pooled, **kw,
                     se=cabi.make("mds_se_tail_t", R=R, w1=se["w1"], b1=se["b1"], w2t=se["w2t"], b2=se["b2"], hidden=hidden, gate=gate,
                                  ticket=ticket))
    gates = []
    for _ in range(3):
        pooled.zero_()
        gate.fill_(UNWRITTEN)
        be.call("dw_fwd", args)
        be.sync()
        assert int(ticket.abs().sum()) == 0
        gates.append(gate.clone())
    assert ((gates[0] > 0) & (gates[0] < 1)).all(), "every gate written"
    tol = 0.0 if be.name == "emu" else 1e-6      # GPU: pooled differs in the last bits of a double between runs
    assert (gates[1] - gates[0]).abs().max().item() <= tol and (gates[2] - gates[0]).abs().max().item() <= tol


@pytest.mark.parametrize("cin", [0, 48])
def test_unsupported_combinations_are_refused(be, cin):
    """no pool, no output transform, no w2t, misaligned pointers, R or C beyond the tail's sizes: an error code and a message, and
    the next valid launch works"""
    N, mid, R = 2, 192, 12
    kw, se, shape = build(be, "f32", N, 9, 13, mid, R, 1, 1, cin, seed=4)
    _, T, OH, OW, _, tdt = shape
    y = be.out((N, T, OH, OW, mid), tdt, float("nan"))
    pooled = be.out((N, mid), torch.float64, 0)
    hidden, gate = be.out((N, R), torch.float32, float("nan")), be.out((N, mid), torch.float32, float("nan"))
    ticket = be.out(N, torch.int32, 0)
    pad = be.out(R * mid + 4, torch.float32, 0)

    def tail(**over):
        f = dict(R=R, w1=se["w1"], b1=se["b1"], w2t=se["w2t"], b2=se["b2"], hidden=hidden, gate=gate, ticket=ticket)
        f.update(over)
        return cabi.make("mds_se_tail_t", **f)

    def rc(se_struct, **over):
        k = dict(kw, y=y, pool=pooled)
        k.update(over)
        code = be.rc("dw_fwd", cabi.make("mds_dw_fwd_args", se=se_struct, **k))
        return code, be.lib.dll.mds_last_error().decode()

    bad = [
        ("pool", rc(tail(), pool=None, pool_inv=0.0)),
        ("transform", rc(tail(), epi=cabi.make("mds_epi_t", mode=0, scale=None, shift=None))),
        ("w2t", rc(tail(w2t=None))),
        ("aligned", rc(tail(w1=pad[1:1 + R * mid]))),
        ("aligned", rc(tail(w2t=pad[1:1 + R * mid]))),
        ("R must be", rc(tail(R=cabi.MDS_SE_TAIL_RMAX + 1))),
        ("null", rc(tail(ticket=None))),
    ]
    for word, (code, msg) in bad:
        assert code < 0 and word in msg, (word, code, msg)
    # C beyond the tail's registers (an aligned launch of that width would be valid without the tail)
    Cb = cabi.MDS_SE_TAIL_CMAX + 64
    if not cin:
        kwb, seb, shb = build(be, "f32", 1, 4, 8, Cb, 8, 1, 1, 0, seed=5)
        yb = be.out((1, 1, 4, 8, Cb), torch.float32, float("nan"))
        pb = be.out((1, Cb), torch.float64, 0)
        t = cabi.make("mds_se_tail_t", R=8, w1=seb["w1"], b1=seb["b1"], w2t=seb["w2t"], b2=seb["b2"], hidden=be.out((1, 8), torch.float32, float("nan")),
                      gate=be.out((1, Cb), torch.float32, float("nan")), ticket=ticket)
        code = be.rc("dw_fwd", cabi.make("mds_dw_fwd_args", y=yb, pool=pb, se=t, **kwb))
        assert code < 0 and "C <=" in be.lib.dll.mds_last_error().decode()
    # 3D stacks other than T = 5 have no pooling kernel, with or without the tail
    code, msg = rc(tail(), kt=3, T=3) if not cin else (-1, "sliding-window")
    assert code < 0 and ("sliding-window" in msg)
    assert int(ticket.abs().sum()) == 0
    # a following valid launch succeeds
    be.call("dw_fwd", cabi.make("mds_dw_fwd_args", y=y, pool=pooled, se=tail(), **kw))
    be.sync()
    h_fc, g_fc = se_fc(be, se, pooled)
    assert_close(gate, g_fc, "f32", msg="gate after refusals")
