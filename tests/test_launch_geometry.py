"""Production-size launch geometry at small shapes.

Almost every launcher in csrc/ picks its kernel, tile size, grid and loop structure from the problem size, and the kernel tests
use a few hundred rows: they take the small-launch branch of each choice.  The developer knobs of include/mds.h force the other
branch at the same few hundred rows.  Every test here sets knobs through backends.knobs(), compares with a float64 reference fed
exactly what the kernel is fed (bf16 inputs rounded first, bf16-rounded activations where the kernel rounds them), and asserts
on the simulator's launch record that the launch really has the geometry the test is there for - a knob that stopped doing
anything would otherwise leave the test passing.  On the MI355X the same host routing code runs (mds_cu_count() is 256 on both
backends); there the values alone are checked."""
import glob
import os
import re

import pytest
import torch
import torch.nn.functional as F

import test_k_conv
import test_k_dw_stem
import test_k_pw
from test_k_elem import bn_bwd_reference, check_bn_bwd_sums, check_se_backward, silu_grad64
from backends import be, DT, ABS, U, assert_close, assert_sum_close, assert_post_close, knobs  # noqa: F401
from mds import cabi

SLOTS = cabi.MDS_STAT_SLOTS
F64 = torch.float64


def gen(s):
    return torch.Generator().manual_seed(s)


def cdiv(a, b):
    return -(-a // b)


def rows_per_pass(C):
    """elem.h: row_slices() column slices, rows_per_pass() rows of a 256-thread block per pass"""
    ns = 2 if (C // 8 > 128 and (C // 8) % 2 == 0) else 1
    return ns, max(1, 256 // (C // 8 // ns))


def q(x, tdt):
    """what a kernel that stores `tdt` leaves behind, as float64"""
    return x.to(tdt).to(F64)


def silu_grad(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def assert_trips(be, kernel, M, C, slots=2):
    """capped grid-stride kernels: every thread makes at least 3 trips; returns whether the last trip is ragged"""
    ls = be.launches(kernel)
    if ls is None:
        return None
    assert len(ls) == 1, ls
    rpp = rows_per_pass(C)[1]
    assert ls[0].gx * rpp * 2 < M, f"{kernel}: grid.x = {ls[0].gx}, {rpp} rows per pass: fewer than 3 trips over {M} rows"
    return M % (slots * ls[0].gx * rpp) != 0


# ------------------------------------------------------------------------------------------------ BatchNorm backward chain
def bn_forward_table(be, y, gamma, beta, eps):
    """[4][C] scale, shift, mean, rstd of a train-mode BatchNorm over y, through mds_bn_finalize"""
    M, C = y.shape
    stats = torch.zeros(SLOTS, 2, C, dtype=F64)
    stats[0, 0] = y.to(F64).sum(0); stats[0, 1] = (y.to(F64) ** 2).sum(0)
    out = be.out((4, C), torch.float32, float("nan"))
    be.call("bn_finalize", cabi.make("mds_bn_finalize_args", C=C, count=M, stats=be.t(stats), gamma=be.t(gamma), beta=be.t(beta),
                                     eps=eps, momentum=0.1, training=1, running_mean=None, running_var=None,
                                     num_batches_tracked=None, out=out))
    return out


# M = 330: three trips and a last trip in which the second row slot is wholly out of range (C = 40: 51 rows per pass).
# M = 766: 766 mod 2 * stride lies in (stride, 2 * stride) for every stride the caps below give - 51, 102, 153 rows at C = 40 and
# 3 rows at C = 1152 (two column slices: the cap is halved, one block) - so the last trip is ragged in BOTH slots: the first is
# full, the second ends inside a block's rows.
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,C", [(m, c) for c in (40, 1152) for m in (0, 1, 2, 3)])
@pytest.mark.parametrize("M", [330, 766])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_bn_backward_chain_grid_stride_trips(be, dt, mode, C, M, cap):
    """bn_bwd_reduce_kernel (four rolling row slots, MDS_KNOB_REDUCE_BLOCKS) and bn_bwd_apply_kernel (MDS_APPLY_SLOTS rolling
    slots, stream cap MDS_KNOB_STREAM_BLOCKS) with 1 - 3 blocks: the clamped prologue, the prefetch row rn = rr + NSL * stride
    and the ragged last trip, which the 2048- / 512-block caps reach only above a hundred thousand rows"""
    code, tdt = DT[dt]
    rpg, eps = 110, 1e-5
    G = cdiv(M, rpg)
    g = gen(11 + mode + M)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(tdt)
    u = torch.randn(M, C, generator=g).to(tdt)
    gamma = 1 + 0.2 * torch.randn(C, generator=g); beta = 0.2 * torch.randn(C, generator=g)
    gate = torch.rand(G, C, generator=g); dpool = 0.1 * torch.randn(G, C, generator=g)
    mask = torch.tensor([0.0, 1.25, 1.25, 0.0, 1.25, 1.25, 1.25][:G])
    dy_ref, dgamma_ref, dbeta_ref = bn_bwd_reference(y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps)
    bn = bn_forward_table(be, y, gamma, beta, eps)
    gs = cabi.gsrc(mode, be.t(u), be.t(gate), be.t(dpool), be.t(mask), rpg)
    st2 = be.out((SLOTS, 2, C), F64, 0)
    yd = be.t(y)
    dgamma = be.out(C, torch.float32, 0); dbeta = be.out(C, torch.float32, 0)
    coef = be.out((3, C), torch.float32, float("nan"))
    guard = 2 * 3 * 51 + 14      # rows behind dy that must stay NaN: more than the two row slots of the longest stride reach past M
    buf = be.out((M + guard, C), tdt, float("nan"))
    dy = buf[:M]
    with knobs(be, {cabi.MDS_KNOB_STREAM_BLOCKS: cap, cabi.MDS_KNOB_REDUCE_BLOCKS: cap}):
        be.call("bn_bwd_reduce", cabi.make("mds_bn_bwd_reduce_args", dtype=code, M=M, C=C, g=gs, y=yd, bn=bn, stats=st2))
        be.call("bn_bwd_finalize", cabi.make("mds_bn_bwd_finalize_args", C=C, count=M, stats=st2, gamma=be.t(gamma),
                                             bn=bn, dgamma=dgamma, dbeta=dbeta, coef=coef, batch_stats=1))
        be.call("bn_bwd_apply", cabi.make("mds_bn_bwd_apply_args", dtype=code, M=M, C=C, g=gs, y=yd, bn=bn, coef=coef, dy=dy))
        be.sync()
        assert_trips(be, "bn_bwd_reduce_kernel", M, C, slots=4)
        ragged = assert_trips(be, "bn_bwd_apply_kernel", M, C)
        if ragged is not None and M == 766:
            ns, rpp = rows_per_pass(C)
            stride = be.launches("bn_bwd_apply_kernel")[0].gx * rpp
            assert stride < M % (2 * stride) < 2 * stride, "the last trip must end inside the second slot"
        if ragged is not None and C == 40:
            assert ragged
    assert bool(torch.isnan(buf[M:].float()).all()), "bn_bwd_apply stored a row past M"
    check_bn_bwd_sums(dgamma, dbeta, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, dt)
    assert_close(dy, dy_ref, dt, scale=2, msg="dy")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,C", [(330, 40), (766, 40), (67, 1152)])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_bn_res_grid_stride_trips(be, dt, M, C, cap):
    """bn_res_kernel under the stream cap (stream_blocks in elem.h, MDS_KNOB_STREAM_BLOCKS): several trips of the grid-stride
    loop with DropPath mask + shortcut + SiLU; C = 1152: one row per pass"""
    code, tdt = DT[dt]
    g = gen(M + C)
    rpg = 40
    y = torch.randn(M, C, generator=g).to(tdt); sc_ = torch.randn(M, C, generator=g).to(tdt)
    scale = 1 + 0.2 * torch.randn(C, generator=g); shift = 0.2 * torch.randn(C, generator=g)
    mask = (torch.rand(cdiv(M, rpg), generator=g) > 0.3).float() / 0.7
    out = be.out((M, C), tdt, float("nan"))
    with knobs(be, {cabi.MDS_KNOB_STREAM_BLOCKS: cap}):
        be.call("bn_res", cabi.make("mds_bn_res_args", dtype=code, M=M, C=C, y=be.t(y), scale=be.t(scale), shift=be.t(shift), act=1,
                                    mask=be.t(mask), rows_per_group=rpg, shortcut=be.t(sc_), out=out))
        be.sync()
        ls = be.launches("bn_res_kernel")
        if ls is not None:
            rpp = max(1, 256 // (C // 8))          # (bn_res_kernel takes no column slices)
            assert len(ls) == 1 and ls[0].gx * rpp * 2 < M and M % (2 * ls[0].gx * rpp) != 0, ls
    z = F.silu(y.to(F64) * scale.to(F64) + shift.to(F64)) * mask.to(F64)[torch.arange(M) // rpg, None] + sc_.to(F64)
    assert_close(out, z, dt)


# ------------------------------------------------------------------------------------------------ grouped reduces
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,RD", [(48, 12), (1152, 48)])
def test_se_grouped_reduces_several_blocks_per_group(be, dt, C, RD):
    """se_pool_kernel / se_bwd_reduce_kernel with grid.x > 1 (group_blocks(), MDS_KNOB_REDUCE_PASSES = 1: 2 blocks per group at
    C = 48, 24 at C = 1152 with two column slices): several blocks add into pooled / dgate, `act` is written by all of them, and
    the per-block bnsums[g][blk] layout goes through mds_se_fc_bwd's bn_stats - against float64 autograd and the float64 sums of
    g = (u * gate + dpooled) * silu'(z).  Raw input (scale / shift) and the materialised activation (scale == NULL)."""
    code, tdt = DT[dt]
    G, R_ = 3, 70
    M = G * R_
    g = gen(5 + C)
    y = torch.randn(M, C, generator=g).to(tdt)
    scale = 1 + 0.2 * torch.randn(C, generator=g); shift = 0.2 * torch.randn(C, generator=g)
    mean = 0.3 * torch.randn(C, generator=g); rstd = 0.5 + torch.rand(C, generator=g)
    w1 = torch.randn(RD, C, generator=g) * 0.3; b1 = torch.randn(RD, generator=g) * 0.1
    w2 = torch.randn(C, RD, generator=g) * 0.3; b2 = torch.randn(C, generator=g) * 0.1
    u = torch.randn(M, C, generator=g).to(tdt)
    # float64 reference
    p = {k: v.to(F64).requires_grad_(True) for k, v in dict(w1=w1, b1=b1, w2=w2, b2=b2).items()}
    z = y.to(F64) * scale.to(F64) + shift.to(F64)
    a = F.silu(z).requires_grad_(True)
    pooled_ref = a.view(G, R_, C).mean(1)
    gate_ref = torch.sigmoid(F.silu(pooled_ref @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"])
    ((a.view(G, R_, C) * gate_ref[:, None, :]).reshape(M, C) * u.to(F64)).sum().backward()
    da_ref = a.grad
    g_ref = da_ref * silu_grad(z)
    xhat = (y.to(F64) - mean.to(F64)) * rstd.to(F64)
    # kernels
    yd, ud, scd, shd = be.t(y), be.t(u), be.t(scale), be.t(shift)
    w1d, b1d, w2d, b2d = be.t(w1), be.t(b1), be.t(w2), be.t(b2)
    pooled = be.out((G, C), F64, 0); pooled_m = be.out((G, C), F64, 0)
    act = be.out((M, C), tdt, float("nan"))
    hidden = be.out((G, RD), torch.float32, float("nan")); gate = be.out((G, C), torch.float32, float("nan"))
    dgate = be.out((G, C), F64, 0); dgate_m = be.out((G, C), F64, 0)
    dpooled = be.out((G, C), torch.float32, float("nan"))
    dw1 = be.out((RD, C), torch.float32, 0); db1 = be.out(RD, torch.float32, 0)
    dw2 = be.out((C, RD), torch.float32, 0); db2 = be.out(C, torch.float32, 0)
    bn_stats = be.out((SLOTS, 2, C), F64, 0)
    with knobs(be, {cabi.MDS_KNOB_REDUCE_PASSES: 1}):
        nblk = be.lib.fn["se_bwd_reduce_blocks"](R_, C)
        assert nblk >= 2
        bnsums = be.out((G, nblk, 4, C), torch.float32, float("nan"))
        be.call("se_pool", cabi.make("mds_se_pool_args", dtype=code, groups=G, rows_per_group=R_, C=C, y=yd, scale=scd, shift=shd,
                                     pooled=pooled, act=act))
        be.call("se_pool", cabi.make("mds_se_pool_args", dtype=code, groups=G, rows_per_group=R_, C=C, y=act, scale=None, shift=None,
                                     pooled=pooled_m))
        be.call("se_fc_fwd", cabi.make("mds_se_fc_fwd_args", groups=G, C=C, R=RD, pooled=pooled, w1=w1d, b1=b1d, w2=w2d, b2=b2d,
                                       hidden=hidden, gate=gate))
        be.call("se_bwd_reduce", cabi.make("mds_se_bwd_reduce_args", dtype=code, groups=G, rows_per_group=R_, C=C, u=ud, y=yd,
                                           scale=scd, shift=shd, dgate=dgate, mean=be.t(mean), rstd=be.t(rstd), bnsums=bnsums))
        be.call("se_bwd_reduce", cabi.make("mds_se_bwd_reduce_args", dtype=code, groups=G, rows_per_group=R_, C=C, u=ud, y=act,
                                           scale=None, shift=None, dgate=dgate_m))
        be.call("se_fc_bwd", cabi.make("mds_se_fc_bwd_args", groups=G, C=C, R=RD, rows_per_group=R_, dgate=dgate, gate=gate,
                                       hidden=hidden, pooled=pooled, w1=w1d, w2=w2d, dpooled=dpooled,
                                       scratch=be.out((G, RD), torch.float32, float("nan")), dw1=dw1, db1=db1, dw2=dw2, db2=db2,
                                       bnsums=bnsums, bn_nblk=nblk, bn_stats=bn_stats))
        be.sync()
        for name in ("se_pool_kernel", "se_bwd_reduce_kernel"):
            ls = be.launches(name)
            assert ls is None or (len(ls) == 2 and all(l.gx >= 2 for l in ls)), ls
        ls = be.launches("se_bwd_reduce_kernel")
        assert ls is None or ls[0].gx == nblk
    assert_close(act, F.silu(z), dt, msg="act")
    assert_close(pooled, pooled_ref, dt, msg="pooled (raw input)")
    act64 = act.cpu().to(F64)
    assert_close(pooled_m, act64.view(G, R_, C).mean(1), dt, msg="pooled (materialised input)")
    assert_close(gate, gate_ref, dt, msg="gate")
    # sums over the R_ rows of a group, the groups and the channels: float64 on the same operands + the fp32 summation bound
    check_se_backward(dict(dgate=dgate, dw1=dw1, db1=db1, dw2=dw2, db2=db2), dict(dgate=dgate, gate=gate, hidden=hidden, pooled=pooled),
                      y, scale, shift, w1, w2, u, G, R_, dt)
    um = (u.to(F64) * act64).view(G, R_, C)
    cutg = um.clone(); cutg[-1] = 0
    assert_sum_close(dgate_m, um.sum(1), [(R_, um.abs().sum(1))], "dgate (materialised input)",
                     [("last group left out", cutg.sum(1)), ("last 6 rows of every group left out", um[:, :-6].sum(1))], cap=(dt, R_ ** 0.5))
    grp = torch.arange(M) // R_
    da = u.to(F64) * gate.cpu().to(F64)[grp] + dpooled.cpu().to(F64)[grp]
    assert_close(da, da_ref, dt, scale=3, msg="da")
    s = bn_stats.sum(0).cpu()
    assert float(bn_stats[1:].abs().sum()) == 0.0, "se_fc_bwd adds the BatchNorm sums to slot 0"
    # g = (u * gate + dpooled) * silu'(z) from the KERNELS' gate and dpooled (checked above), so that the sums see the same operands
    d, dmag, derr = silu_grad64(z, (y.to(F64) * scale.to(F64)).abs() + shift.to(F64).abs())
    damag = (u.to(F64) * gate.cpu().to(F64)[grp]).abs() + dpooled.cpu().to(F64)[grp].abs()
    xmag = (y.to(F64).abs() + mean.to(F64).abs()) * rstd.to(F64)
    probes = [("last group left out", lambda t: t[:-R_]), ("first 16 rows counted twice", lambda t: torch.cat([t, t[:16]], 0))]
    assert_post_close(s, da * d, xhat, xmag, (dt, M ** 0.5), probes, gerr=damag * derr + 4 * U * damag * dmag)


# ------------------------------------------------------------------------------------------------ mds_pw_fwd
def pw_operands(be, dt, M, K, N, pmode, rpg, seed):
    code, tdt = DT[dt]
    g = gen(seed)
    x = torch.randn(M, K, generator=g).to(tdt)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(tdt)
    r = torch.randn(M, N, generator=g).to(tdt)
    scale = 1.0 + 0.2 * torch.randn(K, generator=g); shift = 0.3 * torch.randn(K, generator=g)
    gate = torch.rand(cdiv(M, rpg), K, generator=g)
    return g, x, w, r, scale, shift, gate


def pw_pro_reference(x, pmode, scale, shift, gate, rpg, tdt):
    """float64 prologue of mds_pro_t, rounded to the storage type as the kernel rounds what it stages"""
    a = x.to(F64)
    grp = torch.arange(x.shape[0]) // rpg
    if pmode in (cabi.MDS_PRO_AFFINE, cabi.MDS_PRO_BN_SILU, cabi.MDS_PRO_BN_SILU_GATE):
        a = a * scale.to(F64) + shift.to(F64)
    if pmode in (cabi.MDS_PRO_BN_SILU, cabi.MDS_PRO_BN_SILU_GATE):
        a = F.silu(a)
    if pmode in (cabi.MDS_PRO_BN_SILU_GATE, cabi.MDS_PRO_GATE):
        a = a * gate.to(F64)[grp]
    return q(a, tdt) if tdt == torch.bfloat16 else a


# (M, N, MDS_KNOB_PW_GY): 1001..1100 rows are above the 1000-row bar of MDS_KNOB_PW_BM64 = 1, i.e. 8 or 9 row tiles of 128 with
# a ragged last one; N = 128 / 144 / 272: one, two (128 + 16) and three (128 + 128 + 16) n-tiles; block target 1: grid.y = 1, one
# block walks every n-tile; 18: grid.y = 2 of 3, the blocks of a row walk two n-tiles and one
PW_GEO = [(1001, 128, 0), (1037, 144, 0), (1037, 144, 1), (1100, 272, 1), (1061, 272, 18)]
PW_K = 72      # a K tail in both types: 64 + 8 (bf16 chunks of 64), 2 * 32 + 8 (fp32 chunks of 32)


def pw_knobs(gy):
    kn = {cabi.MDS_KNOB_PW_BM64: 1}
    if gy:
        kn[cabi.MDS_KNOB_PW_GY] = gy
    return kn


def assert_pw_geometry(be, M, N, gy):
    ls = be.launches("pw_fwd_kernel")
    if ls is None:
        return
    assert len(ls) == 1 and "2, 128" in ls[0].kernel, ls
    assert ls[0].gx == cdiv(M, 128), ls
    if gy:
        assert ls[0].gy < cdiv(N, 128), ls
    else:
        assert ls[0].gy == cdiv(N, 128), ls


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("pmode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("res,stats", [(False, False), (True, True)])
@pytest.mark.parametrize("M,N,gy", PW_GEO)
def test_pw_fwd_large_tiles(be, dt, M, N, gy, pmode, res, stats):
    """pw_fwd_kernel<T, PRO, 2, 128, 0>: the 128-row tiles that N > 64 takes above bar64 rows (MDS_KNOB_PW_BM64), every
    prologue, residual + statistics, and the loop in which a block walks several n-tiles (gy < nt, MDS_KNOB_PW_GY): the filter
    is re-staged and the statistics slot picked again per n-tile"""
    code, tdt = DT[dt]
    K, rpg = PW_K, 50
    g, x, w, r, scale, shift, gate = pw_operands(be, dt, M, K, N, pmode, rpg, M * 7 + N + pmode)
    y = be.out((M, N), tdt, float("nan"))
    st = be.out((SLOTS, 2, N), F64, 0)
    with knobs(be, pw_knobs(gy)):
        be.call("pw_fwd", cabi.make("mds_pw_fwd_args", dtype=code, M=M, K=K, N=N, x=be.t(x), w=be.t(w), y=y,
                                    pro=cabi.pro(pmode, be.t(scale), be.t(shift), be.t(gate), rpg),
                                    residual=be.t(r) if res else None, stats=st if stats else None))
        be.sync()
        assert_pw_geometry(be, M, N, gy)
    ref = pw_pro_reference(x, pmode, scale, shift, gate, rpg, tdt) @ w.to(F64).t()
    if res:
        ref = ref + r.to(F64)
    assert_close(y, ref, dt, msg="y")
    if stats:      # (the statistics are those of the fp32 accumulators + residual, before the store: as tests/test_k_pw.py)
        a, aerr = test_k_pw._pro64(x, pmode, scale, shift, gate, rpg, dt)
        v = a @ w.to(F64).t() + r.to(F64)
        vabs = a.abs() @ w.to(F64).abs().t() + r.to(F64).abs()
        test_k_pw._check_stats(st, v, vabs, aerr @ w.to(F64).abs().t() if pmode else None, K + 1, M, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("gmode,res,post", [(0, False, 1), (3, True, 2), (0, True, 3), (3, False, 3)])
@pytest.mark.parametrize("M,N,gy", PW_GEO[2:])
def test_pw_fwd_large_tiles_data_gradient(be, dt, M, N, gy, gmode, res, post):
    """pw_fwd_kernel<T, MDS_PRO_NONE, 2, 128, 1>: the data-gradient form with the next BatchNorm's backward sums in the epilogue
    (mds_poststat_t: PLAIN / MASK / SILU) at 128-row tiles, several n-tiles per block - post.y fragments, the bn table and the
    statistics slot are picked per n-tile.  The operand is the materialised dy of a BatchNorm backward (PLAIN / MASK source)."""
    code, tdt = DT[dt]
    C, rpg = PW_K, 37
    groups = cdiv(M, rpg)
    grp = torch.arange(M) // rpg
    g_ = gen(M + 13 * N + post)
    u = torch.randn(M, C, generator=g_).to(tdt)
    yb = (1.5 * torch.randn(M, C, generator=g_) + 0.3).to(tdt)
    gamma = 1 + 0.2 * torch.randn(C, generator=g_); beta = 0.1 * torch.randn(C, generator=g_)
    mask = (torch.rand(groups, generator=g_) < 0.7).float() / 0.7
    w = (torch.randn(N, C, generator=g_) / C ** 0.5).to(tdt)
    r = torch.randn(M, N, generator=g_).to(tdt)
    dy_ref, _, _ = bn_bwd_reference(yb, u, gamma, beta, gmode, None, None, mask, rpg, 1e-5)
    dy = dy_ref.to(tdt)
    ys = (torch.randn(M, N, generator=g_) * 1.2 - 0.2).to(tdt)
    gamma2 = 1 + 0.2 * torch.randn(N, generator=g_); beta2 = 0.1 * torch.randn(N, generator=g_)
    mask2 = (torch.rand(groups, generator=g_) < 0.6).float() / 0.6
    bn2 = bn_forward_table(be, ys, gamma2, beta2, 1e-5)
    st2 = be.out((SLOTS, 2, N), F64, 0)
    out = be.out((M, N), tdt, float("nan"))
    with knobs(be, pw_knobs(gy)):
        be.call("pw_fwd", cabi.make("mds_pw_fwd_args", dtype=code, M=M, K=C, N=N, x=be.t(dy), w=be.t(w), y=out, pro=cabi.pro(0),
                                    residual=be.t(r) if res else None, stats=None,
                                    post=cabi.poststat(post, be.t(ys), bn2, st2, be.t(mask2), rpg)))
        be.sync()
        assert_pw_geometry(be, M, N, gy)
    v = dy.to(F64) @ w.to(F64).t() + (r.to(F64) if res else 0.0)
    b2 = bn2.cpu().to(F64)
    stored = v * silu_grad(ys.to(F64) * b2[0] + b2[1]) if post == cabi.MDS_POST_SILU else v
    assert_close(out, stored, dt, scale=2, msg="out")
    gq = out.cpu().to(F64) * (mask2.to(F64)[grp, None] if post == cabi.MDS_POST_MASK else 1.0)   # the sums are defined on what was stored
    test_k_pw._check_post(st2, gq, ys, b2, M, C)


def pw_epi_reference(x, w, r, pmode, scale, shift, gate, rpg, esc, esh, emode, tdt):
    ref = pw_pro_reference(x, pmode, scale, shift, gate, rpg, tdt) @ w.to(F64).t()
    if emode:
        ref = ref * esc.to(F64) + esh.to(F64)
    if emode == cabi.MDS_EPI_BN_SILU:
        ref = F.silu(ref)
    return ref + r.to(F64) if r is not None else ref


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("pmode,emode,res", [(0, 2, False), (4, 1, True), (2, 2, False)])
@pytest.mark.parametrize("M,N,gy", PW_GEO[2:])
def test_pw_fwd_large_tiles_output_transform(be, dt, M, N, gy, pmode, emode, res):
    """pw_fwd_kernel<T, PRO, 2, 128, 2>: the output transform (mds_epi_t) at 128-row tiles with several n-tiles per block - the
    transform's scale / shift table is re-read per n-tile"""
    code, tdt = DT[dt]
    K, rpg = PW_K, 97
    g, x, w, r, scale, shift, gate = pw_operands(be, dt, M, K, N, pmode, rpg, M + N + emode)
    esc = 1.0 + 0.3 * torch.randn(N, generator=g); esh = 0.5 * torch.randn(N, generator=g)
    y = be.out((M, N), tdt, float("nan"))
    with knobs(be, pw_knobs(gy)):
        be.call("pw_fwd", cabi.make("mds_pw_fwd_args", dtype=code, M=M, K=K, N=N, x=be.t(x), w=be.t(w), y=y,
                                    pro=cabi.pro(pmode, be.t(scale), be.t(shift), be.t(gate), rpg), residual=be.t(r) if res else None,
                                    stats=None, epi=cabi.make("mds_epi_t", mode=emode, scale=be.t(esc), shift=be.t(esh))))
        be.sync()
        assert_pw_geometry(be, M, N, gy)
    assert_close(y, pw_epi_reference(x, w, r if res else None, pmode, scale, shift, gate, rpg, esc, esh, emode, tdt), dt, msg="y")


@pytest.mark.parametrize("pmode", [0, 4])
def test_pw_fwd_one_or_two_chunks_in_flight(be, pmode):
    """the fp32 inference launches keep two K chunks in flight (DEEP: output transform, 64-row tiles, >= 3 chunks, at most 256
    blocks) unless MDS_KNOB_PW_DEEP = 1: pw_fwd_kernel<float, PRO, 2, 64, 2, false, true> against <float, PRO, 2, 64, 2>, both
    against float64; 10 chunks + a K tail, ragged last row tile, two n-tiles"""
    dt = "f32"
    code, tdt = DT[dt]
    M, K, N, rpg, emode = 140, 328, 144, 97, 2
    g, x, w, r, scale, shift, gate = pw_operands(be, dt, M, K, N, pmode, rpg, 17 + pmode)
    esc = 1.0 + 0.3 * torch.randn(N, generator=g); esh = 0.5 * torch.randn(N, generator=g)
    ref = pw_epi_reference(x, w, None, pmode, scale, shift, gate, rpg, esc, esh, emode, tdt)
    names = []
    for deep_off in (0, 1):
        y = be.out((M, N), torch.float32, float("nan"))
        with knobs(be, {cabi.MDS_KNOB_PW_DEEP: deep_off}):
            be.call("pw_fwd", cabi.make("mds_pw_fwd_args", dtype=code, M=M, K=K, N=N, x=be.t(x), w=be.t(w), y=y,
                                        pro=cabi.pro(pmode, be.t(scale), be.t(shift), be.t(gate), rpg), residual=None, stats=None,
                                        epi=cabi.make("mds_epi_t", mode=emode, scale=be.t(esc), shift=be.t(esh))))
            be.sync()
            ls = be.launches("pw_fwd_kernel")
            if ls is not None:
                assert len(ls) == 1, ls
                names.append(ls[0].kernel)
        assert_close(y, ref, dt, msg=f"y (MDS_KNOB_PW_DEEP = {deep_off})")
    if names:
        assert "false, sizeof(T) == 4" in names[0] and "false, sizeof(T) == 4" not in names[1], names


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("knob", [6, 2])
def test_pw_fwd_split_rule_with_a_forced_factor(be, dt, knob):
    """mds_pw_fwd_split under MDS_KNOB_PW_SPLIT = n >= 2: 'that factor instead of 4', still only for < 100 tiles that walk >= 16
    chunks, capped at chunks / 3 and MDS_PW_MAX_SPLIT; 1 = never.  The launch at the factor it returns matches float64, twice
    bit for bit, and leaves its tickets at zero."""
    code, tdt = DT[dt]
    f = be.lib.fn["pw_fwd_split"]
    M, K, N, rpg, pmode, emode = 200, 1160, 144, 97, 4, 1
    kc = 64 if dt == "bf16" else 32
    chunks = cdiv(K, kc)
    with knobs(be, {cabi.MDS_KNOB_PW_SPLIT: knob}):
        split = f(M, K, N, code)
        assert split == min(knob, chunks // 3, cabi.MDS_PW_MAX_SPLIT) and split != 4
        assert f(M, 15 * kc, N, code) == 1 and f(64 * 100, K, N, code) == 1          # < 16 chunks; 100 tiles
        assert f(M, 18 * kc, N, code) == min(knob, 6)                                # chunks / 3 caps the factor
        g, x, w, r, scale, shift, gate = pw_operands(be, dt, M, K, N, pmode, rpg, 23 + knob)
        esc = 1.0 + 0.3 * torch.randn(N, generator=g); esh = 0.5 * torch.randn(N, generator=g)
        part = be.out((split * M * N,), torch.float32, float("nan"))
        tiles = cdiv(M, cabi.MDS_PW_SPLIT_TILE_ROWS) * cdiv(N, 128)
        ticket = be.out(tiles * cabi.MDS_PW_SPLIT_TICKET_STRIDE, torch.int32, 0)
        outs = []
        for _ in range(2):
            y = be.out((M, N), tdt, float("nan"))
            be.call("pw_fwd", cabi.make("mds_pw_fwd_args", dtype=code, M=M, K=K, N=N, x=be.t(x), w=be.t(w), y=y,
                                        pro=cabi.pro(pmode, be.t(scale), be.t(shift), be.t(gate), rpg), residual=be.t(r), stats=None,
                                        epi=cabi.make("mds_epi_t", mode=emode, scale=be.t(esc), shift=be.t(esh)),
                                        split=split, split_part=part, split_ticket=ticket))
            be.sync()
            outs.append(y.float().cpu())
            assert int(ticket.abs().sum()) == 0, "tickets must reset themselves"
        ls = be.launches("pw_fwd_kernel")
        assert ls is None or all(l.gz == split for l in ls), ls
    with knobs(be, {cabi.MDS_KNOB_PW_SPLIT: 1}):
        assert f(M, K, N, code) == 1
    assert f(M, K, N, code) == min(4, chunks // 3)
    assert_close(outs[0], pw_epi_reference(x, w, r, pmode, scale, shift, gate, rpg, esc, esh, emode, tdt), dt, msg="y (split)")
    assert torch.equal(outs[0], outs[1]), "two split launches must agree bit for bit"


# ------------------------------------------------------------------------------------------------ mds_pw_wgrad
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("M", [900, 5000])
@pytest.mark.parametrize("budget", [1, 4096])
def test_pw_wgrad_block_budget(be, dt, budget, M, det):
    """pw_wgrad_geo under MDS_KNOB_WG_BLOCKS: budget 1 - ONE fp32 block walks every row of M = 900 (bf16: the minimum of 8 row
    splits); budget 4096 - 256-row splits, the floor of the rule, with a ragged last one (900 = 3 * 256 + 132, 5000 = 19 * 256 + 136).
    With a partial buffer (mds_partial_t): mds_pw_wgrad_partial_floats under the knob is exactly what the launch accepts, and two
    launches agree bit for bit.  2 x 2 output tiles with ragged edges (N = 144, K = 72), BN + SiLU + gate prologue."""
    import ctypes
    code, tdt = DT[dt]
    K, N, rpg, pmode = 72, 144, 97, cabi.MDS_PRO_BN_SILU_GATE
    g, x, w, r, scale, shift, gate = pw_operands(be, dt, M, K, N, pmode, rpg, M * 3 + budget)
    dy = r                                           # [M][N], rounded to the storage type
    ref = dy.to(F64).t() @ pw_pro_reference(x, pmode, scale, shift, gate, rpg, tdt)
    outs = []
    with knobs(be, {cabi.MDS_KNOB_WG_BLOCKS: budget}):
        for run in range(2 if det else 1):
            dw = be.out((N, K), torch.float32, 0)
            args = cabi.make("mds_pw_wgrad_args", dtype=code, M=M, K=K, N=N, x=be.t(x), dy=be.t(dy), dw=dw,
                             pro=cabi.pro(pmode, be.t(scale), be.t(shift), be.t(gate), rpg))
            need = int(be.lib.fn["pw_wgrad_partial_floats"](ctypes.byref(args)))
            assert need > 0 and need % (N * K) == 0
            splits = need // (N * K)
            if det:
                part = be.out((need,), torch.float32, float("nan"))
                args.partial = cabi.make("mds_partial_t", buf=part, floats=need - 1)
                with pytest.raises(cabi.MdsError):
                    be.call("pw_wgrad", args)
                args.partial = cabi.make("mds_partial_t", buf=part, floats=need)
            be.call("pw_wgrad", args)
            be.sync()
            outs.append(dw.cpu())
        ls = be.launches("pw_wgrad")
        if ls is not None:
            ls = [l for l in ls if "finish" not in l.kernel]
            tiles = cdiv(N, 128) * cdiv(K, 64)
            for l in ls:      # fp32: grid = (row splits, tiles); bf16: row splits rounded up to 8, times the tiles, in grid.x
                assert (l.gx, l.gy) == ((splits, tiles) if dt == "f32" else (cdiv(splits, 8) * 8 * tiles, 1)), (l, splits)
            if budget == 1:
                assert splits == {("f32", 900): 1, ("f32", 5000): 2, ("bf16", 900): 4, ("bf16", 5000): 8}[(dt, M)]
            else:
                assert splits == cdiv(M, 256) and M % 256 != 0
        if budget == 4096:      # at these M the default budget ends at the same 256-row floor; where it does not, the knob must show
            big = cabi.make("mds_pw_wgrad_args", dtype=code, M=100000, K=K, N=N, pro=cabi.pro(0))
            assert int(be.lib.fn["pw_wgrad_partial_floats"](ctypes.byref(big))) // (N * K) == cdiv(100000, 256)
    a, aerr = test_k_pw._pro64(x, pmode, scale, shift, gate, rpg, dt)
    d64 = dy.to(F64)
    r_, t_ = M % 256, M // 8       # (an eighth of the rows: 16 rows are below the bound's resolution at M = 5000)
    probes = [(f"last {r_} rows (the ragged split) left out", d64[:-r_].t() @ a[:-r_]), (f"first {t_} rows counted twice", d64.t() @ a + d64[:t_].t() @ a[:t_])]
    assert_sum_close(outs[0], d64.t() @ a, [(M, d64.abs().t() @ a.abs()), (ABS, d64.abs().t() @ aerr)], "dw", probes, cap=(dt, M ** 0.5))
    if det:
        assert torch.equal(outs[0], outs[1]), "two launches with a partial buffer must agree bit for bit"


# ------------------------------------------------------------------------------------------------ depthwise
DW_PATHS = [  # dtype, then N, T, H, W, C, stride, kt: one case of each path of tests/test_k_dw_stem.py::DW_CASES whose strip-block
    # count differs from its channel-chunk count in at least one launch (else the two grid orders have the same dim3)
    ("f32", 1, 1, 14, 37, 72, 1, 1), ("bf16", 1, 1, 14, 37, 72, 1, 1),      # 2D stride 1: several bands / segments, half-filled channel chunk
    ("f32", 1, 1, 11, 38, 72, 2, 1), ("bf16", 1, 1, 11, 38, 72, 2, 1),      # 2D stride 2, mixed padding (pad_t 1, pad_l 0), several segments
    ("f32", 1, 5, 6, 9, 576, 1, 3), ("bf16", 1, 5, 6, 9, 576, 1, 3),        # T = 5: the 3x3x3 sliding-window kernels, nine channel chunks
    ("bf16", 2, 11, 6, 13, 72, 1, 3),      # T = 11: time chunks (the bf16 forward; every other T = 11 launch is a tiled kernel with a grid of its own)
]
assert all(c[1:] in test_k_dw_stem.DW_CASES for c in DW_PATHS)


@pytest.mark.parametrize("dt,N,T,H,W,C,stride,kt", DW_PATHS)
@pytest.mark.parametrize("order", [1, 2])
def test_dw_grid_orders(be, dt, order, N, T, H, W, C, stride, kt):
    """dw_grid / dw_block under MDS_KNOB_DW_ORDER: 1 = channel chunk fastest (dim3(nchunks, strip blocks), the kernels swap
    blockIdx back), 2 = strip fastest without the XCD-aware remap of the default; forward, backward with atomics, and backward
    with a partial buffer (slot = strip block, whatever the order) through DetBackend's comparison of the two forms.  Order 1
    shows in the launch record; order 2 has the default's dim3 and differs from it only in dw_block's decoding inside the
    kernels, so for it the record can only say that the strip kernels ran.  (dw_grid's fall-back from order 1 to 2 needs 65536
    strip blocks in grid.y: out of reach of a quick test.)"""
    from test_deterministic_kernels import DetBackend
    with knobs(be, {cabi.MDS_KNOB_DW_ORDER: order}):
        test_k_dw_stem._dw_fwd_bwd(DetBackend(be), dt, N, T, H, W, C, stride, kt)
        ls = be.launches()
        if ls is not None:
            ls = [l for l in ls if re.search(r"dw2s?_|dw3g?_", l.kernel)]       # the launches that go through dw_grid
            assert ls, "no strip kernel was launched"
            nchunks = cdiv(C, 64)
            if order == 1:
                assert all(l.gx == nchunks and l.gz == 1 for l in ls) and any(l.gy != nchunks for l in ls), ls
            else:
                assert all(l.gy == nchunks and l.gz == 1 for l in ls), ls


@pytest.mark.parametrize("N,T,H,W,C,stride,kt", [(2, 3, 5, 7, 24, 1, 3), (2, 11, 6, 13, 72, 1, 3), test_k_dw_stem.DW_TILED_WIDE])
def test_dw3_tiled_forward_bf16(be, N, T, H, W, C, stride, kt):
    """dw_fwd_kernel<bf16_t>: the LDS-tiled 3x3x3 forward, which bf16 launches at T != 5 take only with MDS_KNOB_DW3G = 1
    (by default they take the time-chunked sliding window dw3g_fwd_kernel).  The last case has three tiles along W: three
    forward blocks, and two blocks of the tiled backward dw_bwd_kernel, which walks two tiles per block (the second block's walk
    ends after one)"""
    with knobs(be, {cabi.MDS_KNOB_DW3G: 1}):
        test_k_dw_stem._dw_fwd_bwd(be, "bf16", N, T, H, W, C, stride, kt, act_rounded=True)
        ls = be.launches("_fwd_kernel")
        assert ls is None or (len(ls) == 1 and "dw_fwd_kernel" in ls[0].kernel and "dw3g" not in ls[0].kernel), ls
        lb = be.launches("dw_bwd_kernel")
        if ls is not None and W == 37:
            assert ls[0].gx == 3 and len(lb) == 1 and lb[0].gx == 2, (ls, lb)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dw2_strip_count_rule(be, dt):
    """dw2_len under MDS_KNOB_DW2_BLOCKS: a block target of 1 keeps the longest strips (W = 37: 19 + 18 columns), a large one
    the shortest the rule allows (8 + 8 + 8 + 8 + 5): a ragged last segment in both, forward and backward"""
    N, T, H, W, C, stride, kt = 1, 1, 14, 37, 72, 1, 1
    blocks = {}
    for target in (1, 100000):
        with knobs(be, {cabi.MDS_KNOB_DW2_BLOCKS: target}):
            test_k_dw_stem._dw_fwd_bwd(be, dt, N, T, H, W, C, stride, kt)
            ls = be.launches("dw2_")
            if ls is not None:
                assert len(ls) == 2, ls
                blocks[target] = [l.gx for l in ls]
    if blocks:      # two-row bands forward, four-row bands backward, 8 strips per block: 2 / 5 segments per row
        assert blocks[1] == [cdiv(7 * 2, 8), cdiv(4 * 2, 8)] and blocks[100000] == [cdiv(7 * 5, 8), cdiv(4 * 5, 8)], blocks


# ------------------------------------------------------------------------------------------------ 3x3 data gradients, stem
@pytest.mark.parametrize("blocks", [1, 3])
def test_c3_data_gradient_block_count(be, blocks):
    """c3_blocks(passes, bwd = true) under MDS_KNOB_C3_BWD_BLOCKS: the data-gradient launches of k_c3.hip (stride 1: the residual
    form without statistics; stride 2: the tap-group form) with 1 and 3 persistent blocks that walk several items each"""
    with knobs(be, {cabi.MDS_KNOB_C3_BWD_BLOCKS: blocks}):
        N, H, W, Cin, Cout, res, stats, cap = test_k_conv.C3_CASES[3]
        assert res and not stats
        test_k_conv.test_c3_filter_in_registers(be, N, H, W, Cin, Cout, res, stats, 0)      # (0: MDS_KNOB_CONV_BLOCKS stays off)
        N, H, W, Cin, Cout, cap = test_k_conv.C3T_CASES[3]
        test_k_conv.test_c3t_stride2_data_gradient(be, N, H, W, Cin, Cout, 0)
        ls = be.launches("c3")
        if ls is not None:
            assert len(ls) == 2 and all(l.gx == blocks for l in ls), ls


@pytest.mark.parametrize("N,H,W", [(2, 20, 36), (1, 17, 23), (3, 6, 70), (2, 40, 150)])
def test_stem_fwd_gather_kernel_bf16(be, N, H, W):
    """stem_fwd_kernel<bf16_t> without an output transform: the training forward takes the LDS-tiled kernel (stem_fwd_tiled)
    unless MDS_KNOB_STEM_FWD = 1; the gather kernel's raw bf16 output and its statistics, at the shapes of test_stem_fwd_wgrad"""
    with knobs(be, {cabi.MDS_KNOB_STEM_FWD: 1}):
        test_k_dw_stem.test_stem_fwd_wgrad(be, "bf16", N, H, W)
        ls = be.launches("stem_fwd")
        assert ls is None or (len(ls) == 1 and ls[0].kernel.startswith("stem_fwd_kernel")), ls


# ------------------------------------------------------------------------------------------------ knob coverage
KNOBS_WITHOUT_A_TEST = {
    # name: why no test names it
}


def test_every_knob_is_named_by_a_test_or_a_reason():
    """a new MDS_KNOB_* arrives with a test that sets it, or with a reason here (the expected one: measurement only, changes no
    result)"""
    names = sorted(k for k in cabi.DEFINES if k.startswith("MDS_KNOB_") and k != "MDS_KNOB_COUNT")
    assert len(names) >= 20
    here = os.path.dirname(os.path.abspath(__file__))
    text = "".join(open(f).read() for f in glob.glob(os.path.join(here, "**", "*.py"), recursive=True))
    unnamed = [k for k in names if not re.search(r"\b%s\b" % k, text) and k not in KNOBS_WITHOUT_A_TEST]
    assert not unnamed, f"no file under tests/ names {unnamed}: add a test that sets it, or a reason to KNOBS_WITHOUT_A_TEST"
    stale = [k for k in KNOBS_WITHOUT_A_TEST if k not in names]
    assert not stale, f"{stale}: not a knob of include/mds.h"
