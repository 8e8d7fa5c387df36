"""Row-streaming and latency-class kernels against torch fp32 references (autograd for bwd)."""
import pytest
import torch
import torch.nn.functional as F

from backends import be, DT, ABS, U, assert_close, assert_sum_close, assert_post_close, pro_operand  # noqa: F401
from mds import cabi

SLOTS = cabi.MDS_STAT_SLOTS


def gen(s):
    return torch.Generator().manual_seed(s)


def bn_finalize(be, stats, count, gamma, beta, eps=1e-3, momentum=0.1, training=1, rm=None, rv=None, nbt=None):
    C = gamma.numel()
    out = be.out((4, C), torch.float32, float("nan"))
    be.call("bn_finalize", cabi.make("mds_bn_finalize_args", C=C, count=count, stats=stats, gamma=gamma,
                                     beta=beta, eps=eps, momentum=momentum, training=training,
                                     running_mean=rm, running_var=rv, num_batches_tracked=nbt, out=out))
    return out


F64 = torch.float64


def silu_grad64(z, zmag):
    """(silu'(z), silu'(z) on magnitudes, bound of the error of the kernels' fp32 evaluation): s (1 + z (1 - s)) through v_exp / v_rcp
    is (|z| + 12) U of its magnitude off (the reasoning of backends.pro_operand), and z's own rounding U * zmag moves it by at most
    |silu''| <= 1/2 times that (z: two roundings on fp32-rounded tables, 2 U * zmag)"""
    s = torch.sigmoid(z)
    mag = s * (1 + z.abs() * (1 - s))
    return s * (1 + z * (1 - s)), mag, U * ((z.abs() + 12) * mag + zmag)


def check_bn_bwd_sums(dgamma, dbeta, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, dt, running=None):
    """dbeta = sum g and dgamma = sum g * xhat of mds_bn_bwd_reduce / _finalize against their float64 values on the stored y and u,
    g formed as mds_gsrc_t says; bound: the fp32 sum over M rows + the error of g where the kernel computes a SiLU factor.
    xhat comes from the float64 mean / rstd of y, which the kernels' fp32 table rounds (see backends.assert_post_close).
    Probes at the row loops' seams: the last rows (a ragged last trip) left out / taken twice, in a DropPath group that is kept."""
    M, C = y.shape
    y64, u64, grp = y.to(F64), u.to(F64), torch.arange(M) // rpg
    if running is None:
        mean, var = y64.mean(0), y64.var(0, unbiased=False)
    else:
        mean, var = running[0].to(F64), running[1].to(F64)
    rstd = 1 / torch.sqrt(var + eps)
    sc = gamma.to(F64) * rstd
    sh = beta.to(F64) - mean * sc
    z, zmag = y64 * sc + sh, (y64 * sc).abs() + sh.abs()
    src, smag = u64, u64.abs()
    if mode == cabi.MDS_G_SE_SILU:
        src, smag = u64 * gate.to(F64)[grp] + dpool.to(F64)[grp], (u64 * gate.to(F64)[grp]).abs() + dpool.to(F64)[grp].abs()
    if mode == cabi.MDS_G_MASK:
        src, smag = u64 * mask.to(F64)[grp, None], smag * mask.to(F64)[grp, None].abs()
    gerr = None
    if mode in (cabi.MDS_G_SILU, cabi.MDS_G_SE_SILU):
        d, dmag, derr = silu_grad64(z, zmag)
        src, gerr = src * d, smag * derr + 2 * U * smag * dmag
    xhat, xmag = (y64 - mean) * rstd, (y64.abs() + mean.abs()) * rstd
    r, end = M % 32 + 16, M
    if mode == cabi.MDS_G_MASK:     # the rows up to the end of the last group DropPath keeps
        end = min(M, (int(mask.nonzero().max()) + 1) * rpg)
    keep = torch.cat([torch.arange(end - r), torch.arange(end, M)])
    probes = [(f"rows {end - r}..{end - 1} left out", lambda t: t[keep]), (f"rows {end - r}..{end - 1} counted twice", lambda t: torch.cat([t, t[end - r:end]], 0))]
    assert_post_close(torch.stack([dbeta.detach().double().cpu(), dgamma.detach().double().cpu()]), src, xhat, xmag, (dt, 20),
                      probes if M <= 3000 else (), "dbeta / dgamma: ", gerr)


def se_backward64(dgate, gate, hidden, pooled, w1, w2, drop_c=0):
    """the parameter gradients of mds_se_fc_bwd in float64 from ITS operands - the dgate, gate, hidden and pooled buffers the
    launches before it left - with their a-priori bounds: {name: (want, parts)}.  dpre = dgate * gate (1 - gate);
    db2 = sum_g dpre, dw2 = sum_g dpre (x) silu(hidden); dh = dpre W2 (a sum over the C channels), dhid = dh * silu'(hidden);
    db1 = sum_g dhid, dw1 = sum_g dhid (x) pooled.  silu / silu' through v_exp / v_rcp: 12 U of their magnitude (the reasoning of
    backends.pro_operand); the sum over C is inherited by dw1 / db1 as an absolute part.  drop_c: a probe - the last drop_c
    channels left out of the sum over C.  The chains, none of them fitted:
      db2: G additions; a term dgate * gate * (1 - gate) is 1 - gate, two products and the fp64 -> fp32 conversion of dgate: 4
      roundings more than the helper's + 8 allows for one product, hence G + 4;
      dw2: the same term times silu(hidden): 12 more for silu through v_exp / v_rcp and 4 as above, hence G + 16;
      dhid: C additions for dh, + 8 for the term dpre * w2 (as db2's, itself 4 + the product: within 8), + 16 for
      silu'(hidden) = s (1 + hid (1 - s)): 12 for the sigmoid as in pro_operand and 4 roundings of the polynomial, hence C + 8 + 16."""
    G, C = gate.shape
    dg, gt, hid, pl, W1, W2 = (t.detach().to(F64).cpu() for t in (dgate, gate, hidden, pooled, w1, w2))
    s = torch.sigmoid(hid)
    h, dh_ = hid * s, s * (1 + hid * (1 - s))
    dh_m = s * (1 + hid.abs() * (1 - s))
    dpre = dg * gt * (1 - gt)
    keep = C - drop_c
    dh, dhm = dpre[:, :keep] @ W2[:keep], dpre[:, :keep].abs() @ W2[:keep].abs()
    dhid, dhid_m = dh * dh_, dhm * dh_m
    dhid_e = (C + 8 + 16) * U * dhid_m
    return {"db2": (dpre.sum(0), [(G + 4, dpre.abs().sum(0))]),
            "dw2": (dpre.t() @ h, [(G + 16, dpre.abs().t() @ h.abs())]),
            "db1": (dhid.sum(0), [(G, dhid_m.sum(0)), (ABS, dhid_e.sum(0))]),
            "dw1": (dhid.t() @ pl, [(G, dhid_m.t() @ pl.abs()), (ABS, dhid_e.t() @ pl.abs())])}


def check_se_backward(got, bufs, y, scale, shift, w1, w2, u, G, R_, dt):
    """got: {name: kernel output}: dgate [G][C] = the sum over a group's R_ rows of u * a, a = silu(y * scale + shift) held in
    fp32, and the four parameter gradients (se_backward64 on bufs = the kernels' own dgate, gate, hidden, pooled).
    Probes: the last group left out; the first group taken twice (dw2 / db2); the last 8 channels left out of the sum over C
    (dw1 / db1); for dgate the last 6 rows of every group left out"""
    C = w1.shape[1]
    y64, sc, sh = y.to(F64), scale.to(F64), shift.to(F64)
    a, aerr = pro_operand(y64 * sc + sh, (y64 * sc).abs() + sh.abs(), True, "f32")
    ua, ue = (u.to(F64) * a).view(G, R_, C), (u.to(F64).abs() * aerr).view(G, R_, C)
    cutg = ua.clone(); cutg[-1] = 0
    assert_sum_close(got["dgate"], ua.sum(1), [(R_, ua.abs().sum(1)), (ABS, ue.sum(1))], "dgate",
                     [("last group left out", cutg.sum(1)), ("last 6 rows of every group left out", ua[:, :-6].sum(1))], cap=(dt, R_ ** 0.5))
    ref = se_backward64(w1=w1, w2=w2, **bufs)
    zero_last = dict(bufs, dgate=torch.cat([bufs["dgate"][:-1], torch.zeros_like(bufs["dgate"][-1:])]))
    twice = {k: torch.cat([v, v[:1]]) for k, v in bufs.items()}
    wrong = {"last group left out": se_backward64(w1=w1, w2=w2, **zero_last), "first group counted twice": se_backward64(w1=w1, w2=w2, **twice),
             "last 8 channels left out of the sum over C": se_backward64(w1=w1, w2=w2, drop_c=8, **bufs)}
    for name in ("dw1", "db1", "dw2", "db2"):
        want, parts = ref[name]
        names = ["last group left out", "first group counted twice" if name in ("dw2", "db2") else "last 8 channels left out of the sum over C"]
        assert_sum_close(got[name], want, parts, name, [(n, wrong[n][name][0]) for n in names], cap=(dt, 10))


def gem_dp64(y, scale, shift, pro_mode, p, dpo, G, R_, eps):
    """GeM's dp = d/dp sum(dpooled * pooled), pooled = (mean_r x^p)^(1/p), x = max(a, eps), in float64: per (group, channel)
    dpooled * pooled * [T / (p S) - ln(S / R) / p^2] with S = sum_r x^p, T = sum_r x^p ln x.  -> (want [1], parts).
    Bound: the fp32 chain over R_ rows and over the G * C terms, the power x^p = exp2(p log2 x) (v_log / v_exp: 1 ulp each, the
    rounded exponent moves it by p |ln x| U), p times the activation's own error ((|z| + 4) U, backends.pro_operand), + 32 =
    four more transcendental evaluations at 8 U each (log2 and exp2 of a term's power: 1 ulp + argument and result roundings;
    the root (S / R)^(1 / p), again a log2 / exp2 pair; ln(S / R)); on magnitudes: |ln x| for ln x, and |ln(S / R)| + 1 because S's relative error is an
    ABSOLUTE error of its logarithm."""
    C, y = y.shape[1], y.detach()
    z = y.to(F64) * scale.to(F64) + shift.to(F64) if pro_mode else y.to(F64)
    a = z * torch.sigmoid(z) if pro_mode else z
    x = a.clamp(min=eps).view(G, R_, C)
    pw, lx = x.pow(p), x.log()
    S, T, Tm = pw.sum(1), (pw * lx).sum(1), (pw * lx.abs()).sum(1)
    pooled = (S / R_).pow(1 / p)
    d64 = dpo.to(F64)
    want = (d64 * pooled * (T / (p * S) - (S / R_).log() / p ** 2)).sum().view(1)
    mag = (d64.abs() * pooled * (Tm / (p * S) + ((S / R_).log().abs() + 1) / p ** 2)).sum().view(1)
    chain = R_ + G * C + p * (float(lx.abs().max()) + (float(z.abs().max()) + 4 if pro_mode else 0)) + 32
    return want, [(chain, mag)]


def check_gem_dp(dp, y, scale, shift, pro_mode, p, dpo, G, R_, eps, dt):
    """probes: the last group left out; the last eighth of every group's rows left out"""
    want, parts = gem_dp64(y, scale, shift, pro_mode, p, dpo, G, R_, eps)
    cut = dpo.clone(); cut[-1] = 0
    k = max(1, R_ // 8)
    rows = y.view(G, R_, -1)[:, :-k].reshape(G * (R_ - k), -1)
    probes = [("last group left out", gem_dp64(y, scale, shift, pro_mode, p, cut, G, R_, eps)[0]),
              (f"last {k} rows of every group left out", gem_dp64(rows, scale, shift, pro_mode, p, dpo, G, R_ - k, eps)[0])]
    assert_sum_close(dp, want, parts, "dp", probes, cap=(dt, 5))


def test_bn_finalize_train_and_eval(be):
    C, M = 24, 1000
    y = torch.randn(M, C, generator=gen(0)) * 2 + 0.5
    stats = torch.zeros(SLOTS, 2, C, dtype=torch.float64)
    stats[3, 0] = y[:400].sum(0); stats[3, 1] = (y[:400] ** 2).sum(0)
    stats[17, 0] = y[400:].sum(0); stats[17, 1] = (y[400:] ** 2).sum(0)
    gamma = 1 + 0.1 * torch.randn(C, generator=gen(1)); beta = 0.1 * torch.randn(C, generator=gen(2))
    rm = be.t(torch.zeros(C)); rv = be.t(torch.ones(C)); nbt = be.t(torch.zeros((), dtype=torch.long))
    out = bn_finalize(be, be.t(stats), M, be.t(gamma), be.t(beta), eps=1e-3, rm=rm, rv=rv, nbt=nbt)
    be.sync()
    bn = torch.nn.BatchNorm1d(C, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    ref = bn(y)
    z = y * out[0].cpu() + out[1].cpu()
    assert_close(z, ref, "f32", msg="train normalise")
    assert_close(rm, bn.running_mean, "f32"); assert_close(rv, bn.running_var, "f32")
    assert int(nbt.item()) == 1
    out = bn_finalize(be, None, 0, be.t(gamma), be.t(beta), eps=1e-3, training=0, rm=rm, rv=rv)
    be.sync()
    bn.eval()
    assert_close(y * out[0].cpu() + out[1].cpu(), bn(y), "f32", msg="eval normalise")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,C,act,use_mask,use_sc", [(300, 16, 0, True, True), (77, 112, 1, False, False),
                                                       (64, 1152, 0, True, True), (1000, 48, 0, False, True)])
def test_bn_res(be, dt, M, C, act, use_mask, use_sc):
    code, tdt = DT[dt]
    g = gen(M + C)
    rpg = 40
    y = torch.randn(M, C, generator=g).to(tdt); sc_ = torch.randn(M, C, generator=g).to(tdt)
    scale = 1 + 0.2 * torch.randn(C, generator=g); shift = 0.2 * torch.randn(C, generator=g)
    mask = (torch.rand((M + rpg - 1) // rpg, generator=g) > 0.3).float() / 0.7
    out = be.out((M, C), tdt, float("nan"))
    be.call("bn_res", cabi.make("mds_bn_res_args", dtype=code, M=M, C=C, y=be.t(y), scale=be.t(scale),
                                shift=be.t(shift), act=act, mask=be.t(mask, name="mask") if use_mask else None,
                                rows_per_group=rpg, shortcut=be.t(sc_) if use_sc else None, out=out))
    be.sync()
    z = y.float() * scale + shift
    if act:
        z = F.silu(z)
    if use_mask:
        z = z * mask[torch.arange(M) // rpg, None]
    if use_sc:
        z = z + sc_.float()
    assert_close(out, z, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("packed,C,RD", [(True, 48, 12), (False, 48, 12), (True, 328, 28), (True, 1152, 48),
                                         (True, 1536, 64), (True, 2048, 20)])   # > 1280 channels: two trips of the mat-vec; R = 64: 16 rows per wave
def test_se_forward_backward(be, dt, packed, C, RD):
    """se_pool + se_fc_fwd + (gated consumer) and the SE backward chain vs autograd; with and without
    the packed [R][C] copy of w2 (made by pack_weights / MDS_PACK_IO_F32)."""
    code, tdt = DT[dt]
    G, R_ = 3, 70
    M = G * R_
    g = gen(5)
    y = torch.randn(M, C, generator=g).to(tdt)
    scale = 1 + 0.2 * torch.randn(C, generator=g); shift = 0.2 * torch.randn(C, generator=g)
    w1 = torch.randn(RD, C, generator=g) * 0.3; b1 = torch.randn(RD, generator=g) * 0.1
    w2 = torch.randn(C, RD, generator=g) * 0.3; b2 = torch.randn(C, generator=g) * 0.1
    u = torch.randn(M, C, generator=g).to(tdt)          # grad wrt gated output
    # reference
    yf = y.float().requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in dict(w1=w1, b1=b1, w2=w2, b2=b2).items()}
    a = F.silu(yf * scale + shift).view(G, R_, C)
    pooled_ref = a.mean(1)
    hid = pooled_ref @ p["w1"].t() + p["b1"]
    gate_ref = torch.sigmoid(F.silu(hid) @ p["w2"].t() + p["b2"])
    out = a * gate_ref[:, None, :]
    a.retain_grad()
    (out * u.float().view(G, R_, C)).sum().backward()
    # kernels
    yd = be.t(y); ud = be.t(u); scd = be.t(scale); shd = be.t(shift)
    pooled = be.out((G, C), torch.float64, 0)      # cross-block sums that feed activations: fp64
    be.call("se_pool", cabi.make("mds_se_pool_args", dtype=code, groups=G, rows_per_group=R_, C=C, y=yd,
                                 scale=scd, shift=shd, pooled=pooled))
    hidden = be.out((G, RD), torch.float32, float("nan")); gate = be.out((G, C), torch.float32, float("nan"))
    w1d, b1d, w2d, b2d = be.t(w1), be.t(b1), be.t(w2), be.t(b2)
    w2t = None
    if packed:
        w2t = be.out((RD, C), torch.float32, float("nan"))
        job = cabi.make("mds_pack_job", src=w2d, dst=w2t, kind=cabi.MDS_PACK_IO_F32, O=C, I=RD, taps=1)
        be.call_raw("pack_weights", job, 1, C * RD, code)
        be.sync()
        assert torch.equal(w2t.cpu(), w2.t().contiguous())
    be.call("se_fc_fwd", cabi.make("mds_se_fc_fwd_args", groups=G, C=C, R=RD, pooled=pooled, w1=w1d, b1=b1d,
                                   w2=w2d, b2=b2d, hidden=hidden, gate=gate, w2t=w2t))
    dgate = be.out((G, C), torch.float64, 0)
    be.call("se_bwd_reduce", cabi.make("mds_se_bwd_reduce_args", dtype=code, groups=G, rows_per_group=R_, C=C,
                                       u=ud, y=yd, scale=scd, shift=shd, dgate=dgate))
    dpooled = be.out((G, C), torch.float32, float("nan"))
    dw1 = be.out((RD, C), torch.float32, 0); db1 = be.out(RD, torch.float32, 0)
    dw2 = be.out((C, RD), torch.float32, 0); db2 = be.out(C, torch.float32, 0)
    be.call("se_fc_bwd", cabi.make("mds_se_fc_bwd_args", groups=G, C=C, R=RD, rows_per_group=R_, dgate=dgate,
                                   gate=gate, hidden=hidden, pooled=pooled, w1=w1d, w2=w2d, dpooled=dpooled,
                                   scratch=be.out((G, RD), torch.float32, float("nan")), dw1=dw1, db1=db1, dw2=dw2, db2=db2,
                                   w2t=w2t))
    be.sync()
    assert_close(pooled, pooled_ref, dt, msg="pooled")
    assert_close(gate, gate_ref, dt, msg="gate")
    check_se_backward(dict(dgate=dgate, dw1=dw1, db1=db1, dw2=dw2, db2=db2), dict(dgate=dgate, gate=gate, hidden=hidden, pooled=pooled),
                      y, scale, shift, w1, w2, u, G, R_, dt)
    # total grad wrt a = u*gate + dpooled(broadcast): check through the BN-backward g-source
    da_ref = a.grad.view(M, C)
    da = ud.float().cpu() * gate.cpu()[torch.arange(M) // R_] + dpooled.cpu()[torch.arange(M) // R_]
    assert_close(da, da_ref, dt, scale=3, msg="da")


def test_se_parameter_gradients_table_equals_the_per_layer_launches(be):
    """mds_se_fc_bwd_params_table (a device-resident array of layers, grid.y = layer: what the planner issues once per gradient
    bucket) against one mds_se_fc_bwd_params launch per layer, on layers of different widths: bit-identical, accumulating (+=)"""
    g = gen(77)
    G = 5
    SJ = cabi.STRUCTS["mds_se_fc_bwd_args"]
    shapes = [(48, 12), (1152, 48), (328, 28)]
    jobs, outs = [], []
    for C, R in shapes:
        dgate = be.t(torch.randn(G, C, generator=g).double()); gate = be.t(torch.rand(G, C, generator=g))
        hidden = be.t(torch.randn(G, R, generator=g)); pooled = be.t(torch.randn(G, C, generator=g).double())
        scratch = be.t(torch.randn(G, R, generator=g)); w1 = be.t(torch.randn(R, C, generator=g)); w2 = be.t(torch.randn(C, R, generator=g))
        init = [torch.randn(R, C, generator=g), torch.randn(R, generator=g), torch.randn(C, R, generator=g), torch.randn(C, generator=g)]
        two = []
        for _ in range(2):
            gr = [be.out(t.shape, torch.float32, t, name=n) for t, n in zip(init, ("dw1", "db1", "dw2", "db2"))]
            two.append((gr, cabi.make("mds_se_fc_bwd_args", groups=G, C=C, R=R, rows_per_group=70, dgate=dgate, gate=gate, hidden=hidden,
                                      pooled=pooled, w1=w1, w2=w2, dpooled=be.out((G, C), torch.float32, float("nan")), scratch=scratch,
                                      dw1=gr[0], db1=gr[1], dw2=gr[2], db2=gr[3])))
        be.call("se_fc_bwd_params", two[0][1])
        jobs.append(two[1][1]); outs.append((two[0][0], two[1][0]))
    arr = (SJ * len(jobs))(*jobs)
    tab = be.t(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))
    be.call("se_fc_bwd_params_table", cabi.make("mds_se_fc_bwd_table_args", jobs=tab, njobs=len(jobs), max_rc=max(C * R for C, R in shapes)))
    be.sync()
    for (C, R), (ref, got) in zip(shapes, outs):
        for a_, b_, name in zip(ref, got, ("dw1", "db1", "dw2", "db2")):
            assert torch.equal(a_.cpu(), b_.cpu()), (C, R, name)
    with pytest.raises(Exception):
        be.call("se_fc_bwd_params_table", cabi.make("mds_se_fc_bwd_table_args", jobs=tab, njobs=0, max_rc=1))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,C", [(0, 40), (1, 40), (2, 40), (3, 40), (1, 1152)])
def test_bn_backward_chain(be, dt, mode, C):
    """reduce -> finalize -> apply == autograd through act(batch_norm(y)) for every g-source
    (C = 1152 takes the two-slice path of the reduce kernels)."""
    code, tdt = DT[dt]
    M, rpg = 330, 110
    G = M // rpg
    g = gen(11 + mode)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(tdt)
    u = torch.randn(M, C, generator=g).to(tdt)
    gamma = 1 + 0.2 * torch.randn(C, generator=g); beta = 0.2 * torch.randn(C, generator=g)
    gate = torch.rand(G, C, generator=g); dpool = 0.1 * torch.randn(G, C, generator=g)
    mask = torch.tensor([0.0, 1.25, 1.25])
    eps = 1e-5
    yf = y.float().requires_grad_(True)
    gam = gamma.clone().requires_grad_(True); bet = beta.clone().requires_grad_(True)
    z = F.batch_norm(yf, None, None, gam, bet, True, 0.1, eps)
    grp = torch.arange(M) // rpg
    uf = u.float()
    if mode == 0:
        z.backward(uf)
    elif mode == 1:
        F.silu(z).backward(uf)
    elif mode == 2:
        F.silu(z).backward(uf * gate[grp] + dpool[grp])
    else:
        (z * mask[grp, None]).backward(uf)
    # kernels
    stats = torch.zeros(SLOTS, 2, C, dtype=torch.float64)
    stats[0, 0] = y.float().sum(0); stats[0, 1] = (y.float() ** 2).sum(0)
    bn = bn_finalize(be, be.t(stats), M, be.t(gamma), be.t(beta), eps=eps)
    gs = cabi.gsrc(mode, be.t(u), be.t(gate), be.t(dpool), be.t(mask, name="mask"), rpg)
    st2 = be.out((SLOTS, 2, C), torch.float64, 0)     # backward sums: fp64 slots
    yd = be.t(y)
    be.call("bn_bwd_reduce", cabi.make("mds_bn_bwd_reduce_args", dtype=code, M=M, C=C, g=gs, y=yd, bn=bn, stats=st2))
    dgamma = be.out(C, torch.float32, 0, name="dgamma"); dbeta = be.out(C, torch.float32, 0, name="dbeta")
    coef = be.out((3, C), torch.float32, float("nan"))
    be.call("bn_bwd_finalize", cabi.make("mds_bn_bwd_finalize_args", C=C, count=M, stats=st2, gamma=be.t(gamma),
                                         bn=bn, dgamma=dgamma, dbeta=dbeta, coef=coef, batch_stats=1))
    dy = be.out((M, C), tdt, float("nan"))
    be.call("bn_bwd_apply", cabi.make("mds_bn_bwd_apply_args", dtype=code, M=M, C=C, g=gs, y=yd, bn=bn, coef=coef, dy=dy))
    be.sync()
    check_bn_bwd_sums(dgamma, dbeta, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, dt)
    assert_close(dy, yf.grad, dt, scale=2, msg="dy")


def bn_bwd_reference(y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, running=None):
    """float64 autograd through act(batch_norm(y)) for the four gradient sources of mds_gsrc_t -> dy, dgamma, dbeta, on exactly
    the stored y and u; running = (mean, var): eval-mode BatchNorm (the statistics are constants)"""
    F64 = torch.float64
    M = y.shape[0]
    yd = y.to(F64).requires_grad_(True)
    gam = gamma.to(F64).requires_grad_(True); bet = beta.to(F64).requires_grad_(True)
    if running is None:
        z = F.batch_norm(yd, None, None, gam, bet, True, 0.1, eps)
    else:
        z = F.batch_norm(yd, running[0].to(F64), running[1].to(F64), gam, bet, False, 0.1, eps)
    grp = torch.arange(M) // rpg
    ud = u.to(F64)
    if mode == cabi.MDS_G_PLAIN:
        z.backward(ud)
    elif mode == cabi.MDS_G_SILU:
        F.silu(z).backward(ud)
    elif mode == cabi.MDS_G_SE_SILU:
        F.silu(z).backward(ud * gate.to(F64)[grp] + dpool.to(F64)[grp])
    else:
        (z * mask.to(F64)[grp, None]).backward(ud)
    return yd.grad, gam.grad, bet.grad


def _bn_bwd_chain(be, dt, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, use64=False, running=None):
    """reduce -> finalize -> apply; use64: with fwd_stats / coef64 (the fp64 means of the fp32 training plans, engine.py);
    running = (mean, var): batch_stats = 0 on the table of mds_bn_finalize(training = 0).  -> dy, dgamma, dbeta, coef, lin"""
    code, tdt = DT[dt]
    M, C = y.shape
    fwd = torch.zeros(SLOTS, 2, C, dtype=torch.float64)
    fwd[0, 0] = y.double().sum(0); fwd[0, 1] = (y.double() ** 2).sum(0)
    fwd = be.t(fwd)
    if running is None:
        bn = bn_finalize(be, fwd, M, be.t(gamma), be.t(beta), eps=eps)
    else:
        bn = bn_finalize(be, None, 0, be.t(gamma), be.t(beta), eps=eps, training=0, rm=be.t(running[0]), rv=be.t(running[1]))
    gs = cabi.gsrc(mode, be.t(u), be.t(gate) if gate is not None else None, be.t(dpool) if dpool is not None else None,
                   be.t(mask) if mask is not None else None, rpg)
    st2 = be.out((SLOTS, 2, C), torch.float64, 0)
    yd = be.t(y)
    be.call("bn_bwd_reduce", cabi.make("mds_bn_bwd_reduce_args", dtype=code, M=M, C=C, g=gs, y=yd, bn=bn, stats=st2))
    dgamma = be.out(C, torch.float32, 0, name="dgamma"); dbeta = be.out(C, torch.float32, 0, name="dbeta")
    coef = be.out((3, C), torch.float32, float("nan")); lin = be.out((3, C), torch.float32, float("nan"))
    coef64 = be.out((3, C), torch.float64, float("nan")) if use64 else None
    be.call("bn_bwd_finalize", cabi.make("mds_bn_bwd_finalize_args", C=C, count=M, stats=st2, gamma=be.t(gamma), bn=bn, dgamma=dgamma,
                                         dbeta=dbeta, coef=coef, lin=lin, batch_stats=0 if running is not None else 1,
                                         fwd_stats=fwd if use64 else None, coef64=coef64))
    dy = be.out((M, C), tdt, float("nan"))
    be.call("bn_bwd_apply", cabi.make("mds_bn_bwd_apply_args", dtype=code, M=M, C=C, g=gs, y=yd, bn=bn, coef=coef, dy=dy, coef64=coef64))
    be.sync()
    return dy, dgamma, dbeta, coef, lin


def _bn_bwd_inputs(M, C, rpg, tdt, seed):
    g = gen(seed)
    G = (M + rpg - 1) // rpg
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(tdt)
    u = torch.randn(M, C, generator=g).to(tdt)
    gamma = 1 + 0.2 * torch.randn(C, generator=g); beta = 0.2 * torch.randn(C, generator=g)
    gate = torch.rand(G, C, generator=g); dpool = 0.1 * torch.randn(G, C, generator=g)
    mask = (torch.rand(G, generator=g) > 0.3).float() / 0.7
    return g, y, u, gamma, beta, gate, dpool, mask


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_bn_backward_chain_fp64_means(be, mode):
    """mds_bn_bwd_finalize_args.fwd_stats / coef64 and mds_bn_bwd_apply_args.coef64 (every fp32 training plan passes them): the
    batch mean from the forward pass's fp64 sums, sum g / M and sum g * xhat / M in fp64, subtracted in fp64 in the apply pass -
    against float64 autograd for every g-source, at the fp32 tolerance of test_bn_backward_chain"""
    M, C, rpg, eps = 330, 40, 110, 1e-5
    _, y, u, gamma, beta, gate, dpool, mask = _bn_bwd_inputs(M, C, rpg, torch.float32, 61 + mode)
    dy_ref, dgamma_ref, dbeta_ref = bn_bwd_reference(y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps)
    dy, dgamma, dbeta, _, _ = _bn_bwd_chain(be, "f32", y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, use64=True)
    check_bn_bwd_sums(dgamma, dbeta, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, "f32")
    assert_close(dy, dy_ref, "f32", scale=2, msg="dy")


def test_bn_backward_fp64_means_keep_the_column_sums(be):
    """what coef64 is there for: the fp32-rounded means are the SAME for every row, so their rounding error adds up M times in
    every column sum of dy (the bias gradients upstream).  A per-channel offset in y (mean ~ 10: half an ulp is 5e-7) and a
    gradient that correlates with y and has a mean of its own (sum g / M and sum g * xhat / M of order 1) make that error
    M * ~1e-7 per channel against ~sqrt(M) * 2e-8 from the one rounding per element that both forms share - at M = 20 000 rows
    two orders of magnitude apart.  In exact arithmetic every column sum of dy is zero."""
    M, C, rpg, eps = 20000, 16, 20000, 1e-5
    g = gen(71)
    off = 8 + 4 * torch.rand(C, generator=g)
    y = torch.randn(M, C, generator=g) + off
    u = torch.randn(M, C, generator=g) + 0.5 * (y - off) + 1.0
    gamma = 1 + 0.2 * torch.randn(C, generator=g); beta = 0.2 * torch.randn(C, generator=g)
    dy_ref, dgamma_ref, dbeta_ref = bn_bwd_reference(y, u, gamma, beta, 0, None, None, None, rpg, eps)
    err = {}
    for use64 in (False, True):
        dy, dgamma, dbeta, _, _ = _bn_bwd_chain(be, "f32", y, u, gamma, beta, 0, None, None, None, rpg, eps, use64=use64)
        assert_close(dy, dy_ref, "f32", scale=2, msg=f"dy (coef64: {use64})")
        check_bn_bwd_sums(dgamma, dbeta, y, u, gamma, beta, 0, None, None, None, rpg, eps, "f32")
        err[use64] = float((dy.cpu().double().sum(0) - dy_ref.sum(0)).abs().max())
    assert err[True] <= err[False], f"worst column sum of dy: {err[True]:.3e} off the float64 sum with coef64, {err[False]:.3e} without"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [1, 3])
def test_bn_backward_eval_mode(be, dt, mode):
    """mds_bn_bwd_finalize_args.batch_stats = 0: the BatchNorm backward of the frozen-encoder configuration - running statistics
    (the table of mds_bn_finalize with training = 0) are constants, so coef1 = coef2 = 0 and dy = gamma * rstd * g; dgamma / dbeta
    are still the sums; lin = {A, 0, 0}"""
    code, tdt = DT[dt]
    M, C, rpg, eps = 330, 40, 110, 1e-5
    g, y, u, gamma, beta, gate, dpool, mask = _bn_bwd_inputs(M, C, rpg, tdt, 81 + mode)
    rm = 0.3 + 0.2 * torch.randn(C, generator=g); rv = 1.5 + torch.rand(C, generator=g)
    dy_ref, dgamma_ref, dbeta_ref = bn_bwd_reference(y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, running=(rm, rv))
    dy, dgamma, dbeta, coef, lin = _bn_bwd_chain(be, dt, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, running=(rm, rv))
    check_bn_bwd_sums(dgamma, dbeta, y, u, gamma, beta, mode, gate, dpool, mask, rpg, eps, dt, running=(rm, rv))
    assert_close(dy, dy_ref, dt, scale=2, msg="dy")
    A = gamma.double() / torch.sqrt(rv.double() + eps)
    assert_close(coef[0], A, "f32", msg="coef0"); assert_close(lin[0], A, "f32", msg="A")
    assert float(coef[1:].abs().sum()) == 0.0 and float(lin[1:].abs().sum()) == 0.0, "coef1 = coef2 = 0, B = D = 0"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("pro_mode,split,R_,C", [(0, False, 35, 16), (2, False, 35, 16), (2, True, 35, 16), (2, True, 920, 64)])
def test_gem_fwd_bwd(be, dt, pro_mode, split, R_, C, golden):
    """single-block path and the row-split path (caller-zeroed accumulators)"""
    code, tdt = DT[dt]
    G = 4
    g = gen(21)
    y = (torch.randn(G * R_, C, generator=g) * 1.5).to(tdt)
    scale = 1 + 0.2 * torch.randn(C, generator=g); shift = 0.2 * torch.randn(C, generator=g)
    p = torch.tensor([3.0]); dpo = torch.randn(G, C, generator=g)
    yf = y.float().requires_grad_(True); pp = p.clone().requires_grad_(True)
    a = F.silu(yf * scale + shift) if pro_mode else yf
    a.retain_grad()
    pooled_ref = a.view(G, R_, C).clamp(min=1e-6).pow(pp).mean(1).pow(1.0 / pp)
    (pooled_ref * dpo).sum().backward()
    yd = be.t(y)
    pro = cabi.pro(pro_mode, be.t(scale), be.t(shift))
    pooled = be.out((G, C), torch.float32, float("nan")); pd = be.t(p)
    acc1 = be.out((G, C), torch.float64, 0) if split else None
    acc2 = be.out((G, C), torch.float64, 0) if split else None
    be.call("gem_fwd", cabi.make("mds_gem_fwd_args", dtype=code, groups=G, rows_per_group=R_, C=C, y=yd, pro=pro,
                                 p=pd, eps=1e-6, pooled=pooled, accum=acc1))
    u = be.out((G * R_, C), tdt, float("nan")); dp = be.out(1, torch.float32, 0, name="dp")
    be.call("gem_bwd", cabi.make("mds_gem_bwd_args", dtype=code, groups=G, rows_per_group=R_, C=C, y=yd, pro=pro,
                                 p=pd, eps=1e-6, pooled=pooled, dpooled=be.t(dpo), u=u, dp=dp, accum=acc2))
    be.sync()
    assert_close(pooled, pooled_ref, dt, msg="pooled")
    assert_close(u, a.grad, dt, msg="u")
    check_gem_dp(dp, y, scale, shift, pro_mode, 3.0, dpo, G, R_, 1e-6, dt)


def test_gem_matches_reference_golden(be, golden):
    """GeM against the vectors produced by the reference class itself (tests/golden/gem.npz)."""
    d = golden("gem")
    x = torch.from_numpy(d["x"])                       # (2,6,5,7) NCHW
    B, C, H, W = x.shape
    Cp = 8                                             # pad channels to the kernel's multiple of 8
    rows = torch.zeros(B * H * W, Cp)
    rows[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    rows[:, C:] = 1.0
    pooled = be.out((B, Cp), torch.float32, float("nan")); p = be.t(torch.tensor([3.0]))
    yd = be.t(rows)
    be.call("gem_fwd", cabi.make("mds_gem_fwd_args", dtype=0, groups=B, rows_per_group=H * W, C=Cp, y=yd,
                                 pro=cabi.pro(0), p=p, eps=1e-6, pooled=pooled))
    dpo = torch.zeros(B, Cp); dpo[:, :C] = torch.from_numpy(d["g"])
    u = be.out((B * H * W, Cp), torch.float32, float("nan")); dp = be.out(1, torch.float32, 0, name="dp")
    be.call("gem_bwd", cabi.make("mds_gem_bwd_args", dtype=0, groups=B, rows_per_group=H * W, C=Cp, y=yd,
                                 pro=cabi.pro(0), p=p, eps=1e-6, pooled=pooled, dpooled=be.t(dpo), u=u, dp=dp))
    be.sync()
    assert_close(pooled[:, :C], torch.from_numpy(d["y"]), "f32", msg="y")
    dx = u.cpu()[:, :C].view(B, H, W, C).permute(0, 3, 1, 2)
    assert_close(dx, torch.from_numpy(d["dx"]), "f32", msg="dx")
    assert_close(gem_dp64(rows, None, None, 0, 3.0, dpo, B, H * W, 1e-6)[0], torch.from_numpy(d["dp"]), "f32", msg="the float64 dp is the reference class's")
    check_gem_dp(dp, rows, None, None, 0, 3.0, dpo, B, H * W, 1e-6, "f32")


def test_head_fwd_bwd(be):
    B, Fdim, NC = 3, 200, 5
    g = gen(31)
    pooled = torch.randn(B, Fdim, generator=g); w = torch.randn(NC, Fdim, generator=g) * 0.1
    b = torch.randn(NC, generator=g); mask = (torch.rand(B, Fdim, generator=g) > 0.2).float() / 0.8
    dl = torch.randn(B, NC, generator=g)
    pf = pooled.clone().requires_grad_(True); wf = w.clone().requires_grad_(True); bf = b.clone().requires_grad_(True)
    ref = F.linear(pf * mask, wf, bf)
    ref.backward(dl)
    logits = be.out((B, NC), torch.float32, float("nan"))
    pd, md, wd = be.t(pooled), be.t(mask, name="mask"), be.t(w)
    be.call("head_fwd", cabi.make("mds_head_fwd_args", B=B, F=Fdim, NC=NC, pooled=pd, mask=md, w=wd, b=be.t(b), logits=logits))
    dpo = be.out((B, Fdim), torch.float32, float("nan")); dw = be.out((NC, Fdim), torch.float32, 0, name="dw"); db = be.out(NC, torch.float32, 0, name="db")
    be.call("head_bwd", cabi.make("mds_head_bwd_args", B=B, F=Fdim, NC=NC, pooled=pd, mask=md, w=wd, dlogits=be.t(dl),
                                  dpooled=dpo, dw=dw, db=db))
    be.sync()
    assert_close(logits, ref, "f32"); assert_close(dpo, pf.grad, "f32")
    assert_close(dw, wf.grad, "f32"); assert_close(db, bf.grad, "f32")


@pytest.mark.parametrize("tta", [1, 2, 3])
def test_head_fwd_probs(be, tta):
    """the predictor's nn.Sigmoid + mean over the TTA group (src/predictors.py:69-70) from the head's own launch"""
    B, Fdim, NC = 6, 333, 2
    g = gen(32 + tta)
    pooled = torch.randn(B, Fdim, generator=g); w = torch.randn(NC, Fdim, generator=g) * 0.1; b = torch.randn(NC, generator=g)
    ref = F.linear(pooled, w, b)
    logits = be.out((B, NC), torch.float32, float("nan")); probs = be.out((B // tta, NC), torch.float32, float("nan"))
    be.call("head_fwd", cabi.make("mds_head_fwd_args", B=B, F=Fdim, NC=NC, pooled=be.t(pooled), mask=None, w=be.t(w), b=be.t(b),
                                  logits=logits, probs=probs, tta=tta))
    be.sync()
    assert_close(logits, ref, "f32")
    assert_close(probs, torch.sigmoid(ref).view(B // tta, tta, NC).mean(1), "f32")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pack_weights(be, dt):
    import ctypes as C_
    code, tdt = DT[dt]
    g = gen(41)
    w3 = torch.randn(20, 12, 3, 3, generator=g); w1 = torch.randn(24, 16, 1, 1, generator=g)
    ws = torch.randn(32, 3, 3, 3, generator=g)
    srcs = [be.t(w3), be.t(w3), be.t(w1), be.t(ws)]
    dsts = [be.out(20 * 9 * 12, tdt, float("nan")), be.out(12 * 9 * 20, tdt, float("nan")),
            be.out(24 * 16, tdt, float("nan")), be.out(32 * 32, tdt, float("nan"))]
    kinds = [(0, 20, 12, 9), (1, 20, 12, 9), (0, 24, 16, 1), (2, 32, 27, 1)]
    Job = cabi.STRUCTS["mds_pack_job"]
    jobs = (Job * 4)()
    for j, (s, d, (k, O, I, t)) in enumerate(zip(srcs, dsts, kinds)):
        jobs[j].src = be.ptr(s); jobs[j].dst = be.ptr(d); jobs[j].kind = k; jobs[j].O = O; jobs[j].I = I; jobs[j].taps = t
    be.call_raw("pack_weights", jobs, 4, 20 * 12 * 9, code)
    be.sync()
    assert_close(dsts[0].view(20, 9, 12), w3.view(20, 12, 9).permute(0, 2, 1), dt)
    assert_close(dsts[1].view(12, 9, 20), w3.view(20, 12, 9).flip(2).permute(1, 2, 0), dt)
    assert_close(dsts[2].view(24, 16), w1.view(24, 16), dt)
    ref = torch.zeros(32, 32); ref[:, :27] = ws.view(32, 27)
    assert_close(dsts[3].view(32, 32), ref, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("O,I", [(24, 16), (70, 44), (192, 1152), (33, 5)])
def test_pack_weights_transposed(be, dt, O, I):
    """[O][I] -> [I][O] packs (MDS_PACK_IO_FLIP with one tap: the 1x1 data-gradient filters; MDS_PACK_IO_F32: the fp32
    squeeze-excite w2 copy) go through 32 x 32 LDS tiles: ragged edges, several tiles per block."""
    code, tdt = DT[dt]
    w = torch.randn(O, I, generator=gen(43))
    src = be.t(w)
    d_flip = be.out(I * O, tdt, float("nan"))
    d_f32 = be.out(I * O, torch.float32, float("nan"))
    Job = cabi.STRUCTS["mds_pack_job"]
    jobs = (Job * 2)()
    for j, (d, k) in enumerate(((d_flip, cabi.MDS_PACK_IO_FLIP), (d_f32, cabi.MDS_PACK_IO_F32))):
        jobs[j].src = be.ptr(src); jobs[j].dst = be.ptr(d); jobs[j].kind = k; jobs[j].O = O; jobs[j].I = I; jobs[j].taps = 1
    be.call_raw("pack_weights", jobs, 2, O * I, code)
    be.sync()
    assert_close(d_flip.view(I, O), w.t(), dt)
    assert torch.equal(d_f32.view(I, O).cpu(), w.t().contiguous())
