"""The summation-bound helpers of tests/backends.py prove themselves: plain torch on the CPU, no kernels.  What the kernel tests
rely on: a faithful fp32 sum in any order is far inside the bound, a sum with a seam's share missing is outside it, a probe that
probes nothing is refused, and assert_close no longer takes a tolerance that grows with the size of a sum."""
import pytest
import torch
import torch.nn.functional as F

from backends import ABS, U, assert_close, assert_sum_close, assert_stats_close, bf16_ulp, near_tie, pro_operand, stat_parts


def conv_case(N=2, H=13, W=37, Cin=32, Cout=128, seed=0):
    """the 3x3 layer of test_c3_filter_in_registers' first case: bf16 operands, float64 products, channels last"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).bfloat16().double()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).bfloat16().double()
    v = F.conv2d(x, w, None, 1, 1).permute(0, 2, 3, 1).contiguous()
    vabs = F.conv2d(x.abs(), w.abs(), None, 1, 1).permute(0, 2, 3, 1).contiguous()
    return x, w, v, vabs


PROBES = [("last 5 columns left out", lambda t: t[:, :, :-5]), ("row 0 counted twice", lambda t: torch.cat([t, t[:, :1]], 1)),
          ("last image left out", lambda t: t[:-1])]


def fp32_sums(v):
    """a faithful fp32 evaluation in an order of its own: fp32 values, summed pixel by pixel in fp32 from the LAST pixel backwards"""
    p = v.float().flatten(0, 2).flip(0)
    s, q = torch.zeros(p.shape[1]), torch.zeros(p.shape[1])
    for row in p:
        s, q = s + row, q + row * row
    return torch.stack([s, q])


def test_a_faithful_fp32_sum_is_far_inside_the_bound_and_the_probes_hold():
    x, w, v, vabs = conv_case()
    cnt = v[..., 0].numel()
    got = fp32_sums(v)
    assert_stats_close(got, v, vabs, 9 * 32, cnt, ("bf16", cnt ** 0.5), None, PROBES)
    for i, (want, parts) in enumerate(stat_parts(v, vabs, 9 * 32, cnt).values()):
        bound = sum((c + 8) * U * m for c, m in parts)
        # (the fp32 conversion of v itself is one rounding per term: inside the + 8)
        assert float(((got[i].double() - want).abs() / bound).max()) < 0.05


@pytest.mark.parametrize("name,f", PROBES)
def test_a_wrong_sum_is_out_of_bound_where_the_old_tolerance_passed_it(name, f):
    """each probe as the kernel's answer: assert_sum_close fails, and the size-scaled bf16 tolerance it replaces would have passed"""
    x, w, v, vabs = conv_case()
    cnt = v[..., 0].numel()
    red = (0, 1, 2)
    wrong = torch.stack([f(v).sum(red), (f(v) ** 2).sum(red)])
    with pytest.raises(AssertionError, match="out of bound"):
        assert_stats_close(wrong, v, vabs, 9 * 32, cnt, ("bf16", cnt ** 0.5))
    for i, want in enumerate((v.sum(red), (v * v).sum(red))):
        err = (wrong[i] - want).abs()
        old = err <= 2e-2 * cnt ** 0.5 * max(1.0, float(want.abs().max())) + 2e-2 * want.abs()
        assert float(old.double().mean()) > 0.95, "the old bound let (nearly) every element of this wrong answer pass"


def test_a_probe_equal_to_the_reference_is_refused():
    x, w, v, vabs = conv_case()
    want, parts = stat_parts(v, vabs, 9 * 32, v[..., 0].numel())["sum"]
    with pytest.raises(AssertionError, match="probes nothing"):
        assert_sum_close(want.clone(), want, parts, "sum", [("nothing left out", want.clone())])


def test_a_probe_below_the_bound_is_refused():
    """one pixel is below the resolution of `sumsq` at this shape: a probe must be chosen so that the bound resolves it"""
    x, w, v, vabs = conv_case()
    want, parts = stat_parts(v, vabs, 9 * 32, v[..., 0].numel())["sumsq"]
    one = want - v[0, 0, 0] ** 2
    with pytest.raises(AssertionError, match="does not resolve"):
        assert_sum_close(want.clone(), want, parts, "sumsq", [("one pixel left out", one)])


def test_nan_and_shape_fail():
    want, mag = torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    got = want.clone(); got[2] = float("nan")
    with pytest.raises(AssertionError, match="out of bound"):
        assert_sum_close(got, want, [(10, mag)], "sum")
    with pytest.raises(AssertionError, match="shape"):
        assert_sum_close(want[:3], want, [(10, mag)], "sum")
    assert_sum_close(want + 17 * U, want, [(10, mag)], "sum")           # (10 + 8) U: inside
    with pytest.raises(AssertionError):
        assert_sum_close(want + 19 * U, want, [(10, mag)], "sum")
    assert_sum_close(want + 0.5, want, [(10, mag), (ABS, 0.5 * mag)], "sum")    # an absolute part counts as it stands


def test_the_cap_keeps_the_old_bound_where_it_was_tighter():
    want = torch.full((3,), 100.0, dtype=torch.float64)
    loose = [(ABS, torch.full((3,), 50.0, dtype=torch.float64))]
    assert_sum_close(want + 1.0, want, loose, "sum")
    with pytest.raises(AssertionError):
        assert_sum_close(want + 1.0, want, loose, "sum", cap=("f32", 2.0))      # 2e-5 * 2 * 100 + 2e-4 * 100 = 0.024


def test_assert_close_refuses_a_size_scaled_tolerance():
    a = torch.ones(5)
    assert_close(a, a, "bf16", scale=2, msg="y")
    with pytest.raises(AssertionError, match="assert_sum_close"):
        assert_close(a, a, "bf16", scale=400 ** 0.5, msg="sum")


def test_near_tie_set_and_operand_error():
    """bf16 neighbours 1 and 1 + 2^-7: the tie sits at 1 + 2^-8; an element closer to it than delta is in the set, and pro_operand
    charges exactly one bf16 ulp for it and nothing elsewhere"""
    a = torch.tensor([1 + 2.0 ** -8 + 1e-9, 1 + 2.0 ** -8 + 1e-4, 1.0, -(3 + 2.0 ** -7) * (1 - 1e-10), 0.0], dtype=torch.float64)
    assert near_tie(a, 1e-8).tolist() == [True, False, False, True, False]
    assert bf16_ulp(a).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0]
    z = torch.linspace(-6, 6, 200001, dtype=torch.float64)
    aq, err = pro_operand(z, z.abs(), True, "bf16")
    assert torch.equal(aq, (z * torch.sigmoid(z)).bfloat16().double())
    assert 0 < int((err > 0).sum()) < 0.01 * z.numel(), "the near-tie set is a small part of the elements"
    # the float32 evaluation torch itself makes rounds differently from float64 only inside the set
    a32 = F.silu(z.float()).bfloat16().double()
    assert bool(((a32 - aq).abs() <= err).all())
    a_, e32 = pro_operand(z, z.abs(), True, "f32")
    assert bool(((F.silu(z.float()).double() - a_).abs() <= e32).all())
