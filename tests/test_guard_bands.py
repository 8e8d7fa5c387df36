"""The guard-band harness of tests/backends.py proves itself: plain torch writes, no kernels, on both backends.  Every write stays
inside one parent allocation (payload + its own guards), so nothing here is out of bounds for the device."""
import re

import pytest
import torch

from backends import Backend, assert_close, be, guard_bytes  # noqa: F401
from mds import cabi

SENTINEL = 2.0 ** -100
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]


def parent_of(be, v):
    """(the uint8 parent allocation, payload offset) of a guarded buffer"""
    rec = be._known[v.data_ptr()]
    return rec.parent, rec.off


def hit(be, name, side, offset):
    with pytest.raises(AssertionError) as e:
        be.sync()
    msg = str(e.value)
    assert f"'{name}'" in msg and f"{side} the payload" in msg, msg
    assert int(re.search(r"offset ([+-]\d+)", msg).group(1)) == offset, msg
    be.sync()       # the registry was cleared: nothing is reported twice


def test_guard_size_is_the_stated_condition():
    assert guard_bytes(0) == 4096 and guard_bytes(4097) == 4608 and guard_bytes(1 << 20) == 1 << 20 and guard_bytes(1 << 30) == 1 << 20
    assert all(guard_bytes(n) % 512 == 0 and guard_bytes(n) >= max(4096, min(n, 1 << 20)) for n in (1, 511, 5000, 99999, (1 << 20) + 1))


@pytest.mark.parametrize("dtype", DTYPES + [torch.int32, torch.uint8, torch.int64])
def test_promised_addresses_and_fills(be, dtype):
    x = torch.arange(35).reshape(5, 7).to(dtype)
    for align, mod, res in ((16, 32, 16), (4, 16, 8 if dtype in (torch.float64, torch.int64) else 4)):
        a, o = be.t(x, align=align), be.out((5, 7), dtype, 0, align=align)
        for v in (a, o):
            assert v.data_ptr() % mod == res and v.is_contiguous() and v.shape == (5, 7) and v.dtype == dtype and v.device.type == be.device.type
            parent, off = parent_of(be, v)
            assert off >= 4096 and parent.numel() - off - v.numel() * v.element_size() >= 4096
        assert torch.equal(a.cpu(), x) and float(o.float().abs().sum()) == 0
        parent, off = parent_of(be, a)
        before, after = parent[:off].view(dtype), parent[off + a.numel() * a.element_size():][:64].view(dtype)
        parent_o, off_o = parent_of(be, o)
        before_o = parent_o[:off_o].view(dtype)
        if dtype.is_floating_point:
            assert bool(torch.isnan(before).all()) and bool(torch.isnan(after).all())
            want = 2.0 ** -14 if dtype == torch.float16 else SENTINEL        # fp16 has no 2^-100: its smallest normal number
            assert bool((before_o.double() == want).all()), "the sentinel is exact and normal in the buffer's type"
        else:
            assert bool((parent[:off] == 0xA5).all()) and bool((parent_o[:off_o] == 0x5A).all())
    assert int(parent_of(be, be.out(3, torch.int32, 0))[0][:4].view(torch.int32)) == 0x5A5A5A5A
    be.sync()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clean_round_trip_passes(be, dtype):
    x = torch.randn(37, 9).to(dtype)
    a, o = be.t(x), be.out((37, 9), dtype, float("nan"))
    o.copy_(a * 2)
    o += 1
    be.sync()
    assert torch.equal(o.cpu(), x * 2 + 1)


@pytest.mark.parametrize("dtype", DTYPES + [torch.int32])
def test_one_element_before_after_and_at_the_far_end(be, dtype):
    isz = torch.empty((), dtype=dtype).element_size()
    n = 3000
    G = guard_bytes(n * isz)
    for where, side, offset in (("before", "before", -isz), ("after", "after", 0), ("far", "after", G - isz), ("far before", "before", None)):
        y = be.out(n, dtype, 0, name="y")
        be.out(16, dtype, 0, name="bystander")
        parent, off = parent_of(be, y)
        typed = parent.view(dtype)
        first = off // isz
        idx = {"before": first - 1, "after": first + n, "far": first + n + G // isz - 1, "far before": 0}[where]
        typed[idx] = 1
        hit(be, "y", side, -off if offset is None else offset)


def test_an_atomic_style_add_into_an_out_guard(be):
    """what a NaN guard would absorb: x + 1e-3 is NaN bit for bit when x is NaN, and differs from 2^-100 when x is 2^-100"""
    for dtype in DTYPES:
        y = be.out((6, 10), dtype, 0, name="sums")
        parent, off = parent_of(be, y)
        end = off + 60 * y.element_size()
        parent[end:end + 10 * y.element_size()].view(dtype).add_(1e-3)     # one row of 10 past the last
        hit(be, "sums", "after", 0)
    nan = torch.full((4,), float("nan"))
    assert torch.equal((nan + 1e-3).view(torch.int32), nan.view(torch.int32))


def test_a_store_into_an_inputs_guard(be):
    x = be.t(torch.randn(20, 8), name="x")
    parent, off = parent_of(be, x)
    parent[off + 640 + 64:].view(torch.float32)[0] = 0.0
    hit(be, "x", "after", 64)
    idx = be.t(torch.arange(5, dtype=torch.int32), name="slots")
    parent, off = parent_of(be, idx)
    parent[off - 1] = 0
    hit(be, "slots", "before", -1)


def test_buffers_are_named_by_position_without_a_name(be):
    be.sync()
    start = be._serial
    be.t(torch.zeros(3)); y = be.out(3, torch.float32, 0)
    parent, off = parent_of(be, y)
    parent[off - 4:off].view(torch.float32)[0] = 2.0
    hit(be, f"out#{start + 2}", "before", -4)


def test_a_consumed_over_read_poisons_the_result(be):
    """a reference-only 'kernel' that reads one row too many: in a fresh tensor of its own the row behind would be finite slack"""
    M = 12
    x = be.t(torch.randn(M, 8))
    parent, off = parent_of(be, x)
    rows = parent[off:off + (M + 1) * 32].view(torch.float32).view(M + 1, 8)       # what a kernel indexing row M reaches
    assert bool(torch.isnan(rows.sum(0)).all()) and bool(torch.isnan((rows * torch.cat([torch.ones(M, 1), torch.zeros(1, 1)]).to(be.device)).sum(0)).all())
    assert bool(torch.isfinite(x.sum(0)).all())
    be.sync()


def test_call_refuses_an_unguarded_tensor(be):
    M, K, N = 64, 16, 16
    x, w = be.t(torch.randn(M, K)), be.t(torch.randn(N, K))
    stray = torch.zeros(M, N, device=be.device)
    args = cabi.make("mds_pw_fwd_args", dtype=0, M=M, K=K, N=N, x=x, w=w, y=stray, pro=cabi.pro(0), residual=None, stats=None)
    with pytest.raises(AssertionError, match="unguarded tensor"):
        be.call("pw_fwd", args)
    nested = cabi.make("mds_pw_fwd_args", dtype=0, M=M, K=K, N=N, x=x, w=w, y=be.out((M, N), torch.float32, 0),
                       pro=cabi.pro(1, torch.ones(K, device=be.device), be.t(torch.zeros(K))), residual=None, stats=None)
    with pytest.raises(AssertionError, match="unguarded tensor"):
        be.call("pw_fwd", nested)
    with pytest.raises(AssertionError, match="unguarded tensor"):
        be.ptr(stray)
    y = be.out((M, N), torch.float32, 0)
    with pytest.raises(AssertionError, match="unguarded tensor"):
        be.ptr(y.view(-1)[M * N - 4:].as_strided((8,), (1,)))       # starts inside the payload, ends in the guard
    assert be.ptr(y[1:]) == y.data_ptr() + 4 * N                  # a slice of a guarded buffer is one
    assert float(stray.abs().sum()) == 0, "a refused call launched"
    be._launched = False                                          # (ptr() counts as a launch: none happened here)
    be.sync()


def test_a_launch_left_unverified_fails_at_teardown(be):
    fresh = Backend(be.name)                    # the fixture's teardown path on a backend of its own: same library, own registry
    y = fresh.out((64, 16), torch.float32, float("nan"))
    fresh.ptr(y)                                # what call() does with every tensor of a launch, without a kernel
    with pytest.raises(AssertionError, match="left unverified"):
        fresh.finish()
    fresh.finish()                              # verified by the failed teardown: clean now
    # and a guard hit that only the teardown sees fails there too
    z = fresh.out(8, torch.float32, 0, name="z")
    parent, off = parent_of(fresh, z)
    parent[off + 32:].view(torch.float32)[0] = 1.0
    with pytest.raises(AssertionError, match="'z'"):
        fresh.finish()


def test_assert_close_counts_a_nan_result_as_a_mismatch():
    """what the NaN guards rely on: `err > bound` is False for a NaN, so a poisoned element used to pass"""
    want = torch.ones(4, 3)
    got = want.clone()
    assert_close(got, want, "f32")
    got[2, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"1/12 mismatches.*first bad idx \[2, 1\]"):
        assert_close(got, want, "f32")
