"""Backends for the kernel tests: 'emu' = the same kernel sources run through the host simulator
(CPU tensors, no GPU needed); 'gpu' = the hipcc-built gfx950 library on cuda:0 (pytest -m gpu).

Every buffer a kernel test hands to a launch is a GUARDED buffer: Backend.t() (inputs) and Backend.out() (everything a launch
writes or accumulates into) return a view of the middle of a parent allocation of their own.  Each side of the payload carries
max(4 KiB, min(payload bytes, 1 MiB)) bytes of guard, rounded up to 512.
  - inputs: NaN guards (integers: 0xA5 bytes) - an over-read that is USED, even multiplied by zero, poisons the result;
  - outputs: the finite sentinel 2^-100 (fp16: 2^-14, its smallest normal number; integers: 0x5A bytes) - it changes under any store and under an atomic add of any normal
    number, which a NaN guard would absorb bit for bit.
The payload sits at an address = 16 mod 32 (16-byte aligned, on purpose not 32), or with align=4 at 4 mod 16 (fp64: 8 mod 16):
the least-aligned pointer the engine's dense arenas (Lazy.sub, carve, Plan.grad) produce.  Backend.sync() compares every guard
with its pattern bit for bit and raises AssertionError naming buffer, side and byte offset; Backend.call() refuses a tensor that
is not a guarded buffer; the fixtures verify once more on teardown and fail a test that left a launch unverified.

Two assertions: assert_close for elementwise outputs (the error is the store's rounding), assert_sum_close for every output that is
a sum over rows, pixels or groups - float64 on the operands the kernel holds, the a-priori fp32 summation bound on magnitudes, and
probes (wrong sums built from the reference) that the bound must still resolve.  tests/test_sum_bounds.py holds the helpers to that.

Out of scope, because they allocate inside product code (Plan / engine arenas, torch modules): test_train_ops.py,
test_augment.py, and the module, predictor and parallel tests - they use Backend only for its library handle and t()."""
import contextlib
import ctypes
import weakref

import pytest
import torch


_SENTINEL = 2.0 ** -100          # exactly representable and normal in bf16, fp32 and fp64
_SENTINEL_F16 = 2.0 ** -14       # fp16 cannot hold 2^-100 (it would be 0, which a store of 0 leaves unchanged): its smallest normal number
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_GUARD_FLOOR = 4096
_GUARD_CAP = 1 << 20
_PATTERN = {}                    # (dtype, "t" | "out") -> the guard fill's bit pattern as an integer of the element's size
# Every kernel instantiation ('conv_wgrad_kernel<float, 0, 2, 4, 9>') that a successful Backend.call() / Backend.rc() launched on
# the simulator in this process: the launches that ran on guarded buffers from a kernel test.  Launches a Plan issues (module,
# predictor, train-ops tests) do not pass through call() and are not in it - a whole-model comparison does not pin one variant.
# Kept by the simulator apart from its launch record, so reset_launches(), knobs() and the record's 65,536-entry cap leave it
# alone.  tests/test_zz_kernel_census.py compares it with the compiled kernels.
KERNEL_TEST_INSTANTIATIONS = set()


def guard_bytes(payload_bytes):
    """bytes of guard on EACH side of a payload: a stray row, tile or image row lands within one payload length"""
    return -(-max(_GUARD_FLOOR, min(payload_bytes, _GUARD_CAP)) // 512) * 512


class _Guarded:
    """one parent allocation: [guard | payload | guard]; `regions` are (side, typed-or-byte integer view, pattern, bytes per element)"""

    def __init__(self, name, kind, parent, view, off, nbytes):
        self.name, self.kind, self.parent, self.off, self.nbytes = name, kind, parent, off, nbytes
        self.view = weakref.ref(view)
        self.lo = view.data_ptr()
        self.hi = self.lo + max(nbytes, 1)
        self.regions = []

    def counts(self):
        return [(r != pat).count_nonzero() for _, r, pat, _ in self.regions]

    def first_bad(self):
        """(side, byte offset relative to the payload edge) of the lowest-addressed guard element that changed"""
        for (side, r, pat, isz) in self.regions:
            bad = (r != pat).nonzero()
            if bad.numel():
                i = int(bad[0]) * isz
                return (side, i - r.numel() * isz) if side == "before" else (side, i)


class Backend:
    def __init__(self, name):
        self.name = name
        if name == "emu":
            from hipemu.loader import load_emulator
            self.lib = load_emulator()
            self.device = torch.device("cpu")
        else:
            from mds.cabi import load
            self.lib = load()
            self.device = torch.device("cuda:0")
        self._known = {}        # payload address -> _Guarded, for as long as the payload view is alive
        self._pending = []      # guarded buffers created or launched on since the last verification (kept alive until then)
        self._serial = 0
        self._launched = False
        self._arena = {}        # name -> buffers placed at the arena alignment while arena(name, ...) is active

    def stream(self):
        if self.name == "emu":
            return 0
        return torch.cuda.current_stream().cuda_stream

    # ------------------------------------------------------------------------------------------------ guarded buffers
    def _alloc(self, kind, shape, dtype, align, name):
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
        isz = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for d in shape:
            numel *= int(d)
        nbytes = numel * isz
        G = guard_bytes(nbytes)
        if name in self._arena:
            align, self._arena[name] = 4, self._arena[name] + 1
        if align == 16:
            mod, res = 32, 16                       # 16-byte aligned and deliberately not 32
        elif align == 4:
            mod, res = 16, (4 if isz <= 4 else 8)   # the least alignment a dense carve of fp32 (fp64) sub-buffers produces
        else:
            raise ValueError(f"align={align}: 16 (default) or 4")
        parent = torch.empty(G + mod + nbytes + G, dtype=torch.uint8, device=self.device)
        off = G + (res - parent.data_ptr() - G) % mod
        assert off % isz == 0, "the allocator's base address is less aligned than the element size"
        total = off + nbytes + G
        view = parent[off:off + nbytes].view(dtype).view(shape)
        self._serial += 1
        rec = _Guarded(name or f"{kind}#{self._serial}", kind, parent, view, off, nbytes)
        floating = dtype.is_floating_point
        for side, a, b in (("before", 0, off), ("after", off + nbytes, total)):
            raw = parent[a:b]
            if floating:
                value = float("nan") if kind == "t" else (_SENTINEL_F16 if dtype == torch.float16 else _SENTINEL)
                if (dtype, kind) not in _PATTERN:       # the fill's bits, taken on the host once: nothing is copied back here
                    _PATTERN[dtype, kind] = int(torch.full((1,), value, dtype=dtype).view(_INT_VIEW[isz]))
                iv = raw.view(_INT_VIEW[isz])
                iv.fill_(_PATTERN[dtype, kind])         # (as bits: the same NaN on every device)
                rec.regions.append((side, iv, _PATTERN[dtype, kind], isz))
            else:
                pat = 0xA5 if kind == "t" else 0x5A      # 0x5A5A5A5A as an int32
                raw.fill_(pat)
                rec.regions.append((side, raw, pat, 1))
        assert view.data_ptr() % mod == res
        self._known[view.data_ptr()] = rec
        self._pending.append((rec, view))
        return view

    @contextlib.contextmanager
    def arena(self, *names):
        """for the body of a `with`: every buffer that t() / out() is asked for under one of `names` sits where the engine's dense
        arenas put it - at a 4-byte-only address (align=4).  Each name must be asked for at least once."""
        self._arena = dict.fromkeys(names, 0)
        try:
            yield
            missed = [n for n, k in self._arena.items() if k == 0]
            assert not missed, f"no buffer named {missed} was allocated: the arena case did not place what it names"
        finally:
            self._arena = {}

    def t(self, x, dtype=None, align=16, name=None):
        """an input: a contiguous copy of x in the middle of an allocation of its own, NaN (integers: 0xA5 bytes) on both sides"""
        x = torch.as_tensor(x)
        if dtype is not None:
            x = x.to(dtype)
        v = self._alloc("t", x.shape, x.dtype, align, name)
        v.copy_(x)
        return v

    def out(self, shape, dtype=torch.float32, fill=0, align=16, name=None):
        """a buffer a launch writes or accumulates into, filled with `fill`; 2^-100 (integers: 0x5A bytes) on both sides - finite,
        because most of these buffers are reached by atomic adds and NaN + x leaves a NaN guard bit-identical"""
        v = self._alloc("out", shape, dtype, align, name)
        if torch.is_tensor(fill):       # a buffer a launch accumulates into (+=) on top of given values
            v.copy_(fill)
        else:
            v.fill_(fill)
        return v

    def _lookup(self, tensor):
        p = tensor.data_ptr()
        rec = self._known.get(p)
        if rec is None or rec.view() is None:
            rec = next((r for r in self._known.values() if r.view() is not None and r.lo <= p < r.hi), None)
        if rec is None or p + tensor.numel() * tensor.element_size() > rec.lo + rec.nbytes:
            return None
        return rec

    def ptr(self, tensor):
        """address of a guarded buffer for an entry point that takes raw pointers (mds_pack_weights' job table, ...); raises like
        call() on anything that did not come from t() / out(), and counts as a launch to verify"""
        self._launched = self._launched or tensor is not None
        return self._guarded_ptr(tensor)

    def _guarded_ptr(self, tensor):
        if tensor is None:
            return 0
        rec = self._lookup(tensor)
        if rec is None:
            raise AssertionError(f"unguarded tensor {tuple(tensor.shape)} {tensor.dtype} passed to a launch: allocate it with be.t() / be.out()")
        assert tensor.is_contiguous()
        if not any(r is rec for r, _ in self._pending):
            self._pending.append((rec, rec.view()))
        return tensor.data_ptr()

    def call(self, op, args):
        """launch through the C ABI; every tensor of the argument struct (cabi.make's _keep list, nested structs included) must
        be a guarded buffer - a test cannot hand an unguarded tensor to a launch"""
        for tensor in getattr(args, "_keep", ()):
            self._guarded_ptr(tensor)
        self._inst_begin()
        self.lib.call(op, args, self.stream())      # raises when the launcher refuses: nothing was launched then
        self._inst_collect()
        self._launched = True

    def rc(self, op, args):
        """call() for tests of the refusals: the entry point's return code instead of an exception"""
        for tensor in getattr(args, "_keep", ()):
            self._guarded_ptr(tensor)
        self._inst_begin()
        code = self.lib.fn[op](ctypes.byref(args), self.stream())
        if code == 0:
            self._inst_collect()
        self._launched = self._launched or code == 0
        return code

    def call_raw(self, op, jobs, *args):
        """call() for the entry points that take a device-resident job table and counts instead of an argument struct
        (mds_pack_weights, mds_bn_eval_table).  jobs: the host struct or ctypes array of structs; every pointer field of every job
        must be null or an address inside a guarded buffer - checked here, as call() checks its tensors.  The table is copied into a
        guarded buffer of its own; the stream is appended to `args`."""
        for j, job in enumerate(jobs if isinstance(jobs, ctypes.Array) else [jobs]):
            for name, ctype in job._fields_:
                addr = getattr(job, name) if ctype is ctypes.c_void_p else None
                if addr:
                    rec = next((r for r in self._known.values() if r.view() is not None and r.lo <= addr < r.hi), None)
                    if rec is None:
                        raise AssertionError(f"job {j}: field '{name}' is no address inside a guarded buffer: allocate it with be.t() / be.out() and pass be.ptr()")
                    if not any(r is rec for r, _ in self._pending):
                        self._pending.append((rec, rec.view()))
        table = self.t(torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8))
        self._inst_begin()
        self.lib.check(self.lib.fn[op](self._guarded_ptr(table), *args, self.stream()), op)
        self._inst_collect()
        self._launched = True

    def _inst_begin(self):
        if self.name == "emu":
            from hipemu.loader import inst_begin
            inst_begin()

    def _inst_collect(self):
        """simulator only: what the successful call just launched joins KERNEL_TEST_INSTANTIATIONS"""
        if self.name == "emu":
            from hipemu.loader import inst_seen
            KERNEL_TEST_INSTANTIATIONS.update(inst_seen())

    def sync(self):
        """synchronise, then compare every guard registered (or launched on) since the last verification with its pattern"""
        if self.name != "emu":
            torch.cuda.synchronize()
        pending, self._pending, self._launched = self._pending, [], False
        self._known = {p: r for p, r in self._known.items() if r.view() is not None}
        if not pending:
            return
        # the compare runs where the buffers live; one scalar comes back, and on a hit one index
        if int(torch.stack([c for rec, _ in pending for c in rec.counts()]).sum()) == 0:
            return
        for rec, _ in pending:
            hit = rec.first_bad()
            if hit is not None:
                side, offset = hit
                what = "store into the guard of input" if rec.kind == "t" else "stray store or accumulate next to output"
                raise AssertionError(f"guard band: {what} '{rec.name}', {side} the payload, first changed byte at offset {offset:+d} "
                                     f"from the payload's {'start' if side == 'before' else 'end'} ({rec.nbytes} payload bytes)")

    def finish(self):
        """fixture teardown: verify what is left; a launch nobody verified fails the test"""
        launched = self._launched
        self.sync()
        assert not launched, "a launch was left unverified: call be.sync() after the last be.call() of the test"

    def launches(self, name=None):
        """simulator only: the launches since the last knobs() entry / reset_launches(), optionally those whose kernel expression
        contains `name`; None on the GPU (the same host routing code runs there, but nothing records it)"""
        if self.name != "emu":
            return None
        from hipemu.loader import launches
        return [l for l in launches() if name is None or name in l.kernel]

    def reset_launches(self):
        if self.name == "emu":
            from hipemu.loader import reset_launches
            reset_launches()


@contextlib.contextmanager
def knobs(be, values):
    """developer knobs ({MDS_KNOB_*: value}) for the body of a `with`; every one is back at 0 afterwards, also when the body
    raises - the knobs are process-global per library, and a failing test must not leak them into the next.  Clears the
    simulator's launch record on entry, so that be.launches() inside the body sees the body's launches only."""
    be.reset_launches()
    try:
        for k, v in values.items():
            be.lib.check(be.lib.fn["dev_set"](k, v), "dev_set")
        yield
    finally:
        for k in values:
            be.lib.fn["dev_set"](k, 0)


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
_cache = {}


@pytest.fixture(params=BACKENDS)
def be(request):
    name = request.param
    if name not in _cache:
        _cache[name] = Backend(name)
    yield _cache[name]
    _cache[name].finish()


@pytest.fixture
def be_gpu():
    """the gfx950 library only: for tests that never run on the simulator (it is then not even built on the GPU box)"""
    if "gpu" not in _cache:
        _cache["gpu"] = Backend("gpu")
    yield _cache["gpu"]
    _cache["gpu"].finish()


DT = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16)}


def tol(dt):
    return dict(rtol=2e-4, atol=2e-5) if dt == "f32" else dict(rtol=2e-2, atol=2e-2)


def assert_close(got, want, dt, scale=1.0, msg=""):
    """elementwise outputs (y, dx, g, out, dy, da): their error is the store's rounding.  A sum over rows, pixels or groups is NOT
    checked here: a tolerance that grows with the size of the sum (scale = sqrt(count), 20, 10 ...) on top of max|want|, which
    grows with it too, lets a bf16 sum with a whole image missing pass - such quantities go to assert_sum_close."""
    assert scale <= 4, (f"{msg}: assert_close(scale={scale:.3g}) - a size-scaled tolerance is refused; a quantity that is a sum is "
                        f"checked by assert_sum_close (float64 reference of the same operands + the fp32 summation bound)")
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    t = tol(dt)
    err = (got - want).abs()
    bound = t["atol"] * scale * max(1.0, want.abs().max().item()) + t["rtol"] * want.abs()
    bad = ~(err <= bound)       # (not `err > bound`: a NaN result - a consumed over-read of a NaN guard - compares False both ways)
    assert not bad.any(), (f"{msg}: {int(bad.sum())}/{bad.numel()} mismatches, max err {err.max().item():.3e} "
                           f"(ref max {want.abs().max().item():.3e}) first bad idx {bad.nonzero()[0].tolist()}")


# ------------------------------------------------------------------------------------------------ sums: a derived bound
U = 2.0 ** -23        # one fp32 ulp (twice the unit roundoff: the bound also holds for adders that truncate)
SUM_OBSERVERS = []    # callables (msg, worst err / bound) a measuring run may register (profiles/LOG.md's table); empty in the suite
ABS = 1.0 / U         # `chain` of a part whose `mag` already IS an absolute error bound: (ABS + 8) * U * mag = mag (1 + 1e-6)


def assert_sum_close(got, want, parts, msg, probes=(), cap=None):
    """a kernel output that is an fp32 (then fp64) SUM of values the kernel holds exactly, against `want`: the float64 evaluation of
    the same sum over the same operands (inputs rounded to the storage type, activations rounded where the kernel rounds them).

    parts: [(chain, mag), ...] - mag: float64, shaped like want, the same computation on absolute values; chain: the number of fp32
    additions on the longest path into one output element.  bound = U * sum_i (chain_i + 8) * mag_i, U = 2^-23: the a-priori bound
    of a sum of chain_i terms taken in ANY order ((n - 1) u sum|t| to first order, u = 2^-24), with u doubled so that it holds for
    a matrix unit whose adders truncate; + 8 for the few fp32 roundings inside one term (a product, (y - mu) * rstd, a mask
    factor).  Neither figure is fitted to results.  A part (ABS, mag) adds mag itself: the error of operands the kernel computes
    (pro_operand below).

    cap = (dt, scale): the bound that assert_close(dt, scale) applied to this quantity before; the smaller of the two holds for
    every element, so nothing is checked more loosely than it was.

    probes: [(name, wrong answer built from the reference alone), ...] - the bound must still tell each of them from `want`: out
    of bound in at least half of the elements the probe changes.  A probe that changes nothing fails.  NaN in `got` fails."""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, f"{msg}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bound = torch.zeros_like(want)
    for chain, mag in parts:
        mag = mag.detach().double().cpu()
        assert mag.shape == want.shape and bool((mag >= 0).all()), f"{msg}: a part's magnitude is shaped like the result and non-negative"
        bound = bound + (chain + 8.0) * U * mag
    if cap is not None:
        t = tol(cap[0])
        bound = torch.minimum(bound, t["atol"] * cap[1] * max(1.0, want.abs().max().item()) + t["rtol"] * want.abs())
    for name, wrong in probes:
        wrong = wrong.detach().double().cpu()
        changed = wrong != want
        assert changed.any(), f"{msg}: probe '{name}' equals the reference: it probes nothing"
        seen = ((wrong - want).abs() > bound) & changed
        assert 2 * int(seen.sum()) >= int(changed.sum()), (f"{msg}: the bound does not resolve probe '{name}': out of bound in "
                                                          f"{int(seen.sum())} of the {int(changed.sum())} elements it changes")
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf"))
    for seen_by in SUM_OBSERVERS:
        seen_by(msg, float(ratio.max()) if ratio.numel() else 0.0)
    bad = ~(err <= bound)       # (a NaN result compares False both ways)
    assert not bad.any(), (f"{msg}: {int(bad.sum())}/{bad.numel()} sums out of bound, worst err / bound {ratio.max().item():.3e}, max err "
                           f"{err.max().item():.3e} (ref max {want.abs().max().item():.3e}) first bad idx {bad.nonzero()[0].tolist()}")


def bf16_ulp(a):
    """distance between the two bf16 numbers around a (float64): 2^(floor(log2|a|) - 7); 0 at 0"""
    _, e = torch.frexp(a.abs())                     # |a| = m * 2^e, m in [0.5, 1)
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), e - 8))


def near_tie(a, delta):
    """elements of float64 `a` within relative distance `delta` (a tensor or a number) of a boundary between two bf16 roundings (the
    midpoint of two neighbouring bf16 numbers): a kernel whose fp32 evaluation of a is off by delta may round it the other way"""
    m, _ = torch.frexp(a.abs())
    t = m * 256.0                                   # in [128, 256): the integers are the bf16 numbers, the ties sit at k + 1/2
    return ((t - torch.floor(t) - 0.5).abs() <= delta * t) & (a != 0)


def pro_operand(z, zmag, silu, dt, roundings=0, factor=None):
    """the operand a kernel FORMS from a stored x: a = act(z) (* factor), z = x * scale + shift, as float64 reference and error bound.
    z: float64; zmag = |x * scale| + |shift|; silu: False = affine only; factor: the squeeze-excite gate (one more product).
    Returns (a, err): for bf16, a is rounded to bf16 (round to nearest even, as the kernels' conversion) and err is one bf16 ulp on
    the NEAR-TIE elements - those within relative distance delta of a rounding boundary, where the kernel's fp32 value may fall on
    the other side - and 0 elsewhere; for f32, a is not rounded and err = delta * |a|.  delta, per element, from the kernel's
    arithmetic (csrc/platform.h: silu(z) = z * rcp(1 + exp2(-z * log2(e)))) and the accuracy the CDNA ISA guide documents for
    v_exp_f32 and v_rcp_f32, 1 ulp each:
      z itself: two fp32 roundings (or one fused), |dz| <= U * zmag, which moves silu(z) by |dz * silu'(z)|;
      the exponent's argument: product and constant rounded, relative U, i.e. |z| U on exp2's result; exp2: U; 1 + e: U / 2;
      rcp: U; the product with z: U / 2; `roundings` more for later factors: (|z| + 4 + roundings) U in all.
    (An issue-style part (2^-8 / U, mag on the ties) would take 2^-8 |a| for the flip; the exact ulp is between 1 and 2 times that.)"""
    if silu:
        s = torch.sigmoid(z)
        a = z * s
        da = U * zmag * (s * (1 + z * (1 - s))).abs() + (z.abs() + 4 + roundings) * U * a.abs()
    else:
        a = z
        da = U * zmag + roundings * U * a.abs()
    if factor is not None:
        a, da = a * factor, da * factor.abs() + U * (a * factor).abs()
    if dt != "bf16":
        return a, da
    tie = near_tie(a, da / a.abs().clamp_min(1e-300))
    aq = a.to(torch.bfloat16).double()
    return aq, torch.where(tie, bf16_ulp(a), torch.zeros_like(a))


def stat_parts(v, vabs, K, cnt, verr=None):
    """forward statistics of a GEMM / convolution with inner length K over cnt pixels, reduced over every dimension but the last.
    v: float64 values the kernel sums (its fp32 accumulators, + residual where the kernel adds one first), vabs: the same product on
    absolute values, verr: the product of the operand's error (pro_operand) with |w|.  Returns {"sum": (want, parts), "sumsq": ...}"""
    red = tuple(range(v.dim() - 1))
    sq = (v * v).sum(red)
    ps = [(K, vabs.sum(red)), (cnt, v.abs().sum(red))]
    pq = [(2 * K + 2, (vabs * vabs).sum(red)), (cnt, sq)]
    if verr is not None:
        ps.append((ABS, verr.sum(red)))
        pq.append((ABS, (2 * vabs * verr + verr * verr).sum(red)))
    return {"sum": (v.sum(red), ps), "sumsq": (sq, pq)}


def assert_post_close(s, g, xhat, xmag, cap, probes=(), msg="", gerr=None):
    """the backward sums of a BatchNorm, s[0] = sum g and s[1] = sum g * xhat over every dimension but the last.  g: float64, the
    values the kernel sums; xhat = (y - mean) * rstd and xmag = (|y| + |mean|) * rstd in float64, from the kernel's fp32 tables or
    from the float64 statistics those tables round (2^-24 of |mean| rstd and of rstd: inside the + 8 on xmag);
    gerr: bound of g's own error where the kernel forms g; probes: [(name, f)], f(t) = the rows a wrong kernel would have summed"""
    red = tuple(range(g.dim() - 1))
    cnt = g[..., 0].numel()
    p0, p1 = [(cnt, g.abs().sum(red))], [(cnt, (g.abs() * xmag).sum(red))]
    if gerr is not None:
        p0.append((ABS, gerr.sum(red))); p1.append((ABS, (gerr * xmag).sum(red)))
    assert_sum_close(s[0], g.sum(red), p0, msg + "sum g", [(n, f(g).sum(red)) for n, f in probes], cap)
    assert_sum_close(s[1], (g * xhat).sum(red), p1, msg + "sum g*xhat", [(n, (f(g) * f(xhat)).sum(red)) for n, f in probes], cap)


def assert_stats_close(s, v, vabs, K, cnt, cap, verr=None, probes=(), msg=""):
    """s[0] / s[1]: a kernel's sum / sum of squares; probes: [(name, f)] with f(v) = the values a wrong kernel would have summed"""
    for i, (key, (want, parts)) in enumerate(stat_parts(v, vabs, K, cnt, verr).items()):
        red = tuple(range(v.dim() - 1))
        pr = [(n, f(v).sum(red) if i == 0 else (f(v) ** 2).sum(red)) for n, f in probes]
        assert_sum_close(s[i], want, parts, f"{msg}{key}", pr, cap)
