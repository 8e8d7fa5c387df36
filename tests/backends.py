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
        self.lib.call(op, args, self.stream())      # raises when the launcher refuses: nothing was launched then
        self._launched = True

    def rc(self, op, args):
        """call() for tests of the refusals: the entry point's return code instead of an exception"""
        for tensor in getattr(args, "_keep", ()):
            self._guarded_ptr(tensor)
        code = self.lib.fn[op](ctypes.byref(args), self.stream())
        self._launched = self._launched or code == 0
        return code

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
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    t = tol(dt)
    err = (got - want).abs()
    bound = t["atol"] * scale * max(1.0, want.abs().max().item()) + t["rtol"] * want.abs()
    bad = ~(err <= bound)       # (not `err > bound`: a NaN result - a consumed over-read of a NaN guard - compares False both ways)
    assert not bad.any(), (f"{msg}: {int(bad.sum())}/{bad.numel()} mismatches, max err {err.max().item():.3e} "
                           f"(ref max {want.abs().max().item():.3e}) first bad idx {bad.nonzero()[0].tolist()}")
