"""The fixed-order way out of the kernels that end in fp32 atomics (mds_partial_t + mds_wgrad_finish, include/mds.h): ABI, and
every affected entry point through the per-family tests of the atomic form - same inputs, same float64 / autograd references,
same assert_close / tol - with the partial buffer set.

`DetBackend` stands in for the `be` fixture of those tests.  For every launch of an affected entry point it
  1. runs the atomic form on a snapshot of the launch's tensors and keeps its result,
  2. runs the partial + finish form into a gradient buffer that holds random values beforehand (the finish accumulates):
     result - those values must agree with step 3's to the family's tolerance,
  3. runs the partial + finish form on the restored tensors - the result the calling test then checks against its reference -
     and compares it with the atomic result at the same tolerance (only the summation order differs),
  4. on the GPU: runs it twice more into fresh buffers - torch.equal, bit for bit.
The partial buffer is filled with NaN before every launch: a slot element that a launch leaves unwritten poisons the result."""
import ctypes as C

import pytest
import torch

import test_k_conv
import test_k_dw_stem
import test_k_elem
import test_k_pw
from backends import BACKENDS, Backend, assert_close, assert_sum_close, _cache
from mds import cabi

RESULT = {"pw_wgrad": "dw", "conv_wgrad": "dw", "stem_wgrad": "dw", "dw_bwd": "dw", "gem_bwd": "dp", "focal_fwd_bwd": "loss"}
NAMES = {0: "f32", 1: "bf16"}


class DetBackend:
    def __init__(self, be):
        self.be, self.name, self.lib, self.device = be, be.name, be.lib, be.device
        self.launches = []          # (op, slots floats) of every deterministic launch made through this backend

    stream = lambda self: self.be.stream()
    sync = lambda self: self.be.sync()
    t = lambda self, x, dtype=None, **kw: self.be.t(x, dtype, **kw)
    out = lambda self, *a, **kw: self.be.out(*a, **kw)
    ptr = lambda self, t: self.be.ptr(t)
    rc = lambda self, op, args: self.be.rc(op, args)

    def call(self, op, args):
        if op not in RESULT:
            return self.be.call(op, args)
        need = int(self.lib.fn[op + "_partial_floats"](C.byref(args)))
        assert need >= 0, self.lib.dll.mds_last_error()
        if need == 0:               # (the loss of <= 256 elements: one block, no buffer)
            return self.be.call(op, args)
        tensors = {t.data_ptr(): t for t in getattr(args, "_keep", ())}
        res = tensors[getattr(args, RESULT[op])].detach()
        dt = NAMES[getattr(args, "dtype", 0)]
        saved = {p: t.detach().clone() for p, t in tensors.items()}

        def restore():
            for p, t in tensors.items():
                t.detach().copy_(saved[p])

        keep = list(args._keep)

        def det():
            part = self.be.out(need, torch.float32, float("nan"))
            args.partial = cabi.make("mds_partial_t", buf=part, floats=need)
            args._keep = keep + [part]                   # (assigned after cabi.make: be.call must see the slots too)
            self.be.call(op, args)
            self.be.sync()
            args.partial = cabi.make("mds_partial_t", buf=None, floats=0)
            args._keep = keep
            return res.clone()

        self.be.call(op, args)                      # 1. atomics
        self.be.sync()
        atomic = res.clone() - saved[res.data_ptr()]
        restore()
        before = torch.randn(res.shape, generator=torch.Generator().manual_seed(7)).to(self.device)
        res.detach().copy_(before)                           # 2. a gradient buffer that is not zero beforehand
        accumulated = det() - before
        restore()
        got = det()                                 # 3. what the calling test checks against its reference
        first = got - saved[res.data_ptr()]
        assert torch.isfinite(got).all(), f"{op}: a slot was left unwritten"
        assert_close(first, atomic, dt, msg=f"{op}: partial + finish against the atomic form")
        # (the add into the buffer and the subtraction above: two fp32 roundings of |before| + |result| - within the helper's + 8)
        assert_sum_close(accumulated, first, [(0, before.abs() + first.abs())], f"{op}: finish into a non-zero gradient buffer",
                         cap=(dt, 1.0 + before.abs().max().item()))
        if self.name == "gpu":                      # 4. bit-identical reruns
            for k in range(2):
                restore()
                assert torch.equal(det(), got), f"{op}: run {k + 2} differs from run 1"
        self.launches.append((op, need))


@pytest.fixture(params=BACKENDS)
def det(request):
    name = request.param
    if name not in _cache:
        _cache[name] = Backend(name)
    yield DetBackend(_cache[name])
    _cache[name].finish()


@pytest.fixture
def det_gpu():
    if "gpu" not in _cache:
        _cache["gpu"] = Backend("gpu")
    yield DetBackend(_cache["gpu"])
    _cache["gpu"].finish()


@pytest.fixture
def emu():
    """the simulator's backend for the tests below that never run on the GPU: guarded buffers, verified on teardown"""
    if "emu" not in _cache:
        _cache["emu"] = Backend("emu")
    yield _cache["emu"]
    _cache["emu"].finish()


def cases(fn, *more):
    """the parameter sets of an existing parametrised test (outermost decorator last), as one list of tuples, + extra cases"""
    import itertools
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    lists = []
    for m in reversed(marks):       # pytestmark lists the decorator nearest the function first; the signature's order is the reverse
        n = len([a for a in m.args[0].split(",")])
        lists.append([tuple(v) if n > 1 else (v,) for v in m.args[1]])
    out = [sum(c, ()) for c in itertools.product(*lists)]
    return out + list(more)


# ---------------------------------------------------------------------------------------------------------------- ABI (no GPU)
def test_abi_declares_and_exports_the_deterministic_way_out():
    from hipemu.loader import load_emulator
    lib = load_emulator()
    assert not lib.missing
    assert "mds_partial_t" in cabi.STRUCTS and "mds_wgrad_finish_args" in cabi.STRUCTS and "wgrad_finish" in lib.fn
    for op, struct in (("pw_wgrad", "mds_pw_wgrad_args"), ("conv_wgrad", "mds_conv_wgrad_args"), ("stem_wgrad", "mds_stem_wgrad_args"),
                       ("dw_bwd", "mds_dw_bwd_args"), ("gem_bwd", "mds_gem_bwd_args"), ("focal_fwd_bwd", "mds_focal_args")):
        assert op + "_partial_floats" in lib.fn, op
        assert dict(cabi.STRUCTS[struct]._fields_)["partial"] is cabi.STRUCTS["mds_partial_t"], struct
    assert cabi.MDS_VERSION >= 136 and lib.dll.mds_version() == cabi.MDS_VERSION
    hip = cabi.Lib(cabi.HIP_LIB)          # the gfx950 library exports them too (dlopen + symbol check needs no GPU)
    assert not hip.missing and "wgrad_finish" in hip.fn


def _check_pw_dw(dw, x, dy, M, dt):
    """dw = dy^T x over M rows against float64 on the stored operands; probes: the ragged last 64 rows left out, 16 rows taken twice"""
    x64, d64, r = x.double().cpu(), dy.double().cpu(), M % 64 or 64
    probes = [(f"last {r} rows left out", d64[:-r].t() @ x64[:-r]), ("first 16 rows counted twice", d64.t() @ x64 + d64[:16].t() @ x64[:16])]
    assert_sum_close(dw, d64.t() @ x64, [(M, d64.abs().t() @ x64.abs())], "dw", probes, cap=(dt, M ** 0.5))


def test_undersized_or_misaligned_partial_buffer_is_a_bad_argument(emu):
    lib = emu.lib
    M, K, N = 700, 40, 72
    x, dy, dw = emu.t(torch.randn(M, K)), emu.t(torch.randn(M, N)), emu.out((N, K), torch.float32, 0)
    args = cabi.make("mds_pw_wgrad_args", dtype=0, M=M, K=K, N=N, x=x, dy=dy, dw=dw, pro=cabi.pro(0))
    need = lib.fn["pw_wgrad_partial_floats"](C.byref(args))
    assert need >= N * K
    part = emu.out(need + 4, torch.float32, 0)
    args._keep = args._keep + [part]
    args.partial = cabi.make("mds_partial_t", buf=part, floats=need - 1)
    assert emu.rc("pw_wgrad", args) == cabi.MDS_ERR_BAD_ARG and b"partial" in lib.dll.mds_last_error()
    assert torch.equal(dw, torch.zeros(N, K)), "a refused launch wrote the gradient"
    args.partial = cabi.make("mds_partial_t", buf=part[1:], floats=need)
    assert emu.rc("pw_wgrad", args) == cabi.MDS_ERR_BAD_ARG
    args.partial = cabi.make("mds_partial_t", buf=part, floats=need)
    assert emu.rc("pw_wgrad", args) == 0
    emu.sync()
    _check_pw_dw(dw, x, dy, M, "f32")
    # the query reads dims only: a struct without buffers gives the same answer
    bare = cabi.make("mds_pw_wgrad_args", dtype=0, M=M, K=K, N=N, pro=cabi.pro(0))
    assert lib.fn["pw_wgrad_partial_floats"](C.byref(bare)) == need


def test_wgrad_finish_adds_the_slots_in_slot_order(emu):
    """mds_wgrad_finish on its own, against the order its header comment states: G contiguous slot ranges (G from the result's
    size), each summed first to last, the range sums added first to last, the total added to the destination - bit for bit,
    aligned and unaligned, in all three size classes, with fewer slots than ranges and with ranges of unequal length"""
    g = torch.Generator().manual_seed(5)
    for numel, slots, off in ((1, 7, 0), (1, 200, 0), (1030, 9, 0), (1030, 2, 1), (516, 13, 0), (27 * 32, 1, 3), (864, 768, 0), (672 * 9, 131, 0),
                               (4096, 37, 0), (5000, 70, 1), (65536, 5, 0), (65540, 9, 3)):
        stride = (numel + 3) // 4 * 4
        part = (torch.randn(slots, stride, generator=g) * 10 ** torch.randint(-3, 4, (slots, 1), generator=g).float()).contiguous()
        base = torch.randn(numel + off, generator=g)
        dst = emu.out(numel + off, torch.float32, base)
        a = cabi.make("mds_wgrad_finish_args", partial=emu.t(part), dst=dst[off:], numel=numel, slots=slots, slot_stride=stride)
        assert emu.rc("wgrad_finish", a) == 0, emu.lib.dll.mds_last_error()
        emu.sync()
        G = cabi.MDS_FINISH_GROUPS if numel >= cabi.MDS_FINISH_WIDE else cabi.MDS_FINISH_GROUPS_MID if numel >= cabi.MDS_FINISH_MID else cabi.MDS_FINISH_GROUPS_SMALL
        per = -(-slots // G)
        total = None
        for gi in range(G):
            s = torch.zeros(numel)
            for k in range(gi * per, min((gi + 1) * per, slots)):
                s = s + part[k, :numel]
            total = s if total is None else total + s
        assert torch.equal(dst[off:], base[off:] + total), (numel, slots, off)
        assert torch.equal(dst[:off], base[:off])


# ---------------------------------------------------------------------------------------------------------------- families
# ragged extras: M not a multiple of the rows per block (bf16: 8 row splits are launched for 4 real ones - four blocks return
# early), K / N tile edges
@pytest.mark.parametrize("dt,M,K,N,mode", cases(test_k_pw.test_pw_wgrad, ("bf16", 1000, 40, 72, 0), ("f32", 1000, 40, 72, 2), ("bf16", 4100, 136, 200, 3)))
def test_pw_wgrad(det, dt, M, K, N, mode):
    test_k_pw.test_pw_wgrad(det, dt, M, K, N, mode)
    assert [op for op, _ in det.launches] == ["pw_wgrad"]


# ragged extras (k_conv.hip's kernel): odd extents - the last tile of every row and column is partial -, a tile count that does not
# divide by the tiles per block, stride 2 with TF-SAME padding on an odd image, Cout = 16 (one of four fragments of the channel tile)
RAGGED_CONV = [("f32", 3, 19, 27, 16, 16, 1, 0), ("bf16", 3, 19, 27, 48, 80, 1, 2), ("f32", 2, 21, 35, 32, 48, 2, 1)]


@pytest.mark.parametrize("dt,N,H,W,Cin,Cout,stride,mode", cases(test_k_conv.test_conv_wgrad, *RAGGED_CONV))
def test_conv_wgrad(det, dt, N, H, W, Cin, Cout, stride, mode):
    test_k_conv.test_conv_wgrad(det, dt, N, H, W, Cin, Cout, stride, mode)
    assert [op for op, _ in det.launches] == ["conv_wgrad"]


# ragged extras (k_c3.hip): a block cap far above the item count (the grid is the item count: no block without a slot's worth of
# work, no slot without a block), a band of 5 of 32 columns, a cap that leaves the last block one item short
RAGGED_C3W = [(1, 2, 37, 32, 128, 64), (2, 7, 69, 48, 192, 5), (3, 5, 33, 32, 128, 4)]


@pytest.mark.parametrize("N,H,W,Cin,Cout,blocks", cases(test_k_conv.test_c3w_weight_gradient_row_streaming, *RAGGED_C3W))
def test_c3w_row_streaming(det, N, H, W, Cin, Cout, blocks):
    test_k_conv.test_c3w_weight_gradient_row_streaming(det, N, H, W, Cin, Cout, blocks)
    assert len(det.launches) == 1


@pytest.mark.parametrize("N,H,W,blocks", cases(test_k_conv.test_c3w_weight_gradient_behind_the_prologue, (1, 2, 70, 64), (3, 5, 130, 4)))
def test_c3wp_behind_the_prologue(det, N, H, W, blocks):
    test_k_conv.test_c3w_weight_gradient_behind_the_prologue(det, N, H, W, blocks)
    assert len(det.launches) == 1


@pytest.mark.parametrize("N,H,W,blocks", cases(test_k_conv.test_c3w2_stride2_weight_gradient, (1, 2, 38, 64), (3, 6, 70, 4)))
def test_c3w2_stride2(det, N, H, W, blocks):
    test_k_conv.test_c3w2_stride2_weight_gradient(det, N, H, W, blocks)
    assert len(det.launches) == 1


def test_ablation_switches_are_refused_not_composed(emu):
    """MDS_KNOB_WG_DBG's ablation bits skip the kernel's sums or stores: with a partial buffer that would leave slots unwritten, so
    the launch is a clear error (the atomic path keeps its meaning: measurement only)"""
    lib = emu.lib
    M, K, N = 600, 32, 64
    x, dy, dw = emu.t(torch.randn(M, K).bfloat16()), emu.t(torch.randn(M, N).bfloat16()), emu.out((N, K), torch.float32, 0)
    args = cabi.make("mds_pw_wgrad_args", dtype=1, M=M, K=K, N=N, x=x, dy=dy, dw=dw, pro=cabi.pro(0))
    need = lib.fn["pw_wgrad_partial_floats"](C.byref(args))
    part = emu.out(need, torch.float32, float("nan"))
    args.partial = cabi.make("mds_partial_t", buf=part, floats=need)
    args._keep = args._keep + [part]
    try:
        for bits in (1, 2, 4):
            lib.check(lib.fn["dev_set"](cabi.MDS_KNOB_WG_DBG, bits), "dev_set")
            assert emu.rc("pw_wgrad", args) == cabi.MDS_ERR_BAD_ARG and b"WG_DBG" in lib.dll.mds_last_error()
            assert torch.equal(dw, torch.zeros(N, K))
        lib.check(lib.fn["dev_set"](cabi.MDS_KNOB_WG_DBG, 32), "dev_set")      # (not an ablation: row splits not rounded to 8 - composes)
        assert emu.rc("pw_wgrad", args) == 0
        emu.sync()
    finally:
        lib.fn["dev_set"](cabi.MDS_KNOB_WG_DBG, 0)
    _check_pw_dw(dw, x, dy, M, "bf16")


def test_c3w_query_follows_the_route_and_the_block_knob(det):
    """the slot count is the launch's grid.x: it moves with MDS_KNOB_CONV_BLOCKS and with the route (k_c3.hip / k_conv.hip)"""
    lib = det.lib
    dy, dx, wi = test_k_conv.geo.taps_fwd(1, 1)
    mk = lambda dtype: cabi.make("mds_conv_wgrad_args", dtype=dtype, N=2, IH=24, IW=64, Cin=32, OH=24, OW=64, Cout=128, **{"is": 1}, ntaps=9,
                                 dy=dy, dx=dx, wi=wi, wtaps=9, pro=cabi.pro(0))
    numel, got = 128 * 32 * 9, {}
    try:
        lib.check(lib.fn["dev_set"](cabi.MDS_KNOB_C3, 2), "dev_set")
        for blocks in (1, 3):
            lib.check(lib.fn["dev_set"](cabi.MDS_KNOB_CONV_BLOCKS, blocks), "dev_set")
            got[blocks] = lib.fn["conv_wgrad_partial_floats"](C.byref(mk(1)))
    finally:
        lib.fn["dev_set"](cabi.MDS_KNOB_C3, 0)
        lib.fn["dev_set"](cabi.MDS_KNOB_CONV_BLOCKS, 0)
    assert got == {1: numel, 3: 3 * numel}
    assert lib.fn["conv_wgrad_partial_floats"](C.byref(mk(0))) % numel == 0


# ragged extras: C not a multiple of the 64- (32-) channel chunk, odd H and W (a partial last band and strip; 8 strips per block do
# not divide the strip count: the last block's spare strips skip their work and still flush), all four kernels: 3x3 stride 1,
# stride 2 on odd and even extents (both TF-SAME pads), 3x3x3 at T = 5 (sliding window) and at T = 3 (tiled kernel, tile edges)
RAGGED_DW = [("bf16", 1, 1, 13, 19, 72, 1, 1), ("f32", 3, 1, 7, 11, 40, 1, 1), ("bf16", 1, 1, 13, 19, 72, 2, 1), ("f32", 2, 1, 10, 18, 40, 2, 1),
             ("bf16", 1, 5, 5, 7, 72, 1, 3), ("f32", 1, 3, 9, 19, 40, 1, 3), ("bf16", 2, 3, 9, 35, 72, 1, 3)]


@pytest.mark.parametrize("dt,N,T,H,W,C,stride,kt", cases(test_k_dw_stem.test_dw_fwd_bwd, *RAGGED_DW))
def test_dw_bwd(det, dt, N, T, H, W, C, stride, kt):
    test_k_dw_stem.test_dw_fwd_bwd(det, dt, N, T, H, W, C, stride, kt)
    assert [op for op, _ in det.launches] == ["dw_bwd"]


# ragged extras: OW = 35 / 11 (not a multiple of the 32-column tile / group), odd H (TF-SAME pad on one side), a tile count that the
# tiles per block do not divide; fp32: fewer pixel groups than waves in the last block (waves without work store zeros)
RAGGED_STEM = [("bf16", 3, 27, 70), ("f32", 3, 27, 70), ("bf16", 1, 9, 22), ("f32", 1, 5, 22)]


@pytest.mark.parametrize("dt,N,H,W", cases(test_k_dw_stem.test_stem_fwd_wgrad, *RAGGED_STEM))
def test_stem_wgrad(det, dt, N, H, W):
    test_k_dw_stem.test_stem_fwd_wgrad(det, dt, N, H, W)
    assert [op for op, _ in det.launches] == ["stem_wgrad"]


@pytest.mark.parametrize("gmode,N,H,W", cases(test_k_dw_stem.test_stem_wgrad_forms_dy_on_load))
def test_stem_wgrad_dy_on_load(det, gmode, N, H, W):
    test_k_dw_stem.test_stem_wgrad_forms_dy_on_load(det, gmode, N, H, W)
    assert "stem_wgrad" in [op for op, _ in det.launches]


@pytest.mark.parametrize("dt,pro_mode,split,R_,C", cases(test_k_elem.test_gem_fwd_bwd, ("f32", 2, True, 77, 24), ("bf16", 2, False, 3, 8), ("bf16", 2, True, 1031, 40)))
def test_gem_bwd(det, golden, dt, pro_mode, split, R_, C):
    test_k_elem.test_gem_fwd_bwd(det, dt, pro_mode, split, R_, C, golden)
    assert [op for op, _ in det.launches] == ["gem_bwd"]


def test_focal_loss_over_several_blocks(det):
    """2000 elements = 8 blocks add to the loss value: through slots, in block order; against float64"""
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(2000, generator=g) * 3, (torch.rand(2000, generator=g) > 0.7).float()
    loss, dx = det.out(1, torch.float32, 0), det.out(2000, torch.float32, float("nan"))
    args = cabi.make("mds_focal_args", n=2000, x=det.t(x), t=det.t(t), alpha=-1.0, gamma=1.2, reduction=cabi.MDS_REDUCE_MEAN, loss=loss, dx=dx)
    det.call("focal_fwd_bwd", args)
    assert det.launches == [("focal_fwd_bwd", 32)]
    xd, td = x.double(), t.double()
    p = torch.sigmoid(xd)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(xd, td, reduction="none")
    want = (ce * (1 - (p * td + (1 - p) * (1 - td))) ** 1.2).mean()
    assert_close(loss, want.float().view(1), "f32")


# ---------------------------------------------------------------------------------------------------------------- config 2's own layer sizes
@pytest.mark.gpu
@pytest.mark.parametrize("H,W,Cin,Cout,stride,mode", test_k_conv.TRAIN_LAYERS)
def test_conv_wgrad_at_the_training_sizes(det_gpu, H, W, Cin, Cout, stride, mode):
    """the 3x3 layers of the benchmarked step (20 images) through the existing k_c3.hip-against-k_conv.hip test: both routes' weight
    gradients take the deterministic way out (blocks.2.1: 256 slots of 82 944 floats)"""
    test_k_conv.test_k_c3_at_the_training_sizes_against_k_conv(det_gpu, H, W, Cin, Cout, stride, mode)
    assert [op for op, _ in det_gpu.launches] == ["conv_wgrad", "conv_wgrad"]


PW_TRAIN_LAYERS = [  # 1x1 layers of the benchmarked step (20 images / 4 stacks): M, K, N, prologue
    (20 * 184 * 320, 128, 32, 2),      # blocks.1.1 projection (edge residual)
    (20 * 92 * 160, 192, 48, 2),       # blocks.2.1 projection
    (20 * 46 * 80, 48, 192, 0),        # blocks.3.0 expansion
    (20 * 46 * 80, 384, 96, 3),        # blocks.3.1 projection behind the squeeze-excite gate
    (20 * 23 * 40, 672, 112, 3),       # blocks.4.x projection
    (20 * 23 * 40, 112, 192, 0),       # conv2d_projection
    (20 * 23 * 40, 192, 576, 0),       # 3D block expansion
    (20 * 23 * 40, 576, 192, 3),       # 3D block projection
]


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,mode", PW_TRAIN_LAYERS)
def test_pw_wgrad_at_the_training_sizes(det_gpu, M, K, N, mode):
    test_k_pw.test_pw_wgrad(det_gpu, "bf16", M, K, N, mode)
    assert [op for op, _ in det_gpu.launches] == ["pw_wgrad"]


DW_TRAIN_LAYERS = [  # depthwise layers of the benchmarked step: N, T, H, W, C, stride, kt
    (20, 1, 92, 160, 192, 2, 1),       # blocks.3.0
    (20, 1, 46, 80, 384, 1, 1),        # blocks.3.1
    (20, 1, 46, 80, 576, 2, 1),        # blocks.5.0's shape class (stride 2)
    (20, 1, 23, 40, 672, 1, 1),        # blocks.4.x
    (4, 5, 23, 40, 576, 1, 3),         # the 3D blocks (T = 5 stacks)
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,H,W,C,stride,kt", DW_TRAIN_LAYERS)
def test_dw_bwd_at_the_training_sizes(det_gpu, N, T, H, W, C, stride, kt):
    test_k_dw_stem.test_dw_fwd_bwd(det_gpu, "bf16", N, T, H, W, C, stride, kt)
    assert [op for op, _ in det_gpu.launches] == ["dw_bwd"]


@pytest.mark.gpu
def test_stem_wgrad_at_the_training_size(det_gpu):
    test_k_dw_stem.test_stem_fwd_wgrad(det_gpu, "bf16", 20, 736, 1280)
    assert [op for op, _ in det_gpu.launches] == ["stem_wgrad"]
