"""Drop-in ``MultiDimStacker`` for MI355X.

Same constructor, attributes, methods and ``state_dict`` as the reference class
(``src/models/multidim_stacker.py:137-243``); ``src/argus_models.py``,
``src/predictors.py`` and ``src/ema.py`` run on it unchanged.  All arithmetic
runs in the hand-written gfx950 kernels of ``libmds_hip.so`` (C ABI: include/mds.h) driven by
``engine.Plan``; if the library is missing this module raises — there is no eager/CPU fallback.

``torch.compile(module)`` (``scripts/ball_action/train.py:83-86``): the training forward is a registered operator,
``torch.ops.mds.forward`` (``torch.library.custom_op`` with a fake implementation and an autograd formula whose backward is
the operator ``torch.ops.mds.backward``), so Dynamo / AOTAutograd / Inductor trace THROUGH ``forward`` with
``fullgraph=True`` and see one opaque node each way - the hot path already is a static launch schedule, there is nothing for a
tracing compiler to add.  The operator finds its module through an integer handle (operators take tensors and scalars,
not modules); BatchNorm's running statistics are updated by the launch as a side effect, as in eager mode.

One bridge to a plan: ``KINDS`` says, per plan kind, which segments run and which buffers are the input, the output, the incoming
gradient and the input gradient, in which of the reference's forms; ``_issue_forward`` / ``_issue_backward`` are the only code that
stages tensors and issues schedules.  The operator's bodies call them, and so does ``_Bridge``, the one ``torch.autograd.Function``:
``forward_tail``, ``forward_2d`` / ``forward_3d`` / ``forward_head`` under autograd, and ``forward`` itself with ``MDS_CUSTOM_OP=0``
(behind ``torch.compiler.disable``: a graph break).

``forward`` and ``forward_2d`` are differentiable in the frame tensor too: with ``x.requires_grad`` the 2D backward chain ends in the
stem's data-gradient kernel (``mds_stem_dgrad``) and ``x.grad`` comes back in the caller's ``(B,T,H,W)`` shape.  The chain exists only
where the 2D encoder trains; with a frozen encoder ``x.grad`` stays ``None`` and the module says so once (a ``RuntimeWarning``).
"""
from __future__ import annotations

import copy
import itertools
import os
import warnings
import weakref
from collections import OrderedDict
from typing import List, NamedTuple, Optional, Tuple

import torch
from torch import nn

from . import cabi
from .engine import Plan, PlanOptions
from .structure import (EncoderP, InvertedResidual3dP, GeneralizedMeanPoolingP, TAIL_BN_EPS)

MAX_PLANS = 8     # launch plans kept per module (LRU); each pins its activation arena (12 GB at config 2)


class _PlanCache:
    """Per-module LRU cache of launch plans.  Never copied or pickled (EMA deep-copies the module,
    src/ema.py:40): a copy starts with an empty cache and re-plans on first use."""

    def __init__(self):
        self.plans = OrderedDict()       # key -> [Plan, ...]

    def __deepcopy__(self, memo):
        return _PlanCache()

    def __reduce__(self):
        return (_PlanCache, ())

    def count(self):
        return sum(len(v) for v in self.plans.values())

    def idle(self):
        return sum(1 for v in self.plans.values() for p in v if not p.in_flight)

    def evict(self, keep_key):
        """drop least-recently-used IDLE plans until at most MAX_PLANS of them remain.  Plans that are in flight - held by
        an autograd graph, or owned by a StreamPredictor for its lifetime - do not count against the budget: they cannot be
        dropped, and counting them made every later shape of the module re-plan on each call once a predictor held eight."""
        for key in list(self.plans):
            if self.idle() <= MAX_PLANS:
                break
            if key == keep_key:
                continue
            pool = self.plans[key]
            pool[:] = [p for p in pool if p.in_flight]
            if not pool:
                del self.plans[key]


class _Release:
    """Marks a plan reusable when the autograd graph that references it dies - unless a later forward has taken the plan since."""

    def __init__(self, plan):
        self.plan, self.generation = plan, plan.generation

    def __del__(self):
        plan = getattr(self, "plan", None)      # __del__ may run on a half-built / torn-down object
        if plan is not None and plan.generation == self.generation:
            plan.in_flight = False


class _Release2:
    """the same for the registered operator's path: lives on the autograd context, releases the plan named by the token"""

    def __init__(self, handle, token):
        self.handle, self.token = handle, token

    def __del__(self):
        try:
            _release_token(self.handle, self.token)
        except Exception:       # interpreter shutdown
            pass


_RELEASED = ("mds: the activations of this forward have been released (backward already ran, or the plan was reused by a "
             "later forward); a second backward / retain_graph is not supported")


# ------------------------------------------------------------------------------------------------ the boundary of each plan kind
class _Kind(NamedTuple):
    """what crosses the boundary between PyTorch and a plan of one kind.  inp / out / gout / dinp name a buffer of the plan and
    the form the caller sees it in: "frames" - the (b,t,h,w) frame stack, bound in place (its gradient, `dx`, exists only on a
    plan with input_grad); "flat" - logits / their gradient; "5d" - (b,s,c,h,w) stacks; "4d" - the merged (b,s*c,h,w)."""
    fwd: Tuple[str, ...]            # forward segments, in issue order
    bwd: Tuple[str, ...]            # backward segments, in issue order
    inp: Tuple[str, str]
    out: Tuple[str, str]
    gout: Tuple[str, str]           # where the incoming gradient is staged
    dinp: Tuple[str, str]           # where the input gradient is read
    params: Tuple[str, ...]         # name prefixes of the parameters this part of the network owns


KINDS = {
    "full": _Kind(("f2d", "f3d", "fhead"), ("bhead", "b3d", "b2d"), ("x_in", "frames"), ("logits", "flat"), ("dlogits", "flat"),
                  ("dx", "frames"), ("",)),
    "2d": _Kind(("f2d",), ("b2d",), ("x_in", "frames"), ("feat", "5d"), ("dfeat_in", "5d"), ("dx", "frames"),
                ("conv2d_encoder.", "conv2d_projection.")),
    "3d": _Kind(("f3d",), ("b3d",), ("feat", "5d"), ("out3d", "4d"), ("uq_in", "4d"), ("dfeat", "5d"),
                ("conv3d_encoder.", "conv3d_projection.")),
    "head": _Kind(("fhead",), ("bhead",), ("yq", "4d"), ("logits", "flat"), ("dlogits", "flat"), ("dyq_out", "4d"),
                  ("global_pool.", "classifier.")),
    # forward_3d -> forward_head as one call on given 2D features: everything that is not the 2D encoder
    "tail": _Kind(("f3d", "fhead"), ("bhead", "b3d"), ("feat", "5d"), ("logits", "flat"), ("dlogits", "flat"), ("dfeat", "5d"),
                  ("conv3d_encoder.", "conv3d_projection.", "global_pool.", "classifier.")),
}


def _rows(plan, buf):
    """a buffer of the plan as the kernels address it: channels-last rows [b][s][h][w][c]"""
    return buf.tensor.view(plan.B, plan.T // plan.m.stack_size, plan.h, plan.w, -1)


def _rows_from_5d(plan, buf, t):
    _rows(plan, buf).copy_(t.detach().permute(0, 1, 3, 4, 2))


def _5d_from_rows(plan, buf):
    """(b,s,c,h,w) like the reference, fp32 - always a copy: the plan's buffer is rewritten by the next step"""
    return _rows(plan, buf).permute(0, 1, 4, 2, 3).float().clone(memory_format=torch.contiguous_format)


def _rows_from_4d(plan, buf, t):
    b, f, h, w = t.shape
    s = plan.T // plan.m.stack_size
    _rows_from_5d(plan, buf, t.reshape(b, s, f // s, h, w))


def _4d_from_rows(plan, buf):
    return _5d_from_rows(plan, buf).flatten(1, 2)


def _stage(plan, where, t):
    """hand a caller's tensor (an input, or the gradient of an output) to the plan"""
    name, form = where
    if form == "frames":
        plan.bind_input(t)          # no staging copy: the stem kernels read the caller's tensor
    elif form == "flat":
        plan.bind_dlogits(t)
    else:
        (_rows_from_5d if form == "5d" else _rows_from_4d)(plan, getattr(plan, name), t)


def _read(plan, where):
    """an output or an input gradient of the plan in the caller's form - a copy, the plan's buffers are rewritten by the next step"""
    name, form = where
    if form == "frames":
        # None for a plan without the stem's data gradient.  Under data parallelism it is the rank's own (each rank
        # differentiates its own frames): never all-reduced, it is not part of the gradient arena.
        return plan.dx.tensor.view(plan.B, plan.T, plan.H, plan.W).clone() if plan.input_grad else None
    if form == "flat":
        return getattr(plan, name).tensor.view(plan.B, -1).clone()
    return (_5d_from_rows if form == "5d" else _4d_from_rows)(plan, getattr(plan, name))


def _issue_forward(module, plan, kind, inp):
    """issue the forward schedule of `plan` on `inp`; returns the output of that kind"""
    k = KINDS[kind]
    with plan.device_guard():
        _stage(plan, k.inp, inp)
        plan.begin_forward(module._mask_override, rng=module._draw(plan))
        for seg in k.fwd:
            plan.run(seg)
        return _read(plan, k.out)


def _issue_backward(module, plan, kind, inp, gout):
    """issue the backward schedule of `plan`; returns the flat gradient buffer (all parameters, parameter order; averaged over
    ranks under data parallelism) and the gradient of `inp` (None where the plan has none)"""
    k = KINDS[kind]
    sync = getattr(module, "_grad_sync", None) if kind == "full" else None       # only the whole network is data parallel
    bucketed = hasattr(sync, "on_cut")
    with plan.device_guard():
        if k.inp[1] == "frames":
            plan.bind_input(inp)                   # the stem's weight and data gradients read the frames again
        _stage(plan, k.gout, gout)                 # (buffers of their own, outside the arena begin_backward zeroes)
        plan.begin_backward()
        plan.cut_hook = sync.on_cut if bucketed else None     # all-reduce each slice of the arena as soon as it is final
        for seg in k.bwd:
            plan.run(seg)
        plan.cut_hook = None
        plan.join_backward()
        if bucketed:
            world = sync.finish(plan)
            flat = plan.grad_arena.tensor / world if world > 1 else plan.grad_arena.tensor.clone()
        else:
            flat = plan.grad_arena.tensor.clone()  # one launch; the arena is reused next step
            if sync is not None:
                sync(flat)                         # one RCCL all-reduce of the flat buffer
        return flat, _read(plan, k.dinp)


def _param_grads(flat, meta):
    """the flat gradient buffer cut into per-parameter views; None for a frozen parameter.  `meta`: (offset, numel, shape,
    requires_grad) per parameter - scalars, so an autograd context can keep it while a compiler traces"""
    return [flat[off:off + n].view(shape) if req else None for off, n, shape, req in meta]


class _Bridge(torch.autograd.Function):
    """the one differentiable call into a plan, for every kind: forward() with MDS_CUSTOM_OP=0, forward_tail, and forward_2d /
    forward_3d / forward_head under autograd (the reference's are ordinary differentiable methods, multidim_stacker.py:210-237).
    Gradients for the input and for the parameters handed in - those of that part of the network.  The plan's activations
    are this forward's while the plan is in flight and no later forward has bumped its generation."""

    @staticmethod
    def forward(ctx, inp, module, plan, kind, *params):
        ctx.module, ctx.plan, ctx.kind = module, plan, kind
        plan.in_flight = True
        plan.generation += 1
        ctx.generation, ctx.release = plan.generation, _Release(plan)
        ctx.meta = [(plan.poff[id(p)], p.numel(), p.shape, p.requires_grad) for p in params]
        ctx.save_for_backward(inp)          # version-checked: an in-place edit of the input before backward raises
        return _issue_forward(module, plan, kind, inp)

    @staticmethod
    def backward(ctx, gout):
        plan = ctx.plan
        if ctx.generation != plan.generation or not plan.in_flight:
            raise RuntimeError(_RELEASED)
        (inp,) = ctx.saved_tensors          # raises if the input was modified in place since forward
        flat, dinp = _issue_backward(ctx.module, plan, ctx.kind, inp, gout)
        plan.in_flight = False
        return (dinp, None, None, None, *_param_grads(flat, ctx.meta))


# ------------------------------------------------------------------------------------------------ registered operators
_MODULES = weakref.WeakValueDictionary()      # handle -> MultiDimStacker (operators cannot take a module argument)
_HANDLES = itertools.count(1)
_TOKENS = itertools.count(1)
USE_CUSTOM_OP = os.environ.get("MDS_CUSTOM_OP", "1") != "0"


def _module_of(handle: int):
    m = _MODULES.get(handle)
    if m is None:
        raise RuntimeError(f"mds: module handle {handle} is gone (the MultiDimStacker it named was deleted)")
    return m


# A training forward also updates the BatchNorm running statistics and draws DropPath / dropout masks.  torch refuses an autograd
# formula on an operator that declares mutated arguments, so the operator stays functional in its schema and carries the
# `nondeterministic_seeded` tag instead (it IS seeded-random with drop rates > 0): graph passes that merge or reorder pure nodes
# leave tagged operators alone.  tests/test_module_emu.py runs two identical calls in one compiled graph and checks that the
# statistics advance twice.
@torch.library.custom_op("mds::forward", mutates_args=(), tags=(torch.Tag.nondeterministic_seeded,))
def _op_forward(x: torch.Tensor, params: List[torch.Tensor], handle: int, need_grad: bool, code: int,
                input_grad: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits of MultiDimStacker.forward + a CPU token naming the launch plan that holds the activations for backward.
    `params` only tells autograd what the result depends on - the kernels read the module's parameters in place.
    `input_grad`: x requires grad (inside the operator autograd is off and x does not say so itself)."""
    m = _module_of(handle)
    b, t, h, w = x.shape
    plan = m._plan(x, "full", b, t, h, w, need_grad, code=code, input_grad=input_grad)
    token = 0
    if need_grad:
        live = m._live
        while len(live) >= 4:                      # forwards whose backward never came (loss evaluated under grad mode, then dropped)
            live.pop(next(iter(live))).in_flight = False
        token = next(_TOKENS)
        live[token] = plan
        plan.in_flight = True
        plan.generation += 1
    return _issue_forward(m, plan, "full", x), torch.tensor(token, dtype=torch.int64)


@_op_forward.register_fake
def _(x, params, handle, need_grad, code, input_grad):
    return x.new_empty((x.shape[0], _module_of(handle).classifier.out_features), dtype=torch.float32), torch.empty((), dtype=torch.int64)


@torch.library.custom_op("mds::backward", mutates_args=())
def _op_backward(dlogits: torch.Tensor, x: torch.Tensor, token: torch.Tensor, handle: int, input_grad: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """the flat fp32 gradient arena (all parameters, parameter order) of the forward named by `token`, and the gradient of x in
    x's shape - an empty tensor unless `input_grad` (what the forward was told) and the plan has the stem's data gradient"""
    m = _module_of(handle)
    plan = m._live.pop(int(token.item()), None)          # (a CPU scalar: no device synchronisation)
    if plan is None:
        raise RuntimeError(_RELEASED)
    flat, dx = _issue_backward(m, plan, "full", x, dlogits)      # (dx only on a plan with input_grad - what the forward was told)
    plan.in_flight = False
    return flat, (dx if dx is not None else x.new_empty((0,)))


@_op_backward.register_fake
def _(dlogits, x, token, handle, input_grad):
    m = _module_of(handle)
    has_dx = input_grad and any(p.requires_grad for p in m.conv2d_encoder.parameters())      # Plan.input_grad's rule
    return (dlogits.new_empty((sum(p.numel() for p in m.parameters()),), dtype=torch.float32),
            x.new_empty(x.shape if has_dx else (0,)))


def _release_token(handle, token):
    """the autograd node of a grad-enabled forward died without running backward (loss only evaluated, an exception): its plan
    - a full activation arena - becomes reusable at once instead of after four later forwards"""
    m = _MODULES.get(handle)
    if m is not None:
        plan = m._live.pop(token, None)
        if plan is not None:
            plan.in_flight = False


def _op_setup_context(ctx, inputs, output):
    x, params, handle, need_grad, code, input_grad = inputs
    ctx.input_grad = bool(input_grad)
    ctx.save_for_backward(x, output[1])     # x is version-checked: an in-place edit before backward raises
    ctx.handle = handle
    tok = output[1]
    if need_grad and type(tok) is torch.Tensor and not torch.compiler.is_compiling():     # (not while tracing: fake tensors have no value)
        ctx._mds_release = _Release2(handle, int(tok))
    offs = itertools.accumulate([0] + [p.numel() for p in params])       # all parameters in parameter order: Plan.poff
    ctx.meta = [(off, p.numel(), p.shape, p.requires_grad) for off, p in zip(offs, params)]


def _op_backward_formula(ctx, dlogits, dtoken):
    x, token = ctx.saved_tensors
    flat, dx = torch.ops.mds.backward(dlogits.contiguous(), x, token, ctx.handle, ctx.input_grad)
    return (dx if ctx.input_grad and dx.numel() else None), _param_grads(flat, ctx.meta), None, None, None, None


_op_forward.register_autograd(_op_backward_formula, setup_context=_op_setup_context)


def _load_pretrained_encoder(encoder: nn.Module, model_name: str, in_chans: int):
    """``pretrained=True`` (configs/ball_action/sampling_weights_001.py:36): the reference gets ImageNet
    weights from ``timm.create_model(..., pretrained=True)`` (multidim_stacker.py:166-176).  Do the same when
    timm and its weight cache are reachable; otherwise say so LOUDLY — never a silent random init."""
    try:
        import timm  # noqa: F401  (absent from the build image; present in the reference's environment)
        src = timm.create_model(model_name, pretrained=True, in_chans=in_chans, features_only=True, out_indices=[4])
        sd = src.state_dict()
        own = encoder.state_dict()
        if set(sd) != set(own) or any(sd[k].shape != own[k].shape for k in own):
            raise RuntimeError("timm state_dict does not match the mds encoder layout (timm version != 0.9.2?)")
        encoder.load_state_dict(sd)
        return True
    except Exception as e:  # ImportError, no network / no cached weights, layout mismatch
        msg = (f"mds.MultiDimStacker(pretrained=True): ImageNet weights for '{model_name}' could not be loaded "
               f"({type(e).__name__}: {e}).")
        if os.environ.get("MDS_ALLOW_RANDOM_INIT") != "1":
            # the reference's timm.create_model(pretrained=True) fails hard here too; stage-1 training from a random encoder
            # is never what the caller meant
            raise RuntimeError(msg + " Install timm with its cached weights, construct with pretrained=False and load a "
                               "checkpoint (load_state_dict / src.utils.load_weights_from_pretrain), or set "
                               "MDS_ALLOW_RANDOM_INIT=1 to continue with a RANDOMLY INITIALISED encoder.") from e
        warnings.warn(msg + " MDS_ALLOW_RANDOM_INIT=1: the 2D encoder is RANDOMLY INITIALISED.", RuntimeWarning, stacklevel=3)
        return False


class MultiDimStacker(nn.Module):
    def __init__(self, model_name: str, num_classes: int, num_frames: int = 15, stack_size: int = 3,
                 index_2d_features: int = 4, pretrained: bool = False, num_3d_blocks: int = 2,
                 num_3d_features: int = 192, num_3d_stack_proj: int = 256, expansion_3d_ratio: int = 6,
                 se_reduce_3d_ratio: int = 24, drop_rate: float = 0., drop_path_rate: float = 0.,
                 act_layer: str = "silu", **kwargs):
        super().__init__()
        assert num_frames > 0 and num_frames % stack_size == 0
        if model_name.split(".")[0] != "tf_efficientnetv2_b0":
            raise NotImplementedError(f"mds HIP engine implements the reference's encoder tf_efficientnetv2_b0, got {model_name}")
        if act_layer != "silu" or index_2d_features != 4 or stack_size != 3:
            raise NotImplementedError("mds HIP engine: act_layer='silu', index_2d_features=4, stack_size=3 (all reference configs)")
        self.num_frames = num_frames
        self.stack_size = stack_size
        self.num_3d_features = num_3d_features
        self.num_stacks = num_frames // stack_size
        self.num_features = num_3d_stack_proj * self.num_stacks
        self.drop_rate = drop_rate
        self.conv2d_encoder = EncoderP(in_chans=stack_size, drop_path_rate=drop_path_rate)
        self.pretrained_loaded = _load_pretrained_encoder(self.conv2d_encoder, model_name, stack_size) if pretrained else False
        enc_chs = self.conv2d_encoder.feature_info[index_2d_features]["num_chs"]
        self.conv2d_projection = nn.Sequential(
            nn.Conv2d(enc_chs, num_3d_features, 1, bias=False), nn.BatchNorm2d(num_3d_features, eps=TAIL_BN_EPS))
        self.conv3d_encoder = nn.Sequential(*[
            InvertedResidual3dP(num_3d_features, num_3d_features, expansion_3d_ratio, se_reduce_3d_ratio, drop_path_rate)
            for _ in range(num_3d_blocks)])
        self.conv3d_projection = nn.Sequential(
            nn.Conv2d(num_3d_features, num_3d_stack_proj, 1, bias=False), nn.BatchNorm2d(num_3d_stack_proj, eps=TAIL_BN_EPS))
        self.global_pool = GeneralizedMeanPoolingP(3.0)
        self.classifier = nn.Linear(self.num_features, num_classes, bias=True)
        # engine state (not part of state_dict)
        self.compute_dtype = "auto"           # "auto": bf16 under autocast, fp32 otherwise | "bf16" | "f32"
        self.eval_fusion = False              # eval + no-grad plans: the 2D blocks' 1x1 expansion runs inside the depthwise launch
        self.eval_se_fusion = False           # eval + no-grad plans: the pooling depthwise launch also computes the squeeze-excite gate
        self.eval_er_fusion = False           # eval + no-grad plans: the edge-residual blocks' 3x3 expansion and 1x1 projection run in one launch
        self.deterministic = False            # training plans: weight gradients summed in a fixed order (bit-identical reruns of a step)
        self.device_rng = False               # training plans: DropPath / dropout masks from the engine's own Philox stream (mds_mask_fill)
        self.rng_seed = None                  # device_rng: None until the first drawing forward takes torch.initial_seed(); seed_rng() sets it
        self.rng_stream = 0                   # device_rng: mds.parallel sets the rank, so that ranks sharing a seed draw different masks
        self.rng_draws = 0                    # device_rng: forwards that filled a mask arena so far = the draw number of the next one
        self._cache = _PlanCache()
        self._lib: Optional[cabi.Lib] = None  # tests inject the kernel simulator here; product: cabi.load()
        self._mask_override = None            # parity tests: host-supplied DropPath/dropout masks
        self._grad_sync = None                # mds.parallel.data_parallel installs the all-reduce here
        self._register()

    def _register(self):
        """a fresh operator handle for this instance (never shared with the module it was copied / unpickled from)"""
        self._handle = next(_HANDLES)
        self._live = {}                       # token -> plan of a grad-enabled forward whose backward has not run yet
        self._warned_fp16 = False
        self._warned_input_grad = False
        _MODULES[self._handle] = self

    def __deepcopy__(self, memo):             # src/ema.py:40 deep-copies the module: the copy is its own operator target
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_live" else (v if k == "_lib" else copy.deepcopy(v, memo))     # (a loaded library is shared)
        new._register()
        return new

    def __getstate__(self):                   # plans of forwards in flight are not part of the module's state
        state = dict(self.__dict__)
        state["_live"] = {}
        return state

    def __setstate__(self, state):            # torch.save(module) / pickle
        super().__setstate__(state)
        self._register()

    # ------------------------------------------------------------------ plumbing
    def _apply(self, fn, *a, **k):
        self._cache = _PlanCache()            # .to()/.cuda()/.half() move parameters: re-plan
        return super()._apply(fn, *a, **k)

    def clear_plans(self):
        """Release every cached launch plan (and the activation arenas they pin)."""
        self._cache = _PlanCache()

    def _library(self, x):
        if self._lib is not None:
            return self._lib
        if not x.is_cuda:
            raise cabi.MdsError("MultiDimStacker (mds) runs on MI355X only: move the module and input to cuda")
        return cabi.load()

    def _code(self):
        if self.compute_dtype == "bf16":
            return cabi.MDS_BF16
        if self.compute_dtype == "f32":
            return cabi.MDS_F32
        if torch.is_autocast_enabled() or torch.is_autocast_enabled('cpu'):
            # The reference's AMP is fp16 autocast + GradScaler (src/argus_models.py:36,54).  The kernels store bf16: same
            # range as fp32 (a GradScaler then never finds an overflow and simply keeps its scale), 3 mantissa bits fewer
            # than fp16 - said once, not silently.
            dt = torch.get_autocast_dtype("cuda" if torch.is_autocast_enabled() else "cpu")
            if dt == torch.float16 and not self._warned_fp16 and not torch.compiler.is_compiling():
                self._warned_fp16 = True
                warnings.warn("mds.MultiDimStacker: fp16 autocast is executed with bf16 storage (fp32 accumulation); "
                              "torch.autocast(dtype=torch.bfloat16) is the matching setting and needs no GradScaler.", stacklevel=3)
            return cabi.MDS_BF16
        return cabi.MDS_F32

    def _plan(self, x, kind, B, T, H, W, need_grad, ingest=None, code=None, input_grad=False):
        lib = self._library(x)
        enc_grad = any(p.requires_grad for p in self.conv2d_encoder.parameters())
        code = self._code() if code is None else code
        opts = PlanOptions.of(self, self.training, need_grad)
        # (the frames require grad AND the 2D backward chain exists - Plan.input_grad's rule: a property of the call, not a switch)
        input_grad = bool(input_grad) and bool(need_grad) and enc_grad and kind in ("full", "2d")
        key = (kind, B, T, H, W, code, self.training, need_grad, enc_grad, input_grad, x.device, ingest, opts)
        cache = self._cache
        pool = cache.plans.setdefault(key, [])
        cache.plans.move_to_end(key)
        for plan in pool:
            if not plan.in_flight and not plan.stale():
                return plan
        pool[:] = [p for p in pool if not p.stale()]
        plan = Plan(self, lib, x.device, kind, B, T, H, W, code, self.training, need_grad, enc_grad, ingest=ingest, options=opts,
                    input_grad=input_grad)
        pool.append(plan)
        cache.evict(key)
        return plan

    # ------------------------------------------------------------------ device_rng: the module's own mask stream
    def seed_rng(self, seed: int):
        """fix the seed of the mask stream and restart it at draw 0"""
        self.rng_seed, self.rng_draws = int(seed) & 0xFFFFFFFFFFFFFFFF, 0

    def rng_state(self):
        """what a checkpoint needs to resume the mask sequence (seed is None before the first drawing forward or seed_rng())"""
        return dict(seed=getattr(self, "rng_seed", None), stream=int(getattr(self, "rng_stream", 0)), draws=int(getattr(self, "rng_draws", 0)))

    def set_rng_state(self, state):
        seed = state["seed"]
        self.rng_seed = None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rng_stream, self.rng_draws = int(state["stream"]) & 0xFFFFFFFF, int(state["draws"])

    def _draw(self, plan):
        """(seed, stream, draw) for the forward about to be issued on `plan` and the counter moves on - or None: the plan draws
        nothing from the module's stream (no masks, the switch is off, or a test injects the masks).  The draw number counts
        drawing forwards only: it does not depend on which cached plan runs."""
        if not plan.device_rng or self._mask_override is not None:
            return None
        if getattr(self, "rng_seed", None) is None:       # torch.manual_seed still governs a run that never calls seed_rng()
            self.rng_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        draw = int(getattr(self, "rng_draws", 0))
        self.rng_draws = draw + 1
        return self.rng_seed, int(getattr(self, "rng_stream", 0)) & 0xFFFFFFFF, draw

    def _wants_input_grad(self, x):
        """x requires grad under grad mode - and the 2D backward chain that ends in the stem's data gradient exists.  With a frozen
        2D encoder that chain is pruned from the plan: x.grad stays None, said once per instance, not silently."""
        if not (torch.is_grad_enabled() and x.requires_grad):
            return False
        if any(p.requires_grad for p in self.conv2d_encoder.parameters()):
            return True
        if not getattr(self, "_warned_input_grad", False) and not torch.compiler.is_compiling():
            self._warned_input_grad = True
            warnings.warn("mds.MultiDimStacker: the input requires grad but the 2D encoder is frozen - its backward chain is not "
                          "built, so no input gradient is computed (x.grad stays None). Leave the encoder's parameters trainable "
                          "to get the input gradient.", RuntimeWarning, stacklevel=3)
        return False

    # ------------------------------------------------------------------ reference API
    def forward(self, x):
        b, t, h, w = x.shape
        assert t == self.num_frames and t % self.stack_size == 0
        x = x.float().contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        input_grad = self._wants_input_grad(x)       # (implies need_grad: the encoder's parameters require grad)
        if USE_CUSTOM_OP:      # the registered operator: traceable by torch.compile(fullgraph=True), one opaque node each way
            return torch.ops.mds.forward(x, list(self.parameters()), self._handle, need_grad, self._code(), input_grad)[0]
        return self._forward_untraced(x, need_grad, input_grad)

    @torch.compiler.disable
    def _forward_untraced(self, x, need_grad, input_grad=False):
        b, t, h, w = x.shape
        plan = self._plan(x, "full", b, t, h, w, need_grad, input_grad=input_grad)
        if need_grad:
            return _Bridge.apply(x, self, plan, "full", *plan.params)
        return _issue_forward(self, plan, "full", x)

    def _params_of(self, kind):
        """the parameters of that part of the network, in parameter order"""
        return [p for n, p in self.named_parameters() if n.startswith(KINDS[kind].params)]

    def _sub(self, kind, inp, B, T, H, W):
        """one of the three sub-forwards: inference plan under no_grad (src/predictors.py:58-70), differentiable otherwise"""
        params = self._params_of(kind)
        need_grad = torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in params))
        plan = self._plan(inp, kind, B, T, H, W, need_grad, input_grad=kind == "2d" and self._wants_input_grad(inp))
        if need_grad:
            return _Bridge.apply(inp, self, plan, kind, *params)
        return _issue_forward(self, plan, kind, inp)

    @torch.compiler.disable
    def forward_2d(self, x):
        b, t, h, w = x.shape
        assert t % self.stack_size == 0
        return self._sub("2d", x.float().contiguous(), b, t, h, w)

    @torch.compiler.disable
    def forward_3d(self, x):
        b, t, c, h, w = x.shape
        assert c == self.num_3d_features and t == self.num_stacks
        return self._sub("3d", x, b, t * self.stack_size, h, w)

    @torch.compiler.disable
    def forward_tail(self, feats):
        """logits = forward_head(forward_3d(feats)) for feats of shape (b, num_stacks, 192, h, w), differentiable
        with respect to the features and the tail parameters (not part of the reference API)."""
        b, t, c, h, w = feats.shape
        assert c == self.num_3d_features and t == self.num_stacks
        plan = self._plan(feats, "tail", b, t * self.stack_size, h, w, True)
        return _Bridge.apply(feats, self, plan, "tail", *self._params_of("tail"))

    @torch.compiler.disable
    def forward_head(self, x):
        b, f, h, w = x.shape
        return self._sub("head", x, b, self.num_stacks * self.stack_size, h, w)
