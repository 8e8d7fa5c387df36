"""The liveness rule of every differentiable entry of the module, on the host kernel simulator (host logic only): a grad-enabled
forward holds exactly one plan of its kind until backward has run or the output is dropped, backward fills the gradients of that
part of the network and of nothing else, and a backward on released activations raises."""
import gc

import pytest
import torch

from oracle import multidim_stacker_ref as orc
from test_module_emu import _pair

KW = dict(orc.BASIC_CONFIG_KWARGS, drop_rate=0.0, drop_path_rate=0.0)
P2D, P3D, PHEAD = ("conv2d_encoder.", "conv2d_projection."), ("conv3d_encoder.", "conv3d_projection."), ("global_pool.", "classifier.")
# entry -> (plan kind, name prefixes of the parameters that receive a gradient)
ENTRIES = {"operator": ("full", P2D + P3D + PHEAD), "untraced": ("full", P2D + P3D + PHEAD), "forward_2d": ("2d", P2D),
           "forward_3d": ("3d", P3D), "forward_head": ("head", PHEAD), "forward_tail": ("tail", P3D + PHEAD)}


def _call(prod, entry, x):
    if entry == "operator":
        return torch.ops.mds.forward(x, list(prod.parameters()), prod._handle, True, prod._code(), True)[0]
    if entry == "untraced":          # the autograd.Function behind MDS_CUSTOM_OP=0, reached without a child process
        return prod._forward_untraced(x, True, prod._wants_input_grad(x))
    return getattr(prod, entry)(x)


def _in_flight(prod):
    return [p for pool in prod._cache.plans.values() for p in pool if p.in_flight]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_one_liveness_rule_for_every_entry(entry):
    kind, prefixes = ENTRIES[entry]
    _, prod = _pair(KW)
    prod.train()
    g = torch.Generator().manual_seed(7)
    S, C3, F = prod.num_stacks, prod.num_3d_features, prod.num_features
    shape = {"full": (1, 15, 32, 32), "2d": (1, 15, 32, 32), "3d": (1, S, C3, 3, 3), "tail": (1, S, C3, 3, 3), "head": (1, F, 3, 3)}[kind]
    x = torch.rand(*shape, generator=g).requires_grad_(True)

    out = _call(prod, entry, x)
    (plan,) = _in_flight(prod)                          # exactly one plan is held, and it is one of this kind
    assert plan.kind == kind and plan.need_grad
    loss = out.sum()
    del out
    loss.backward(retain_graph=True)
    assert x.grad is not None and x.grad.shape == x.shape          # (every kind has an input gradient; the 2D encoder trains)
    got = {n for n, p in prod.named_parameters() if p.grad is not None}
    assert got == {n for n, _ in prod.named_parameters() if n.startswith(prefixes)}
    assert got and (kind == "full") == (len(got) == len(list(prod.parameters())))
    assert not _in_flight(prod)                         # idle after backward
    with pytest.raises(RuntimeError, match="released"):
        loss.backward()

    out = _call(prod, entry, x)                         # the same shape again: the same plan
    assert _in_flight(prod) == [plan]
    del loss                                            # the first forward's graph dies late: it must not release the second's plan
    gc.collect()
    assert _in_flight(prod) == [plan]
    del out                                             # dropped without a backward
    gc.collect()
    assert not _in_flight(prod)
    assert all(not hasattr(p, "tail_params") for pool in prod._cache.plans.values() for p in pool)
