"""Generate tests/golden/mixup_ref.npz by running THE REFERENCE's own src/mixup.py (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mixup.py

/root/reference/src/mixup.py is loaded by path.  Its `from timm.data.mixup import Mixup` (timm is absent here) is satisfied by a
placeholder module whose `Mixup` is this repository's restatement (tests/mixup_host.py).  What the fixture pins is therefore the
reference's own file - `mixup_target`, `_params_per_elem`, the mode dispatch and the pairing check of `__call__`, executed line
for line - on top of the restated base class.  Only inputs, settings and recorded results (data) are stored.
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mixup_host  # noqa: E402

REF_FILE = "/root/reference/src/mixup.py"
SHAPE = (4, 3, 12, 16)
CLASSES = 2
# (mixup_alpha, cutmix_alpha, cutmix_minmax lo, hi; nan = no minmax)
CONFIGS = np.array([[0.4, 0.0, np.nan, np.nan], [0.0, 1.0, np.nan, np.nan], [0.4, 1.0, np.nan, np.nan], [0.0, 0.0, 0.2, 0.6]])
MODES = ("batch", "elem", "pair")


def load_reference():
    timm, data, mix = types.ModuleType("timm"), types.ModuleType("timm.data"), types.ModuleType("timm.data.mixup")
    mix.Mixup = mixup_host.Mixup
    timm.data, data.mixup = data, mix
    for n, m in (("timm", timm), ("timm.data", data), ("timm.data.mixup", mix)):
        sys.modules[n] = m
    spec = importlib.util.spec_from_file_location("ref_mixup", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def config_kwargs(row):
    ma, ca, lo, hi = (float(v) for v in row)
    return dict(mixup_alpha=ma, cutmix_alpha=ca, cutmix_minmax=None if np.isnan(lo) else (lo, hi))


def main():
    ref = load_reference()
    g = torch.Generator().manual_seed(52)
    x = torch.rand(*SHAPE, generator=g)
    target = (torch.rand(SHAPE[0], CLASSES, generator=g) < 0.5).float()
    d = dict(x=x.numpy(), target=target.numpy(), configs=CONFIGS)
    # mixup_target: a Python-float lam and a (B, 1) fp32 lam
    d["target.scalar.lam"] = np.array(0.3)
    d["target.scalar.out"] = ref.mixup_target(target, CLASSES, 0.3, 0.1).numpy()
    lam_col = torch.tensor([[0.25], [1.0], [0.7], [0.1]])
    d["target.column.lam"] = lam_col.numpy()
    d["target.column.out"] = ref.mixup_target(target, CLASSES, lam_col, 0.1).numpy()
    # _params_per_elem: the three alpha combinations, prob 0.7, n = 6; `next` = the draw that follows (how much was consumed)
    for ci in range(3):
        np.random.seed(100 + ci)
        m = ref.TimmMixup(prob=0.7, switch_prob=0.5, mode="elem", **config_kwargs(CONFIGS[ci]))
        lam, use_cutmix = m._params_per_elem(6)
        d[f"elem.{ci}.lam"], d[f"elem.{ci}.cut"], d[f"elem.{ci}.next"] = lam, use_cutmix, np.array(np.random.rand())
    # __call__: three modes x four settings, seed 7 + case number
    case = 0
    for mode in MODES:
        for ci in range(len(CONFIGS)):
            np.random.seed(7 + case)
            m = ref.TimmMixup(prob=1.0, switch_prob=0.5, mode=mode, label_smoothing=0.1, num_classes=CLASSES, **config_kwargs(CONFIGS[ci]))
            xo, to = m(x.clone(), target.clone())
            d[f"call.{mode}.{ci}.x"], d[f"call.{mode}.{ci}.t"], d[f"call.{mode}.{ci}.seed"] = xo.numpy(), to.numpy(), np.array(7 + case)
            d[f"call.{mode}.{ci}.next"] = np.array(np.random.rand())
            assert not torch.equal(xo, x), (mode, ci, "this seed does not mix")
            case += 1
    np.savez_compressed(os.path.join(HERE, "mixup_ref.npz"), **d)
    print({k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
