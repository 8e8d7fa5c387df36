"""Generate tests/golden/frames_ref.npz by running THE REFERENCE's own src/frames.py (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frames.py

/root/reference/src/frames.py is loaded by path (it imports abc, typing and torch only).  Each case is a tiny uint8 input, the
constructor arguments, and what `get_frames_processor("pad_normalize", ...)` of that file returns for it - so the fixture
pins the registry, the pad split (top / left = total // 2) and the normalisation in one go.  Only inputs, settings and recorded
results (data) are stored.

Cases:  bytes   all 256 byte values, 16 x 16 -> 16 x 16: no pad
        odd     3 x 5 x 7 -> 8 x 12 (size = (12, 8)): height pad 3 = 1 + 2, width pad 5 = 2 + 3
        fill    2 x 2 x 6 x 10 -> 9 x 13, fill_value 37: two leading dimensions, odd pads of 1 + 2 both ways
        bytes_fill  all 256 byte values, 16 x 16 -> 19 x 20, fill_value 200
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_FILE = "/root/reference/src/frames.py"


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_frames", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    g = torch.Generator().manual_seed(61)
    every = torch.arange(256, dtype=torch.uint8).reshape(16, 16)
    cases = {       # name -> (input, size = (width, height), fill_value)
        "bytes": (every, (16, 16), 0),
        "odd": (torch.randint(0, 256, (3, 5, 7), generator=g, dtype=torch.uint8), (12, 8), 0),
        "fill": (torch.randint(0, 256, (2, 2, 6, 10), generator=g, dtype=torch.uint8), (13, 9), 37),
        "bytes_fill": (every.flip(0).contiguous(), (20, 19), 200),
    }
    d = dict(names=np.array(list(cases)))
    for name, (x, size, fill) in cases.items():
        proc = ref.get_frames_processor("pad_normalize", dict(size=size, pad_mode="constant", fill_value=fill))
        assert type(proc).__name__ == "PadNormalizeFramesProcessor"
        y = proc(x)
        assert y.dtype == torch.float32 and tuple(y.shape[-2:]) == (size[1], size[0])
        d[f"{name}.x"], d[f"{name}.size"], d[f"{name}.fill"], d[f"{name}.y"] = x.numpy(), np.array(size), np.array(fill), y.numpy()
    np.savez_compressed(os.path.join(HERE, "frames_ref.npz"), **d)
    print({k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
