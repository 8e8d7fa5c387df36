"""Host implementation of the mask definition in include/mds.h (mds_mask_fill): Philox4x32-10 in numpy, written from the
header's text - no kernel code, nothing of the product - and the layout of one forward's masks taken from the oracle's own modules.
The device-RNG tests predict every mask bit with it."""
import numpy as np
import torch

from oracle import multidim_stacker_ref as orc

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two 32-bit ints -> four uint32 arrays"""
    c = [np.asarray(w, dtype=np.uint64) & LO for w in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                        # < 2^64: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def uniforms(n, seed, stream, draw):
    """u[e] of the header's definition as fp32, e < n"""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    out = philox4x32_10((blocks, stream & 0xFFFFFFFF, draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    r = np.stack(out, axis=1).reshape(-1)[:n]
    return (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def mask(keep, seed, stream, draw):
    """the arena mds_mask_fill writes for the fp32 keep table `keep` (torch, any device) - a CPU fp32 tensor"""
    kp = keep.detach().cpu().float().contiguous()
    u = torch.from_numpy(uniforms(kp.numel(), seed, stream, draw))
    return torch.where(u < kp, torch.ones_like(kp) / kp, torch.zeros_like(kp))      # IEEE fp32 division, as div_ did


def plan_keep(plan):
    """the keep table of a plan from its `masks` list [(offset, n, keep)] - what Plan._finalize uploads as mask_keep"""
    kp = torch.empty(sum(n for _, n, _ in plan.masks), dtype=torch.float32)
    for off, n, k in plan.masks:
        kp[off:off + n] = k
    return kp


def oracle_keep(ref, B):
    """the keep probability of every mask element of one forward of `ref` at batch B, in the order the network uses them
    (DropPath of the 2D blocks per frame stack, DropPath of the 3D blocks per window, the classifier's dropout) - from the
    oracle's own modules, nothing of the engine; returns (keep table, [(setter, offset, n)])"""
    S = ref.num_stacks
    keeps, slots, off = [], [], 0

    def add(n, keep, setter):
        nonlocal off
        keeps.append(torch.full((n,), keep, dtype=torch.float32))
        slots.append((setter, off, n))
        off += n
    for blk in [b for st in ref.conv2d_encoder.blocks for b in st]:
        if blk.has_skip and isinstance(blk.drop_path, orc.DropPath) and blk.drop_path.drop_prob > 0:
            add(B * S, 1.0 - blk.drop_path.drop_prob, lambda m, dp=blk.drop_path: setattr(dp, "forced_mask", m))
    for blk in ref.conv3d_encoder:
        if isinstance(blk.drop_path, orc.DropPath) and blk.drop_path.drop_prob > 0:
            add(B, 1.0 - blk.drop_path.drop_prob, lambda m, dp=blk.drop_path: setattr(dp, "forced_mask", m))
    if ref.drop_rate > 0:
        F = ref.num_features
        add(B * F, 1.0 - ref.drop_rate, lambda m: setattr(ref, "forced_dropout_mask", m.view(B, F)))
    return torch.cat(keeps), slots


def feed_oracle(ref, B, seed, stream, draw, dtype=torch.float32):
    """give the oracle the masks that forward number `draw` of a device_rng module with this seed and stream draws; returns the arena"""
    keep, slots = oracle_keep(ref, B)
    arena = mask(keep, seed, stream, draw)
    for setter, off, n in slots:
        setter(arena[off:off + n].clone().to(dtype))
    return arena
