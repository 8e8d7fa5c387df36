"""Host side of the mixup tests: nothing of the product, no kernel code.

1. `apply_jobs`: the arithmetic that include/mds.h states for mds_mixup, in numpy - a job list gives the mixed batch and
   the target rows.  Every product and every sum is one fp32 rounding (numpy fp32 arrays never fuse).
2. `Mixup`: what timm 0.9.2's `timm.data.mixup.Mixup` does in the three methods the reference calls (`_mix_elem`, `_mix_pair`,
   `_mix_batch`) and the helpers behind them, restated in torch / numpy ops on the CPU.  timm is not installed where these tests
   run, so EVERY assumption about it lives in this file (unpinned by necessity).
3. `TimmMixup`, `mixup_target`: the reference's `src/mixup.py` restated on top of (2).  tests/golden/make_golden_mixup.py runs
   the reference's own file on top of (2) and records what it gives; tests/test_mixup.py holds this restatement to those
   recordings bit for bit.
"""
import numpy as np
import torch

NONE, BLEND, CUT = 0, 1, 2       # MDS_MIX_* of include/mds.h (tests/test_mixup.py compares them with the header's)
F32 = np.float32


# ------------------------------------------------------------------------------------------------ 1. the header's arithmetic
def job(mode=NONE, lam=1.0, oml=0.0, box=(0, 0, 0, 0)):
    return dict(mode=int(mode), lam=F32(lam), oml=F32(oml), box=tuple(int(v) for v in box))


def _smooth(t, off_value, on_value):
    return (F32(1) - t) * F32(off_value) + t * F32(on_value)


def apply_jobs(x, jobs, target=None, off_value=0.0, on_value=1.0, pair0=0, npairs=None, target_out=None):
    """x: (B, T, H, W) fp32 numpy, jobs: one job() per sample.  Returns (x', target_out): what ONE launch over pairs
    pair0 .. pair0 + npairs - 1 leaves behind; rows of other pairs keep x's (target_out's) values."""
    x = np.asarray(x, dtype=F32)
    B = x.shape[0]
    npairs = B // 2 - pair0 if npairs is None else npairs
    out = x.copy()
    tout = None
    if target is not None:
        target = np.asarray(target, dtype=F32)
        tout = np.zeros_like(target) if target_out is None else np.array(target_out, dtype=F32)
    for p in range(pair0, pair0 + npairs):
        for r in (p, B - 1 - p):
            jb, own, other = jobs[r], x[r], x[B - 1 - r]          # both from the ORIGINAL batch
            if jb["mode"] == BLEND:
                out[r] = own * jb["lam"] + other * jb["oml"]
            elif jb["mode"] == CUT:
                yl, yh, xl, xh = jb["box"]
                out[r][:, yl:yh, xl:xh] = other[:, yl:yh, xl:xh]
            if target is not None:
                y1, y2 = _smooth(target[r], off_value, on_value), _smooth(target[B - 1 - r], off_value, on_value)
                tout[r] = y1 * jb["lam"] + y2 * jb["oml"]
    assert out.dtype == F32 and (tout is None or tout.dtype == F32)
    return out, tout


# ------------------------------------------------------------------------------------------------ 2. timm 0.9.2, restated
def rand_bbox(img_shape, lam, margin=0., count=None):
    ratio = np.sqrt(1 - lam)
    img_h, img_w = img_shape[-2:]
    cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
    margin_y, margin_x = int(margin * cut_h), int(margin * cut_w)
    cy = np.random.randint(0 + margin_y, img_h - margin_y, size=count)
    cx = np.random.randint(0 + margin_x, img_w - margin_x, size=count)
    yl = np.clip(cy - cut_h // 2, 0, img_h)
    yh = np.clip(cy + cut_h // 2, 0, img_h)
    xl = np.clip(cx - cut_w // 2, 0, img_w)
    xh = np.clip(cx + cut_w // 2, 0, img_w)
    return yl, yh, xl, xh


def rand_bbox_minmax(img_shape, minmax, count=None):
    assert len(minmax) == 2
    img_h, img_w = img_shape[-2:]
    cut_h = np.random.randint(int(img_h * minmax[0]), int(img_h * minmax[1]), size=count)
    cut_w = np.random.randint(int(img_w * minmax[0]), int(img_w * minmax[1]), size=count)
    yl = np.random.randint(0, img_h - cut_h, size=count)
    xl = np.random.randint(0, img_w - cut_w, size=count)
    return yl, yl + cut_h, xl, xl + cut_w


def cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None):
    if ratio_minmax is not None:
        yl, yu, xl, xu = rand_bbox_minmax(img_shape, ratio_minmax, count=count)
    else:
        yl, yu, xl, xu = rand_bbox(img_shape, lam, count=count)
    if correct_lam or ratio_minmax is not None:
        bbox_area = (yu - yl) * (xu - xl)
        lam = 1. - bbox_area / float(img_shape[-2] * img_shape[-1])
    return (yl, yu, xl, xu), lam


class Mixup:
    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True

    def _params_per_batch(self):
        lam = 1.
        use_cutmix = False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand() < self.switch_prob
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.:
                use_cutmix = True
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                assert False, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
            lam = float(lam_mix)
        return lam, use_cutmix

    def _params_per_elem(self, batch_size):      # (the reference's TimmMixup overrides this one)
        raise NotImplementedError

    def _mix_elem(self, x):
        batch_size = len(x)
        lam_batch, use_cutmix = self._params_per_elem(batch_size)
        x_orig = x.clone()
        for i in range(batch_size):
            j = batch_size - i - 1
            lam = lam_batch[i]
            if lam != 1.:
                if use_cutmix[i]:
                    (yl, yh, xl, xh), lam = cutmix_bbox_and_lam(x[i].shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                    x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
                    lam_batch[i] = lam
                else:
                    x[i] = x[i] * lam + x_orig[j] * (1 - lam)
        return torch.tensor(lam_batch, device=x.device, dtype=x.dtype).unsqueeze(1)

    def _mix_pair(self, x):
        batch_size = len(x)
        lam_batch, use_cutmix = self._params_per_elem(batch_size // 2)
        x_orig = x.clone()
        for i in range(batch_size // 2):
            j = batch_size - i - 1
            lam = lam_batch[i]
            if lam != 1.:
                if use_cutmix[i]:
                    (yl, yh, xl, xh), lam = cutmix_bbox_and_lam(x[i].shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                    x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
                    x[j][:, yl:yh, xl:xh] = x_orig[i][:, yl:yh, xl:xh]
                    lam_batch[i] = lam
                else:
                    x[i] = x[i] * lam + x_orig[j] * (1 - lam)
                    x[j] = x[j] * lam + x_orig[i] * (1 - lam)
        lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
        return torch.tensor(lam_batch, device=x.device, dtype=x.dtype).unsqueeze(1)

    def _mix_batch(self, x):
        lam, use_cutmix = self._params_per_batch()
        if lam == 1.:
            return 1.
        if use_cutmix:
            (yl, yh, xl, xh), lam = cutmix_bbox_and_lam(x.shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        else:
            x_flipped = x.flip(0).mul_(1. - lam)
            x.mul_(lam).add_(x_flipped)
        return lam


# ------------------------------------------------------------------------------------------------ 3. the reference's file, restated
def mixup_target(target, num_classes, lam=1., smoothing=0.0):
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    y1 = (1 - target) * off_value + target * on_value
    return y1 * lam + y1.flip(0) * (1. - lam)


class TimmMixup(Mixup):
    @torch.no_grad()
    def __call__(self, x, target):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        lam = {'elem': self._mix_elem, 'pair': self._mix_pair}.get(self.mode, self._mix_batch)(x)
        return x, mixup_target(target, self.num_classes, lam, self.label_smoothing)

    def _params_per_elem(self, batch_size):
        lam = np.ones(batch_size, dtype=np.float32)
        use_cutmix = np.zeros(batch_size, dtype=bool)
        if not self.mixup_enabled:
            return lam, use_cutmix
        a_mix, a_cut = self.mixup_alpha, self.cutmix_alpha
        if a_mix > 0. and a_cut > 0.:
            use_cutmix = np.random.rand(batch_size) < self.switch_prob
            from_cut = np.random.beta(a_cut, a_cut, size=batch_size)        # both vectors are drawn, cutmix first
            from_mix = np.random.beta(a_mix, a_mix, size=batch_size)
            lam_mix = np.where(use_cutmix, from_cut, from_mix)
        elif a_mix > 0.:
            lam_mix = np.random.beta(a_mix, a_mix, size=batch_size)
        elif a_cut > 0.:
            use_cutmix = np.ones(batch_size, dtype=bool)
            lam_mix = np.random.beta(a_cut, a_cut, size=batch_size)
        else:
            assert False, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
        lam = np.where(np.random.rand(batch_size) < self.mix_prob, lam_mix.astype(np.float32), lam)       # the probability vector comes last
        return lam, use_cutmix
