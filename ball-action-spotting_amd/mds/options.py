"""The switches of a launch plan as two frozen records: PlanOptions (the user switches of MultiDimStacker, part of the plan-cache key)
and DevSwitches (the MDS_* developer variables, read once per plan build)."""
from __future__ import annotations

import dataclasses
import os


@dataclasses.dataclass(frozen=True)
class PlanOptions:
    """One element of the plan-cache key and the `options` argument of engine.Plan.  The module keeps the switches as plain
    attributes; a new switch is one field here plus its gate line in Plan.__init__."""
    eval_fusion: bool = False
    eval_se_fusion: bool = False
    eval_er_fusion: bool = False
    deterministic: bool = False
    device_rng: bool = False

    @classmethod
    def of(cls, module, training, need_grad):
        """the module's switches as the cache key sees them.  The two gates below decide what the KEY distinguishes (the three
        eval_* switches go in ungated); Plan.__init__ repeats them, and adds eval_epilogues, for the plan's effective values."""
        o = cls(*(bool(getattr(module, f.name, False)) for f in dataclasses.fields(cls)))      # (unpickled from before a switch existed: off)
        # plans without a backward schedule ignore `deterministic`; eval plans have no masks for `device_rng`
        return dataclasses.replace(o, deterministic=o.deterministic and bool(need_grad), device_rng=o.device_rng and bool(training))


# The MDS_* developer switches (README: A/B timing only) as field=(variable, default, parse of the variable's text).  Plan.__init__ reads
# them once into plan.dev: nothing on the launch path looks at the environment.  They are not part of the plan-cache key.
_ON, _NOT0 = (lambda v: v == "1"), (lambda v: v != "0")
_DEV = dict(fuse_bn_bwd=("MDS_FUSE_BN_BWD", "1", _NOT0), eval_epi=("MDS_EVAL_EPI", "1", _ON), se_params_table=("MDS_SE_PARAMS_TABLE", "1", _ON),
            fuse_conv_post=("MDS_FUSE_CONV_POST", "0", _ON), fuse_conv_post_silu=("MDS_FUSE_CONV_POST_SILU", "1", _ON),
            eval_pool=("MDS_EVAL_POOL", "1", _ON), se_act=("MDS_SE_ACT", "0", _ON), stem_dyp=("MDS_STEM_DYP", "1", _ON),
            side_stream=("MDS_SIDE_STREAM", "1", _NOT0), stop_events=("MDS_SIDE_EVENTS", "stop", lambda v: v == "stop"),
            event_flags=("MDS_EVENT_FLAGS", "0x20000002", lambda v: int(v, 0)), hip_memset=("MDS_MEMSET", "hip", lambda v: v == "hip"))
DevSwitches = dataclasses.make_dataclass("DevSwitches", [(f, type(p(d)), dataclasses.field(default=p(d))) for f, (_, d, p) in _DEV.items()], frozen=True)
DevSwitches.from_env = classmethod(lambda cls: cls(**{f: p(os.environ.get(v, d)) for f, (v, d, p) in _DEV.items()}))
