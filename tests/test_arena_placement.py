"""Arena-style placement: one case per operator, at the smallest shape its own test has, with the buffers that mds/engine.py
sub-allocates DENSELY sitting at a 4-byte-only address (Backend.arena -> align=4: address = 4 mod 16), guard bands on both sides.

Which pointer fields can be sub-slices (mds/engine.py: Lazy.sub through Plan.grad / Plan.mask / Plan.zero_*64, and carve):
  - Plan.grad(p): grad_arena at Plan.poff[p] - a running sum of numel() over module.parameters(), so any 4-byte offset; e.g.
    global_pool.p (ONE float) precedes classifier.weight and classifier.bias in every training plan:
        mds_pw_wgrad_args.dw, mds_conv_wgrad_args.dw, mds_stem_wgrad_args.dw, mds_dw_bwd_args.dw,
        mds_bn_bwd_finalize_args.dgamma / dbeta, mds_se_fc_bwd_args.dw1 / db1 / dw2 / db2 (se_fc_bwd_params and the table),
        mds_gem_bwd_args.dp, mds_head_bwd_args.dw / db
  - Plan.mask(n, rate): mask_arena, sub-buffers `groups` (DropPath) or B * F (dropout) floats apart - an odd image count gives a
    4-byte offset: mds_bn_res_args.mask, mds_gsrc_t.mask, mds_poststat_t.mask, mds_head_fwd_args.mask / mds_head_bwd_args.mask
  - Plan.zero_fwd64 / zero_bwd64 (fp64): BatchNorm sums (SLOTS * 2 * C doubles), squeeze-excite pooled / dgate (groups * mid), GeM
    accum (B * S * cq) - C, mid and cq are multiples of 8, so every offset is a multiple of 64 bytes: no fp64 sub-buffer can sit
    at 8 mod 16, and no case here puts one there
  - BNL.buf.sub (scale | shift | mean | rstd, C floats apart) and the arenas themselves (carve: 256-byte boundaries): 16-byte
    aligned by construction
The cases run the operator's own test body - same inputs, same reference, same tolerance - inside Backend.arena(names), which
places the buffers those tests allocate under these names and fails if one of the names was never allocated."""
import pytest

import test_k_conv
import test_k_dw_stem
import test_k_elem
import test_k_pw
from backends import be  # noqa: F401


def test_arena_places_at_4_mod_16(be):
    import torch
    with be.arena("dw", "mask"):
        dw, mask, y = be.out((3, 5), torch.float32, 0, name="dw"), be.t(torch.ones(3), name="mask"), be.out(8, torch.float32, 0, name="y")
    assert dw.data_ptr() % 16 == 4 and mask.data_ptr() % 16 == 4 and y.data_ptr() % 32 == 16
    with pytest.raises(AssertionError, match="no buffer named"):
        with be.arena("dq"):
            pass
    be.sync()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pw_wgrad_dw(be, dt):
    with be.arena("dw"):
        test_k_pw.test_pw_wgrad(be, dt, 64, 192, 16, 1)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pw_fwd_poststat_mask(be, dt):
    """MDS_POST_MASK: the next layer's DropPath mask read in a data-gradient GEMM's epilogue"""
    with be.arena("mask"):
        test_k_pw.test_pw_fwd_bn_backward_fusion(be, dt, 260, 96, 144, 3, True, 2)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_conv_wgrad_dw(be, dt):
    with be.arena("dw"):
        test_k_conv.test_conv_wgrad(be, dt, 1, 9, 18, 48, 192, 1, 0)


def test_c3w_row_streaming_dw(be):
    """the same shape class through k_c3.hip's weight-gradient kernel (OIHW flush through LDS)"""
    with be.arena("dw"):
        test_k_conv.test_c3w_weight_gradient_row_streaming(be, 1, 1, 16, 48, 192, 0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stem_wgrad_dw(be, dt):
    with be.arena("dw"):
        test_k_dw_stem.test_stem_fwd_wgrad(be, dt, 1, 17, 23)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 1, 9, 13, 48, 1, 1), (1, 1, 12, 18, 16, 2, 1), (3, 2, 5, 6, 16, 1, 3)])      # 3x3 stride 1 / 2, 3x3x3
def test_dw_bwd_dw(be, dt, case):
    with be.arena("dw"):
        test_k_dw_stem.test_dw_fwd_bwd(be, dt, *case)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_bwd_finalize_parameter_gradients_and_gsrc_mask(be, dt):
    """dgamma / dbeta in the gradient arena; MDS_G_MASK: the DropPath mask through mds_gsrc_t.mask in the reduce and apply passes"""
    with be.arena("dgamma", "dbeta", "mask"):
        test_k_elem.test_bn_backward_chain(be, dt, 3, 40)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_res_mask(be, dt):
    """the DropPath mask on the residual path"""
    with be.arena("mask"):
        test_k_elem.test_bn_res(be, dt, 300, 16, 0, True, True)


def test_se_fc_bwd_params_and_table(be):
    with be.arena("dw1", "db1", "dw2", "db2"):
        test_k_elem.test_se_parameter_gradients_table_equals_the_per_layer_launches(be)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gem_bwd_dp(be, dt, golden):
    with be.arena("dp"):
        test_k_elem.test_gem_fwd_bwd(be, dt, 0, False, 35, 16, golden)


def test_head_bwd_behind_gems_one_float(be):
    """the production case: classifier.weight / .bias gradients follow global_pool.p's one float; the dropout mask follows the
    DropPath masks"""
    with be.arena("dw", "db", "mask"):
        test_k_elem.test_head_fwd_bwd(be)
