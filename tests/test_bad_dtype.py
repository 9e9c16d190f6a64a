"""Every entry whose storage-type dispatch goes through by_dtype (csrc/launch.h) refuses a dtype outside {0 = fp32,
1 = bf16}: hipErrorInvalidValue from the launch entries, 0 (-1 from dmy_conv_route) from the queries.  Each call has
dtype = 2, null pointers and every size zero, so an entry that tested the empty problem first, or ran dtype 2 as bf16,
would answer 0 and launch nothing.  The max-pool entries get the window k = 3, since they refuse k = 0 whatever the
dtype.  dmy_cast takes two such kinds and refuses a bad one in either place.  The calls go to the library directly:
_lib.call raises on a nonzero status."""
import pytest

INVALID = 1  # hipErrorInvalidValue

LAUNCH = [
    # conv.hip
    'dmy_conv_fwd', 'dmy_conv_fwd_act', 'dmy_conv_fwd_act_ws', 'dmy_conv_dgrad',
    # conv_wgrad.hip
    'dmy_conv_wgrad', 'dmy_conv_wgrad_ex', 'dmy_conv_wgrad_det', 'dmy_conv_wprep', 'dmy_conv_wprep_multi',
    'dmy_conv_wprep_s2d',
    # mha.hip
    'dmy_mha_fwd', 'dmy_mha_fwd_ref', 'dmy_mha_bwd', 'dmy_dropout',
    # swin.hip
    'dmy_layernorm_fwd', 'dmy_layernorm_bwd', 'dmy_winattn_fwd', 'dmy_winattn_bwd', 'dmy_droppath_add',
    'dmy_droppath_grad', 'dmy_sample_scale',
    # detect_loss.hip
    'dmy_detect_decode', 'dmy_detect_decode_levels', 'dmy_detect_decode_tta', 'dmy_yolo_loss_level',
    'dmy_yolo_loss_level_focal', 'dmy_loss_grad',
    # tal.hip
    'dmy_tal_loss', 'dmy_tal_flatten', 'dmy_tal_detect_out',
    # tta.hip
    'dmy_tta_image',
    # bn.hip
    'dmy_bn_stats', 'dmy_bn_act_fwd', 'dmy_bn_bwd_reduce', 'dmy_bn_bwd_apply',
    # eltwise.hip
    'dmy_maxpool_fwd', 'dmy_maxpool_chain3_fwd', 'dmy_maxpool_bwd', 'dmy_avgpool_fwd', 'dmy_avgpool_bwd',
    'dmy_resize_fwd', 'dmy_resize_bwd', 'dmy_space_to_depth', 'dmy_gpool_fwd', 'dmy_gpool_bwd', 'dmy_halves_sigmoid',
    'dmy_cbam_in_fwd', 'dmy_cbam_in_bwd', 'dmy_pixscale', 'dmy_slice_copy', 'dmy_dot_partial', 'dmy_slice_copy_dot',
    'dmy_scgate_fwd', 'dmy_scgate_bwd', 'dmy_ca_pool_fwd', 'dmy_ca_pool_bwd', 'dmy_ca_apply_fwd', 'dmy_ca_apply_bwd',
    'dmy_image_s2d', 'dmy_nchw_to_nhwc', 'dmy_nhwc_to_nchw_f32', 'dmy_pointwise',
]
QUERY = [('dmy_conv_fwd_bn_rows', 0), ('dmy_conv_fwd_splitk_elems', 0), ('dmy_conv_wgrad_ws_elems', 0),
         ('dmy_conv_route', -1), ('dmy_bn_reduce_rows', 0)]


def _call(name, dtype_at=0):
    from dmayolo import _lib
    args = [None if t is _lib.P else t(0).value for t in _lib.SIGNATURES[name]]
    args[dtype_at] = 2
    if name.startswith('dmy_maxpool_'):
        args[-2] = 3  # k, the last argument before the stream
    return getattr(_lib.lib, name)(*args)


@pytest.mark.parametrize('name', LAUNCH)
def test_launch_entry_refuses_dtype_2(name):
    assert _call(name) == INVALID


@pytest.mark.parametrize('at', [0, 1])
def test_cast_refuses_kind_2_as_source_and_as_destination(at):
    assert _call('dmy_cast', at) == INVALID


@pytest.mark.parametrize('name,want', QUERY)
def test_query_entry_answers_nothing_for_dtype_2(name, want):
    assert _call(name, 1 if name == 'dmy_conv_route' else 0) == want
