"""CPU: the entries the depthwise 7x7 with bias adds to the C ABI are bound, and the 7x7 depthwise geometries that
still have no kernel raise the unchanged NotImplementedError before any launch."""
import pytest
import torch

CL = torch.channels_last


def test_new_entries_are_bound():
    from dmayolo import _lib
    for name in ('dmy_dwconv_wgrad_bias', 'dmy_dwconv_wgrad_bias_finalize'):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name


class _Owner(torch.nn.Module):
    def __init__(self, groups):
        super().__init__()
        self.groups = groups


@pytest.mark.parametrize('C,s,dtype', [(16, 2, torch.float32), (12, 1, torch.bfloat16), (6, 1, torch.float32)],
                         ids=['stride2', 'bf16-12ch', 'fp32-6ch'])
def test_dw7_geometries_without_a_kernel_still_raise(C, s, dtype):
    from dmayolo.functional import conv_bn_act, spec_for, ACT_NONE
    x = torch.zeros(1, C, 8, 8, dtype=dtype).contiguous(memory_format=CL)
    w, b = torch.zeros(C, 1, 7, 7), torch.zeros(C)
    with pytest.raises(NotImplementedError, match='grouped conv with groups != channels'):
        conv_bn_act(x, w, b, None, s, 3, ACT_NONE, spec=spec_for(_Owner(C), s, 3, ACT_NONE, None))

