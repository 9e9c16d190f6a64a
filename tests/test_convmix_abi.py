"""CPU: the C ABI of the depthwise 9x9 and the act-then-BN passes is bound (tests/test_abi.py checks every signature
against include/dmayolo.h), and the geometries the kernels do not take are refused before any launch."""
import pytest
import torch

CL = torch.channels_last
NEW = ('dmy_dwconv_fwd_actbn', 'dmy_actbn_stats', 'dmy_actbn_fwd', 'dmy_actbn_bwd_reduce', 'dmy_actbn_bwd_apply')


def test_new_entries_are_bound():
    from dmayolo import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert len(_lib.SIGNATURES['dmy_dwconv_fwd_actbn']) == len(_lib.SIGNATURES['dmy_dwconv_fwd_act'])


def test_header_cites_the_reference_lines():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dmayolo.h')).read()
    for name in NEW:
        i = hdr.index(f'int {name}(')
        assert 'models/cspcm.py:' in hdr[hdr.rindex('/*', 0, i):i], name


def test_dwconv_ok_admits_k9_stride1_only():
    """dmy_dwconv_ok is host arithmetic on the pointers' alignment and the geometry: no launch, no device"""
    from dmayolo.functional import call
    import ctypes
    p = ctypes.c_void_p(4096)
    ok = lambda dt, C, k, s, pad, H, OH: call('dmy_dwconv_ok', dt, p, p, p, 1, H, H, C, C, C, C, k, k, s, pad, OH, OH, C)  # noqa: E731
    assert ok(1, 16, 9, 1, 4, 12, 12) == 1 and ok(0, 4, 9, 1, 4, 3, 3) == 1
    assert ok(1, 16, 9, 2, 4, 12, 6) == 0      # stride 2
    assert ok(1, 12, 9, 1, 4, 12, 12) == 0     # 12 bf16 channels: not a whole vector
    assert ok(1, 16, 9, 1, 3, 12, 10) == 0     # padding other than 4
    assert ok(1, 16, 7, 1, 3, 12, 12) == 1 and ok(1, 16, 7, 2, 3, 12, 6) == 0  # unchanged
    assert ok(1, 16, 11, 1, 5, 12, 12) == 0


@pytest.mark.parametrize('C,s', [(16, 2), (12, 1)], ids=['stride2', 'ragged12'])
def test_k9_unsupported_geometry_raises_the_unchanged_message(C, s):
    """k = 9 at stride 2, and k = 9 with 12 bf16 channels: the unchanged NotImplementedError before any launch (a CPU
    tensor reaches it)"""
    from dmayolo import functional as Fn
    conv = torch.nn.Conv2d(C, C, 9, s, 4, groups=C)
    x = torch.zeros(1, C, 12, 12, dtype=torch.bfloat16).contiguous(memory_format=CL)
    bn = torch.nn.BatchNorm2d(C).eval()
    for fn in (Fn.conv_bn_act, Fn.conv_act_bn):
        with pytest.raises(NotImplementedError, match=r'grouped conv with groups != channels, or a depthwise geometry the '
                                                      r'gfx950 kernels do not take \(dmy_dwconv_ok\)'):
            with torch.no_grad():
                fn(x, conv.weight, conv.bias, bn, s, 4, Fn.ACT_GELU, spec=Fn.spec_for(conv, s, 4, Fn.ACT_GELU, bn))


def test_convmix_refusals():
    from dmayolo.models import common as P
    with pytest.raises(NotImplementedError, match=r'ConvMix: kernel_size=7'):
        P.ConvMix(64, 64, kernel_size=7)
    with pytest.raises(NotImplementedError, match=r'ConvMix: dim=6 '):
        P.ConvMix(6, 6)
    x = torch.zeros(1, 12, 8, 8, dtype=torch.bfloat16).contiguous(memory_format=CL)
    for mod in (P.ConvMix(12, 12), P.CSPCM(24, 24).m):
        with pytest.raises(NotImplementedError, match=r'ConvMix: 12 channels .*bfloat16'):
            mod(x)
