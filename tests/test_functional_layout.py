"""CPU: dmayolo.functional is a package of one module per concern (dmayolo/functional/__init__.py lists them) that
still offers every name the single-file module had, shares its switches and classes by identity, imports in any order,
and whose launches all pass _lib.call's one observer hook.  Needs the built library (like test_abi.py); no GPU."""
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'dma-yolo_amd')

# sorted(n for n in dir(dmayolo.functional) if not n.startswith('__')) of the last single-file functional.py
FROZEN = """
ACT_GELU ACT_HARDSWISH ACT_LEAKY ACT_NONE ACT_RELU ACT_SIGMOID ACT_SILU AdaptAddFn AdaptGateFn AddFn AvgPoolFn
BWD1X1 BnLink CAApplyFn CAPoolFn CBAMInFn CL ConcatFn ConvActBNFn ConvBNActFn ConvGeom ConvSpec DEFER_AFFINE
DETERMINISTIC DT DropPathAddFn DropoutFn F8Emit F8_DELAYED F8_HEADROOM FlattenLevelsFn GPoolFn GateMulFn
GradSink HalvesSigmoidFn KernelTimer LayerNormFn LayerScaleAddFn MHAFn MaxPool2Fn MaxPoolFn PARAM_GEN PixScaleFn
ResizeFn SCGateFn SampleScaleFn SliceSink SpaceToDepthFn SpdSplitFn SplitFn ToNHWC VW WGRAD_OIHW WGRAD_ZEROED
WeightPrep WgradArena WinAttnFn _CONST _DROP_STATE _F8_WS _PSPECS _SPECS _SlicePart _act_bias_bwd _act_pass
_actbn_infer _actbn_stats _bn_bwd_coef _bwd1x1 _conv_bn_stats _conv_fp8 _conv_infer _conv_infer_spd
_conv_operands _conv_wgrad _defer_affine _dgrad _dw_bias_in_wgrad _dw_check _dw_operands _dw_unsupported _f8_ws
_fold_partials _fp8_operands _fp8_weight _image_src _inplace_concat _launch_conv_fwd _launch_dw_fwd _lib _lv3
_param_spec _pgrad _sample_major _save_ctx _seed _spd_shape _wgrad _wgrad_target _write_target call
concat_buffer const_vec conv_act_bn conv_bn_act conv_out_hw ctypes_off dcode eval_coef even_hw f32 f8_saturation
fp8_eligible image_s2d maxpool_chain3 namedtuple new_act os out_view pixel_stride prep_weight ptr
set_deterministic set_fp8 sink_result sink_target spec_for stream torch tta_image vec_check vec_ok vec_pad
vec_view weakref zero_padded_channels
""".split()

SUBMODULES = ['_base', 'sinks', 'timer', 'fp8', 'spd', 'conv', 'convmix', 'pool', 'attention', 'image', 'swin',
              'adapt', 'hor']
# the mutable switches and the module that defines each
SWITCHES = {'DETERMINISTIC': 'conv', 'DEFER_AFFINE': 'conv', 'BWD1X1': 'conv', 'PARAM_GEN': 'conv',
            'F8_DELAYED': 'fp8', 'F8_HEADROOM': 'fp8'}


def _sub(name):
    return importlib.import_module('dmayolo.functional.' + name)


def test_package_replaces_the_single_file():
    import dmayolo.functional as Fn
    assert len(FROZEN) == 136
    assert not os.path.exists(os.path.join(PKG, 'dmayolo', 'functional.py'))
    assert os.path.basename(Fn.__file__) == '__init__.py'
    have = {n for n in dir(Fn) if not n.startswith('__')}
    assert not set(FROZEN) - have, sorted(set(FROZEN) - have)
    files = os.listdir(os.path.dirname(Fn.__file__))
    on_disk = sorted(f[:-3] for f in files if f.endswith('.py') and f != '__init__.py')
    assert on_disk == sorted(SUBMODULES)


def test_switches_are_shared_by_identity():
    import dmayolo.functional as Fn
    import dmayolo.optim
    from dmayolo import _lib
    for name, mod in SWITCHES.items():
        x = getattr(Fn, name)
        assert type(x) is list and len(x) == 1, name
        assert x is getattr(_sub(mod), name), name
    assert dmayolo.optim.PARAM_GEN is Fn.PARAM_GEN
    assert Fn._lib is _lib and Fn.call is _lib.call and Fn.ptr is _lib.ptr and Fn.stream is _lib.stream
    # class-level state lives on the one class object
    assert Fn.WeightPrep is _sub('conv').WeightPrep and 'current' in vars(Fn.WeightPrep)
    assert Fn.WgradArena is _sub('conv').WgradArena and 'current' in vars(Fn.WgradArena)
    assert _sub('adapt').WgradArena is Fn.WgradArena


def test_every_name_is_its_submodules_object():
    """each function / class of the frozen list is defined in exactly one submodule and `Fn.X` is that object: no
    second copy from a double import, no stale re-definition in __init__"""
    import types
    import dmayolo.functional as Fn
    import torch
    mods = {'dmayolo.functional.' + s: _sub(s) for s in SUBMODULES}
    checked = 0
    for name in FROZEN:
        x = getattr(Fn, name)
        if not isinstance(x, (type, types.FunctionType)) or not x.__module__.startswith('dmayolo.'):
            continue
        if x.__module__ == 'dmayolo._lib':
            continue
        assert x.__module__ in mods, (name, x.__module__)
        assert getattr(mods[x.__module__], name) is x, name
        assert sys.modules[x.__module__] is mods[x.__module__]
        holders = [m for m in mods if vars(mods[m]).get(name) is not None and
                   getattr(vars(mods[m])[name], '__module__', None) == m]
        assert holders == [x.__module__], (name, holders)
        checked += 1
    fns = [n for n in FROZEN
           if isinstance(getattr(Fn, n), type) and issubclass(getattr(Fn, n), torch.autograd.Function)]
    assert len(fns) == 30 and checked == 105, (len(fns), checked)  # the single file's 30 Functions, 105 defs
    # a name imported across submodules is the same object everywhere it is visible
    for m in mods.values():
        for name in FROZEN:
            if name in vars(m) and name not in ('os', 'torch', 'weakref', 'namedtuple'):
                assert vars(m)[name] is getattr(Fn, name), (m.__name__, name)


@pytest.mark.parametrize('name', SUBMODULES)
def test_submodule_imports_alone(name):
    """a fresh interpreter importing only this submodule: no import cycle that a lucky import order hides"""
    code = ('import sys; sys.path.insert(0, %r); import importlib; '
            'm = importlib.import_module("dmayolo.functional.%s"); print(m.__name__)' % (PKG, name))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().endswith('dmayolo.functional.' + name)


def test_no_function_local_imports_of_the_package():
    """the dependency order is the import order: no submodule imports a sibling (or the package) inside a function"""
    import ast
    for s in SUBMODULES + ['__init__']:
        path = os.path.join(PKG, 'dmayolo', 'functional', s + '.py')
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level > 0:
                assert node in tree.body, (s, node.lineno)


def test_trace_hook_sees_every_call():
    """_lib.TRACE[0] is given the symbol name and the arguments of every _lib.call, through whichever module imported
    `call` (dmy_bn_partial_rows is a host-only query: no GPU needed); reset to None it records nothing"""
    from dmayolo import _lib
    import dmayolo.functional as Fn
    from dmayolo.functional import conv
    from dmayolo.utils import general
    assert _lib.TRACE == [None]
    seen = []
    _lib.TRACE[0] = lambda name, args: seen.append((name, args))
    try:
        rows = _lib.call('dmy_bn_partial_rows', 4096)
        assert seen == [('dmy_bn_partial_rows', (4096,))] and rows > 0
        for c in (Fn.call, conv.call, general.call, Fn.KernelTimer.run.__globals__['call']):
            assert c('dmy_bn_partial_rows', 4096) == rows
        assert seen == [('dmy_bn_partial_rows', (4096,))] * 5
    finally:
        _lib.TRACE[0] = None
    assert _lib.call('dmy_bn_partial_rows', 4096) == rows
    assert len(seen) == 5
