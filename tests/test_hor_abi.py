"""CPU: the entries csrc/hor.hip adds to the C ABI (gate product, layer-scaled residual) are declared in
include/dmayolo.h and bound in dmayolo/_lib.py, and the host-only row query answers without a GPU."""
from test_abi import header_decls

NEW = ('dmy_gate_fwd', 'dmy_gate_bwd', 'dmy_layerscale_fwd', 'dmy_layerscale_bwd_rows', 'dmy_layerscale_bwd')


def test_new_entries_are_declared_and_bound():
    from dmayolo import _lib
    decls = header_decls()
    for name in NEW:
        assert name in decls, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert len(_lib.SIGNATURES[name]) == len(decls[name][1]), name


def test_layerscale_rows_query():
    """one partial row per 32 pixels, capped: the GPU test's M = 70 and 4099 give >= 3 rows that do not divide M"""
    from dmayolo import _lib
    rows = _lib.lib.dmy_layerscale_bwd_rows
    assert rows(0) == 0 and rows(1) == 1 and rows(70) == 3 and rows(4099) == 129 and rows(1 << 30) == 2048
    assert 70 % 3 and 4099 % 129
