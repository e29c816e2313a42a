"""CPU: libnrhip.so loads and exports every symbol include/nrhip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from newsrecommendation_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "nrhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const int32_t\*)\s+(nr_[a-z0-9_]+)\s*\(", src)))


def test_header_matches_binding_table():
    assert declared_symbols() == sorted(_lib.SIGNATURES)


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), f"libnrhip.so does not export {name}"
    assert _lib.lib().nr_version() >= 100


def test_no_cpu_fallback():
    """Ops refuse CPU tensors instead of silently computing elsewhere."""
    import torch
    from newsrecommendation_amd import ops
    x = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pad_blend(x, None, None, ops.dtype_code("fp32"))


def test_descriptor_layout_and_workspace_sizes_are_host_arithmetic():
    """The binding checks sizeof() of every descriptor against the library at load; the workspace sizes come from the
    library (no hand-copied formulas in ops.py) and grow with the problem."""
    import ctypes as C
    lib = _lib.lib()                                        # raises on a layout mismatch
    d = _lib.MhsaDesc(n=28160, L=30)
    b = lib.nr_mhsa_workspace_bytes(C.byref(d))
    M = 28160 * 30
    assert b >= 4 * (3 * M + 3 * 28160 + M // 32) and b < 4 * (3 * M + 4 * 28160 + M // 32 + 64)
    d2 = _lib.MhsaDesc(n=28161, L=30)
    assert lib.nr_mhsa_workspace_bytes(C.byref(d2)) > b
    assert lib.nr_conv_workspace_bytes(C.byref(_lib.ConvDesc(n=28160, T=30))) >= 4 * (28160 + M // 32)
    p = _lib.PoolDesc(n=28160, L=30, q=200)
    assert lib.nr_pool_workspace_bytes(C.byref(p)) >= 4 * (28160 + M // 32)
    assert lib.nr_linear_workspace_bytes(C.byref(_lib.LinearDesc(M=100, N=400, dtype=_lib.NR_BF16))) == 100 * 400 * 2


def test_option_table_holds_the_reference_switches():
    """The switches the GPU tests use to run a reference path: production defaults, readable and settable by name;
    an unknown name reads -1."""
    defaults = {"NO_SLABS": 0, "NT_WREG": 1, "NO_SCATTER_SORT": 0, "NO_COMPACT_ROWS": 0, "NO_POOL_FUSED": 0}
    assert {k: _lib.get_option(k) for k in defaults} == defaults
    assert _lib.get_option("NR_NT_WREG") == 1 and _lib.get_option("NO_SUCH_OPTION") == -1
    _lib.set_option("NO_SLABS", 1)
    assert _lib.get_option("NO_SLABS") == 1
    _lib.set_option("NO_SLABS", 0)


RETIRED_OPTIONS = ["NO_ATTN_SKIP", "SIDE_STREAM", "ATTN_OLD", "ATTN_VALU", "NO_PAD_SUB", "NO_FUSED_FWD", "NO_TN3", "TN_V1",
                   "TN3_ROUNDS", "TN3_WK", "TN3_NI", "NT_NOWIDE", "NT_NODMA", "DMA_MIN_K", "DMA_WM2_ALL", "ATTN_PRED",
                   "ATTN_GENERIC", "NO_ROW_SUB", "ATTN_BWD_OCC4", "NT_ABLATE", "TN3_MIN_M", "ATTN_BWD_GRID", "TN3_ATOMIC",
                   "TN3_ABLATE", "POOL_ABLATE"]


@pytest.mark.parametrize("name", RETIRED_OPTIONS)
def test_retired_option_is_unknown(name):
    """Switches for superseded or measurement-only paths are gone from the option table: unknown to get and set."""
    assert _lib.get_option(name) == -1
    with pytest.raises(RuntimeError, match="unknown option"):
        _lib.set_option(name, 1)


def test_undersized_workspace_is_refused_before_any_launch():
    """The library validates caller-stated workspace sizes against its own formulas (host check, no GPU work)."""
    import ctypes as C
    lib = _lib.lib()
    d = _lib.MhsaDesc(n=64, L=30, d_model=304, heads=20, d_head=20, dtype=_lib.NR_BF16, src_kind=_lib.NR_SRC_GATHER, x=16, ldx=320,
                      ids=16, w_qkv=16, ldw=320, b_qkv=16, x_rows=16, ld_rows=304, row_ws=16, row_ws_bytes=64)
    rc = lib.nr_mhsa_fwd(C.byref(d), 16, 16, None)
    assert rc == 1 and "nr_mhsa_workspace_bytes" in _lib.last_error()
    p = _lib.PoolDesc(n=64, L=30, N=400, q=200, dtype=_lib.NR_BF16, x=16, w1=16, ldw1=400, b1=16, w2=16, b2=16, partial_bytes=8)
    rc = lib.nr_additive_pool_bwd(C.byref(p), 16, 16, 16, 400, 16, 200, 16, 16, 16, 16, 16, 16, None, None)
    assert rc == 1 and "nr_pool_workspace_bytes" in _lib.last_error()


def _mind_title_desc(**changes):
    """The MIND title-level training descriptor (bf16, gather source, rows kept, scratch given) with fake non-null pointers;
    row_ws_bytes is what the library asks for after the changes."""
    import ctypes as C
    f = dict(n=28160, L=30, d_model=300, heads=20, d_head=20, dtype=_lib.NR_BF16, src_kind=_lib.NR_SRC_GATHER, x=4096, ldx=304,
             ids=4096, w_qkv=4096, ldw=304, b_qkv=4096, x_rows=4096, ld_rows=304, row_ws=4096, table_rows=30000)
    f.update(changes)
    d = _lib.MhsaDesc(**f)
    need = _lib.lib().nr_mhsa_workspace_bytes(C.byref(d))
    assert need > 0
    d.row_ws_bytes = need
    return d


COMPACT_ROWS_OFF = {"fp32": dict(dtype=_lib.NR_F32), "dense_source": dict(src_kind=_lib.NR_SRC_DENSE, ids=None),
                    "no_x_rows": dict(x_rows=None), "no_row_ws": dict(row_ws=None), "no_table_rows": dict(table_rows=0),
                    "M_below_4096": dict(n=128), "M_not_multiple_of_32": dict(n=28161), "L_32": dict(L=32),
                    "ld_rows_below_Kp": dict(ld_rows=296)}


def test_compact_rows_plan_over_a_descriptor_grid():
    """nr_mhsa_compact_rows is the exported face of the MHSA training plan: 1 for the MIND title shape in bf16, and 0 when any
    single term of the plan is taken away -- each descriptor still passes the argument check (a workspace size > 0 and a
    row_ws_bytes of that size), so every zero comes from its own term.  Host arithmetic only."""
    import ctypes as C
    lib = _lib.lib()
    assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc())) == 1
    assert lib.nr_mhsa_compact_rows(None) == 0
    for name, change in COMPACT_ROWS_OFF.items():
        assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc(**change))) == 0, name
    # the neighbours on the permitted side of each bound still store compactly; an empty batch stores nothing
    assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc(n=0))) == 0
    assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc(L=31))) == 1
    assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc(ld_rows=312))) == 1
    for opt in ("NO_COMPACT_ROWS", "NO_SLABS", "NO_SCATTER_SORT"):
        _lib.set_option(opt, 1)
        try:
            assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc())) == 0, opt
        finally:
            _lib.set_option(opt, 0)
        assert lib.nr_mhsa_compact_rows(C.byref(_mind_title_desc())) == 1, opt
