"""CPU: host-side contract of the trainable-title-table entry point (nr_conv1d_k3_bwd_table): the workspace size is host
arithmetic that grows with the problem, and bad arguments are refused before any launch (no GPU is touched)."""
import ctypes as C

from newsrecommendation_amd import _lib


def _desc(n, V=65001, dtype=_lib.NR_BF16):
    return _lib.ConvDesc(n=n, T=30, D=300, Dp=320, N=400, dtype=dtype, table_rows=V, ids_stride=1)


def test_table_workspace_grows_with_n_and_covers_its_buffers():
    lib = _lib.lib()
    sizes = [lib.nr_conv_table_workspace_bytes(C.byref(_desc(n))) for n in (0, 1, 7040, 28160, 28161)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    n = 28160
    # the staged dy (a zero row between titles) and dx, both bf16, plus the int32 lists and the id histogram
    assert sizes[3] >= (n * 31 + 1) * 400 * 2 + n * 30 * 304 * 2 + 4 * (7 * n + 65001 + n * 30)
    assert lib.nr_conv_table_workspace_bytes(C.byref(_desc(n, dtype=_lib.NR_F32))) > sizes[3]
    assert lib.nr_conv_table_workspace_bytes(C.byref(_desc(n, V=131072))) > sizes[3]
    assert lib.nr_conv_table_workspace_bytes(C.byref(_desc(n, V=0))) == 0          # table_rows is required


def test_undersized_table_workspace_is_refused_before_any_launch():
    """Non-null but bogus pointers: the call must fail on the host size check, not dereference anything."""
    lib = _lib.lib()
    d = _desc(7040)
    d.ids = 0x1000
    need = lib.nr_conv_table_workspace_bytes(C.byref(d))
    rc = lib.nr_conv1d_k3_bwd_table(C.byref(d), 0x1000, 0x1000, 1216, 0x1000, 0x1000, need - 1, None)
    assert rc != 0
    msg = _lib.last_error()
    assert "nr_conv_table_workspace_bytes" in msg and str(need) in msg, msg


def test_table_rows_beyond_31_bit_row_numbers_are_refused():
    lib = _lib.lib()
    d = _desc(64, V=2 ** 31 // 30 + 1)
    d.ids = 0x1000
    rc = lib.nr_conv1d_k3_bwd_table(C.byref(d), 0x1000, 0x1000, 1216, 0x1000, 0x1000, 1 << 40, None)
    assert rc != 0 and "31 bits" in _lib.last_error()
    d = _desc(64, V=0)
    d.ids = 0x1000
    assert lib.nr_conv1d_k3_bwd_table(C.byref(d), 0x1000, 0x1000, 1216, 0x1000, 0x1000, 1 << 40, None) != 0
    assert "table_rows" in _lib.last_error()
