"""GPU: the tail split of the table-gradient scatter GEMM (csrc/nr_gemm.hip, gemm_nt_dma_kernel<EPI_SCATTER, 20, false, 4> mapped
by csrc/nr_scatter_tail.h): the 256-row tiles of the last, partly filled round of R = CU-count tiles are split over K among up to
8 workgroups each, and every part scatters its partial sums.

Driven like the sorted-scatter tests of tests/test_gpu_gemm_wreg.py (ops.mhsa with ids / table, p_in = 0.2) and compared, at
their tolerance (2e-3 of the reference's largest value), with the references they use -- batch order (`NO_SCATTER_SORT` = 1)
and the tiled projection (`NT_WREG` = 0) -- and with the deterministic mode, whose fixed-point scatter never splits a tile.

Live-row counts (rows with a non-zero token id), written for R = 256 and valid checks for any R:
  1 920   T = 8 tiles < R: the capped split, 8 parts per tile, and a last tile of 128 rows
  65 536  T = R exactly: nothing to split
  65 537  T = R + 1: one tile of ONE row in 8 parts
  65 636  T = R + 1, 100 rows in the tail tile (no multiple of 256)
"""
import pytest
import torch

from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _opt:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _lib.get_option(self.name)
        _lib.set_option(self.name, self.value)

    def __exit__(self, *a):
        _lib.set_option(self.name, self.old)


@pytest.mark.parametrize("n,live", [(160, 1920), (2200, 65536), (2200, 65537), (2200, 65636)])
def test_table_gradient_with_the_last_round_split_over_k(n, live):
    L, V, D, heads, dh = 30, 997, 300, 20, 20
    g = torch.Generator(device=DEV).manual_seed(n + live)
    cpu = torch.Generator().manual_seed(n + live)
    ids = torch.randint(1, V, (n * L,), device=DEV, generator=g, dtype=torch.int32)
    ids[torch.randperm(n * L, generator=cpu)[:n * L - live].to(DEV)] = 0
    ids = ids.view(n, L)
    assert int((ids != 0).sum()) == live
    table = torch.randn(V, D, device=DEV, generator=g) * 0.4
    table[0] = 0
    table.requires_grad_(True)
    N = heads * dh
    ws = [(torch.randn(N, D, device=DEV, generator=g) * 0.05).requires_grad_(True) for _ in range(3)]
    bs = [(torch.randn(N, device=DEV, generator=g) * 0.05).requires_grad_(True) for _ in range(3)]
    gy = (torch.randn(n, L, N, device=DEV, generator=g) * 0.1).to(torch.bfloat16)

    def run():
        torch.manual_seed(5)                                   # the dropout seeds are drawn from torch's CPU generator
        for p in [table] + ws + bs:
            p.grad = None
        _lib.prof_enable(1)
        try:
            _lib.prof_collect()
            y = ops.mhsa(None, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], heads=heads, code=ops.NR_BF16, ids=ids, table=table,
                         p_in=0.2, p_out=0.2)
            y.backward(gy)
            torch.cuda.synchronize()
            labels = set(_lib.prof_collect().keys())
        finally:
            _lib.prof_enable(0)
        return labels, table.grad.clone()

    labels, got = run()
    assert any(l.startswith("gemm_nt_dma_live[bf16,epi=2") for l in labels), labels     # the compact scatter on the LDS-DMA kernel
    with _opt("NT_WREG", 0):
        _, tiled = run()
    with _opt("NO_SCATTER_SORT", 1):
        _, unsorted = run()
    ops.set_deterministic(True, elements=1 << 22)
    try:
        _, whole = run()
    finally:
        ops.set_deterministic(False)
    assert torch.isfinite(got).all()
    assert got[0].abs().max().item() == 0.0                    # padding_idx row gets no gradient
    for name, ref in (("tiled", tiled), ("unsorted", unsorted), ("deterministic", whole)):
        scale = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        print(f"n={n} live={live} vs {name}: err {err:.3e} tol {2e-3 * scale + 1e-7:.3e}")
        assert scale > 0 and err <= 2e-3 * scale + 1e-7, (name, err, scale)
