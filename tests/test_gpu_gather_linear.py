"""GPU: ops.gather_linear (nr_linear_fwd / nr_linear_bwd: Embedding(padding_idx = 0) -> Linear of the category views) against
fp64, forward and backward, both dtypes, on the two input layers of the GEMM sweep (the first part of
tests/test_gpu_gemm_sweep.py, "GEMM building-block sweep").

  out = emb[ids] . w^T + b          dW = dout^T . emb[ids]     db = column sums of dout
  dtable[id] += dout . w  for id != 0; row 0 (padding_idx) gets exactly zero

It covers what the dense-row sweep cannot reach: the gather row source of the tiled NT and TN kernels (rows=1) and the
non-compacted SCATTER epilogue on its three routes -- the "wide" kernel (K <= 208), the LDS-DMA kernel (N rounded up to a
chunk >= 192 and a multiple of 32, so that w^T needs no padding) and the tiled kernel otherwise; fp32 always takes the tiled
one.  ids: a mix with zeros, one id for every row, all zeros, and a strided view (a column of an [M, 3] tensor).

lattice: integer operands, every result an exact integer -> bit-equal to fp64.  layer2: Gaussian operands rounded to the
compute dtype, a bf16-representable dout (the backward casts it to the compute dtype); bounds as in that file with
T = K products (forward), M (dW, db) and N + M (dtable: N products per row, at most M rows added into one table row by fp32
atomics, each addition one rounding of a partial sum that S bounds).
"""
import pytest
import torch

import test_gpu_gemm_sweep as H
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        K    N     M     V   ids        (bf16 scatter route)
SHAPES = [(8, 12, 1, 2, "mixed"),        # wide
          (100, 100, 129, 19, "same"),   # wide
          (216, 400, 1000, 300, "mixed"),  # tiled
          (8, 192, 129, 19, "strided"),  # dma
          (216, 192, 1000, 300, "mixed"),  # dma
          (100, 400, 1000, 300, "zeros"),  # wide
          (216, 12, 129, 2, "same"),     # tiled
          (100, 192, 1, 19, "mixed"),    # dma
          (216, 100, 129, 300, "strided"),  # tiled
          (8, 400, 1000, 19, "mixed")]   # wide


def _scatter_prefix(dt, K, N):
    if dt == "f32":
        return "gemm_nt[f32,rows=0,epi=2,"
    Nc = H._rup(N, 8)
    if Nc >= 192 and Nc % 32 == 0:
        return "gemm_nt_dma[bf16,epi=2,"
    return "gemm_nt_wide[bf16,epi=2," if K <= 208 else "gemm_nt[bf16,rows=0,epi=2,"


def _ids(mode, M, V, g):
    if mode == "zeros":
        return torch.zeros(M, dtype=torch.int32, device=DEV)
    if mode == "same":
        return torch.full((M,), V - 1, dtype=torch.int32, device=DEV)
    ids = torch.randint(0, V, (M,), generator=g, device=DEV, dtype=torch.int32)
    ids[::3] = 0
    if mode == "strided":
        wide = torch.randint(0, V, (M, 3), generator=g, device=DEV, dtype=torch.int32)
        wide[:, 1] = ids
        return wide[:, 1]
    return ids


def _problem(dt, K, N, M, V, mode, layer):
    g = torch.Generator(device=DEV).manual_seed(K + 7 * N + 13 * M + 17 * V)
    tdt = H._tdt(dt)
    if layer == "lattice":
        emb, w, dout = H._lattice((V, K), g, DEV), H._lattice((N, K), g, DEV), H._lattice((M, N), g, DEV)
        b = torch.randint(-4, 5, (N,), generator=g, device=DEV).float()
    else:
        emb, w = H._gauss((V, K), g, DEV, 0.5, tdt), H._gauss((N, K), g, DEV, 0.1, tdt)
        dout, b = H._gauss((M, N), g, DEV, 0.1, tdt), torch.randn(N, generator=g, device=DEV) * 0.1
    ids = _ids(mode, M, V, g)
    x, x_abs = emb.double()[ids.long()], emb.double().abs()[ids.long()]
    live = (ids != 0).double().unsqueeze(1)
    dt_ref = torch.zeros(V, K, dtype=torch.float64, device=DEV).index_add_(0, ids.long(), (dout.double() @ w.double()) * live)
    dt_S = torch.zeros(V, K, dtype=torch.float64, device=DEV).index_add_(0, ids.long(), (dout.double().abs() @ w.double().abs()) * live)
    ref = dict(out=(x @ w.double().t() + b.double(), x_abs @ w.double().abs().t() + b.double().abs(), K),
               dw=(dout.double().t() @ x, dout.double().abs().t() @ x_abs, M),
               db=(dout.double().sum(0), dout.double().abs().sum(0), M),
               dtable=(dt_ref, dt_S, N + M))
    return emb, w, b, dout, ids, ref


def _run(emb, w, b, dout, ids, code, train_emb):
    emb, w, b = emb.clone().requires_grad_(train_emb), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        out = ops.gather_linear(emb, w, b, ids, code)
        out.backward(dout)
        torch.cuda.synchronize()
        labels = set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)
    return dict(out=out.detach(), dw=w.grad, db=b.grad, dtable=emb.grad), labels


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("K,N,M,V,mode", SHAPES)
def test_gather_linear_forward_and_backward(dt, K, N, M, V, mode):
    code = ops.NR_BF16 if dt == "bf16" else ops.NR_F32
    has = lambda labels, prefix: any(l.startswith(prefix) for l in labels)
    for layer in ("lattice", "layer2"):
        emb, w, b, dout, ids, ref = _problem(dt, K, N, M, V, mode, layer)
        got, labels = _run(emb, w, b, dout, ids, code, True)
        assert has(labels, f"gemm_nt[{dt},rows=1,epi=0,") and has(labels, f"gemm_tn[{dt},rows=1,"), labels
        assert has(labels, _scatter_prefix(dt, K, N)), labels
        for name, (r, S, terms) in ref.items():
            assert got[name].dtype == torch.float32 and got[name].shape == r.shape, name
            ratio = H.gemm_check_values(got[name], r, layer, S, terms)
            if layer == "layer2":
                print(f"\nL2 gather_linear {dt} {name} ratio {ratio:.4f}")
        assert float(got["dtable"][0].abs().max()) == 0.0          # padding_idx row: exactly zero on both layers
        frozen, labels = _run(emb, w, b, dout, ids, code, False)
        assert frozen["dtable"] is None and not any("epi=2" in l for l in labels), labels
        for name in ("out", "dw", "db"):
            r, S, terms = ref[name]
            H.gemm_check_values(frozen[name], r, layer, S, terms)
