"""CPU proof of the GEMM building-block sweep (tests/test_gpu_gemm_sweep.py): its case tables, its input domain and the
power of its checker (both the first part of that file, "GEMM building-block sweep").  Nothing here touches a GPU.

  * every case sits on the route its table row names, by the dispatch rules of csrc/nr_gemm.hip restated in
    gemm_nt_route / gemm_tn_route there (the GPU file asserts the label the library itself reports), every value of the
    tables occurs, every route has a case with lda, ldb, ldc / ldw above the packed value, and both sides of the B-padding
    contract of nr_gemm_nt are present: K % 32 == 0 with B a column slice of a wider (NaN) matrix on the kernels that do not
    predicate B's K tail, K % 32 != 0 with ldb = K on the two that do;
  * the lattice domain: operands exactly representable in bf16, worst-case |sum| below 2^24;
  * a CPU stand-in that computes the same contract in fp32 torch (fp32 products and sums, one rounding to the output type,
    `+=` onto the pre-fill for TN) passes both layers of every case;
  * each mutant of the stand-in fails the layer named, on every case it applies to.

TN cases run here with at most 160 rows (the checker is the same; the domain check uses the real row count).
"""
import pytest
import torch

import test_gpu_gemm_sweep as H

NT, TN = H.gemm_nt_cases(), H.gemm_tn_cases()
DEV = "cpu"


def _tn_rows(c):
    return min(c.M, 128 + c.M % 32)


def _round_out(x, dt, trunc=False):
    """fp32 -> the output type: nearest even as the kernels' (bf16_t) casts, or (mutant) truncation."""
    if dt == torch.float32:
        return x
    if trunc:
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return x.to(torch.bfloat16)


def _nt_standin(p, mutant=None):
    """Writes what a sound kernel (or the named mutant of it) would into p.cbuf."""
    c, odt = p.c, p.cbuf.dtype
    a, b = p.a.float(), p.b.float()
    if mutant == "drop_k8":
        k = max(c.K - 8, 0)
        a, b = a[:, :k], b[:, :k]
    if mutant == "bf16_accum":
        acc = torch.zeros(c.M, c.N)
        for k0 in range(0, c.K, 8):
            acc = (acc + a[:, k0:k0 + 8] @ b[:, k0:k0 + 8].t()).to(torch.bfloat16).float()
    else:
        acc = a @ b.t()
    if mutant == "split_twice":
        acc = acc + a[:, :8] @ b[:, :8].t()
    if mutant == "bias_after_rounding":
        acc = _round_out(acc, odt).float()
    if p.bias is not None:
        acc = acc + p.bias
    if c.tanh:
        acc = torch.tanh(acc.double()).float()
    out = _round_out(acc, odt, trunc=mutant == "bf16_trunc")
    if mutant == "shift_tile":
        out = out.clone()
        out[:, 0:16] = out[:, 16:32].clone()
    rows = c.M - 1 if mutant == "drop_row" else c.M
    p.cbuf[:rows, :c.N] = out[:rows]
    if mutant == "write_past_n":
        p.cbuf[0, c.N] = 1.0


def _tn_standin(p, mutant=None):
    c = p.c
    d, a = p.dc.float(), p.a.float()
    if mutant == "drop_row":
        d, a = d[:-1], a[:-1]
    w, bsum = d.t() @ a, d.sum(0)
    if mutant == "split_twice":
        w, bsum = w + d[:32].t() @ a[:32], bsum + d[:32].sum(0)
    if mutant == "bf16_accum":
        w = w.to(torch.bfloat16).float()
    if mutant == "dw_overwrite":
        p.wbuf[:c.N, :c.K] = w
    else:
        p.wbuf[:c.N, :c.K] += w
    if c.db:
        p.dbbuf[:c.N] += bsum
    if mutant == "write_past_n":
        p.wbuf[0, c.K] = 1.0


# mutant -> (layer it must fail, layer it runs on, the NT cases it applies to)
NT_MUTANTS = {
    "drop_row": ("lattice", "lattice", lambda c: True),
    "drop_k8": ("lattice", "lattice", lambda c: True),
    "shift_tile": ("lattice", "lattice", lambda c: c.N >= 32),
    # sums must leave the 8-bit significand: |sum| reaches 256 for K >= 192 at every element count of the tables
    "bf16_trunc": ("lattice", "lattice", lambda c: c.out == "bf16" and c.K >= 192),
    "split_twice": ("lattice", "lattice", lambda c: True),
    "bias_after_rounding": ("lattice", "lattice", lambda c: c.out == "bf16" and c.bias and c.K >= 192),
    "bf16_accum": ("layer2", "layer2", lambda c: c.out == "f32" or c.K >= 192),
    "write_past_n": ("sentinel", "lattice", lambda c: c.ldc > c.N),
}
TN_MUTANTS = {
    "drop_row": ("lattice", "lattice"),
    "dw_overwrite": ("lattice", "lattice"),
    "split_twice": ("lattice", "lattice"),
    "bf16_accum": ("layer2", "layer2"),
    "write_past_n": ("sentinel", "lattice"),
}


def test_tables_cover_every_route_value_stride_and_both_sides_of_the_padding_contract():
    assert 100 <= len(NT) <= 140 and len(set(NT)) == len(NT) and len(set(TN)) == len(TN)
    for c in NT:
        assert H.gemm_nt_route(c) == c.route, c
        ch = 4 if c.dt == "f32" else 8
        assert c.K % ch == 0 and c.lda % ch == 0 and c.ldb % ch == 0 and c.ldc % 4 == 0, c
        assert c.lda >= c.K and c.ldb >= c.K and c.ldc >= c.N and 1 <= c.M <= 16448, c
    for c in TN:
        assert H.gemm_tn_route(c) == c.route, c
        ch = 4 if c.dt == "f32" else 8
        assert c.N % ch == 0 and c.K % ch == 0 and c.ldc % ch == 0 and c.lda % ch == 0, c
        assert c.ldc >= c.N and c.lda >= c.K and c.ldw > c.K and 1 <= c.M <= 16448, c
    for route, Ks, Ns, Ms, _ in H._nt_rows():
        cs = [c for c in NT if c.route == route]
        for name, vals in (("K", Ks), ("N", Ns), ("M", Ms)):
            assert set(vals) <= {getattr(c, name) for c in cs}, (route, name)
        assert any(c.lda > c.K for c in cs) and any(c.ldc > H._rup(c.N, 8) for c in cs), route
        if route in ("wide", "tiled"):
            assert any(c.K % 32 != 0 and c.ldb == c.K for c in cs), route          # predicated: the next row sits in the "padding"
            assert any(c.K == 304 and c.ldb == 304 for c in cs), route
        if route != "f32":
            assert any(c.K % 32 == 0 and c.ldb > c.K for c in cs), route            # a column slice of a wider non-zero matrix
        if route.startswith("wreg") or route.startswith("dma"):
            assert all(c.ldb >= H._rup(c.K, 32) for c in cs) and any(c.ldb > H._rup(c.K, 32) for c in cs), route
    assert {c.out for c in NT if c.route == "dma20"} == {"bf16", "f32"} and any(c.tanh for c in NT if c.route == "dma20")
    assert any(c.tanh for c in NT if c.route == "f32")
    for r in ("tn3_w320_n256", "tn3_w320_n128", "tn3_w160", "tn2", "tn_f32"):
        cs = [c for c in TN if c.route == r]
        assert {c.db for c in cs} == {True, False} and any(c.ldc > c.N for c in cs) and any(c.lda > c.K for c in cs), r
    assert [c.route for c in H.gemm_nt_wreg_off_cases()] == ["wreg5", "wreg3", "wreg_tanh"]
    assert len(H.gemm_tn_det_cases()) == 5


def _in_domain(ts, hi):
    """Integers of magnitude <= hi, exactly representable in bf16."""
    for t in ts:
        f = t.float()
        assert torch.equal(f, f.to(torch.bfloat16).float()) and torch.equal(f, f.round()) and float(f.abs().max()) <= hi


def test_lattice_domain_is_exact_in_bf16_and_below_2_pow_24():
    for c in NT + TN:
        assert H.gemm_lattice_worst(c) < 2 ** 24, c
    assert max(H.gemm_lattice_worst(c) for c in NT + TN) == 9 * 16448 + 5
    for c in NT:
        p = H.gemm_nt_problem(c, "lattice", DEV)
        _in_domain((p.a, p.b), 3)
        _in_domain((p.bias,) if c.bias else (), 4)
    for c in TN:
        p = H.gemm_tn_problem(c, "lattice", DEV, M=_tn_rows(c))
        _in_domain((p.dc, p.a), 3)
        _in_domain((p.P, p.Pb), 5)


def _fails(check, p, layer):
    with pytest.raises(H.GemmCheckError) as e:
        check(p)
    assert e.value.layer == layer, (p.c, e.value)


def test_nt_standin_passes_and_every_mutant_fails_its_layer():
    hit = {m: 0 for m in NT_MUTANTS}
    for c in NT:
        for layer in (("layer2",) if c.tanh else ("lattice", "layer2")):
            p = H.gemm_nt_problem(c, layer, DEV)
            _nt_standin(p)
            assert H.gemm_check_nt(p) <= 1.0
            for m, (fails, runs_on, applies) in NT_MUTANTS.items():
                if runs_on != layer or not applies(c) or (c.M > 300 and hit[m] > 40):
                    continue
                p.cbuf.copy_(p.before)
                _nt_standin(p, m)
                _fails(H.gemm_check_nt, p, fails)
                hit[m] += 1
    assert all(n >= 20 for n in hit.values()), hit


def test_tn_standin_passes_and_every_mutant_fails_its_layer():
    for c in TN:
        for layer in ("lattice", "layer2"):
            p = H.gemm_tn_problem(c, layer, DEV, M=_tn_rows(c))
            _tn_standin(p)
            assert H.gemm_check_tn(p) <= 1.0
            for m, (fails, runs_on) in TN_MUTANTS.items():
                if runs_on != layer:
                    continue
                p.wbuf.copy_(p.wbefore)
                p.dbbuf.copy_(p.dbbefore)
                _tn_standin(p, m)
                _fails(H.gemm_check_tn, p, fails)
