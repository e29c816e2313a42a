"""CPU proof of the title-convolution sweep (tests/test_gpu_conv_sweep.py): its reference, its case tables and the power of
its checker (all in the first part of that file).  Nothing here touches a GPU.

  * the reference equals torch autograd of F.conv1d(padding=1) over F.embedding(padding_idx=0) with the same keep mask, in
    fp64 (the bounds assume this reference, so it is proven independently);
  * a CPU stand-in that follows the contract (fp32 products and sums, one rounding to the compute dtype, `+=` onto the
    pre-fills, rows of far unneeded titles left unwritten) passes every check on both layers over the whole case table;
  * eleven mutants of the stand-in each fail the layer named;
  * conv_labels over the case table: every label family has at least two cases; the lattice stays below 2^24;
  * argument refusals the library decides before its device guard, with dummy pointers.

Forward / dW cases run here with at most 96 titles (the checker is the same; route and domain checks use the real count).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_gpu_gemm_sweep as H
import test_gpu_conv_sweep as S
from newsrecommendation_amd import _lib

DEV = "cpu"
CONV = S.conv_small_cases() + S.conv_slab_cases() + [S.conv_refused_case()]
TAB = S.conv_table_cases()


def _n(c):
    return min(c.n, 96)


# ------------------------------------------------------------------------------------------ reference against autograd
@pytest.mark.parametrize("n,T,D,Dp,N,ids", [(7, 1, 4, 4, 8, "same"), (12, 5, 5, 8, 8, "mixed"), (6, 30, 20, 24, 16, "mixed"),
                                            (40, 2, 8, 8, 4, "same")])
def test_reference_equals_fp64_autograd(n, T, D, Dp, N, ids):
    """lattice (scale exactly 2): exact.  layer2: y / dW / db without dropout (the reference rounds x * scale to the compute
    dtype, autograd does not), dtable with it (there the reference applies keep * scale in fp64 as autograd does)."""
    for layer, drop in (("lattice", True), ("layer2", False), ("layer2", True)):
        c = S._cc("f32", n, T, D, Dp, N, ids, xr=False, p=drop)
        p = S.conv_problem(c, layer, DEV)
        scale = S._scale32(p.p)
        emb = p.tab.reshape(S.CONV_V, T * D).double().requires_grad_(True)
        w, b = p.w.double().requires_grad_(True), p.b.double().requires_grad_(True)
        x = F.embedding(p.ids.long(), emb, padding_idx=0).view(n, T, D) * (p.keep.double() * scale)
        y = F.conv1d(x.permute(0, 2, 1), w, b, padding=1).permute(0, 2, 1)
        y.backward(p.dy.double())
        tol = 0.0 if layer == "lattice" else 1e-12
        close = lambda a, r: float((a - r).abs().max()) <= tol * max(1.0, float(r.abs().max()))
        if not (layer == "layer2" and drop):
            dw = (p.dw_ref - p.P.double()).view(N, 3, Dp)[:, :, :D].permute(0, 2, 1)
            assert close(p.y_ref.view(n, T, N), y.detach()) and close(dw, w.grad) and close(p.db_ref - p.Pb.double(), b.grad), layer
            assert float((p.dw_ref - p.P.double()).view(N, 3, Dp)[:, :, D:].abs().max() if Dp > D else 0.0) == 0.0
        ref, _, touched = S.conv_dtable_ref(p.ids, p.dy, p.w, p.keep, scale, S.CONV_V, "f32", layer)
        assert close(ref, emb.grad), layer
        assert not bool(touched[0]) and float(emb.grad[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ stand-in and mutants
def _round(x, tdt, trunc=False):
    if tdt == torch.float32:
        return x
    if trunc:
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return x.to(tdt).float()


def _standin_conv(p, mutant=None):
    """Writes what a sound library (or the named mutant of it) would into x_rows, y, dw_pack and db."""
    c, n, T, D, Dp, N, tdt = p.c, p.n, p.c.T, p.c.D, p.c.Dp, p.c.N, H._tdt(p.c.dt)
    x = p.tabbuf[:S.CONV_V].float().view(S.CONV_V, T, Dp)[p.ids.long()]
    if p.p:
        keep = p.keep_flat[:n * T * Dp].view(n, T, Dp)[:, :, :D] if mutant == "drop_index_dp" else p.keep
        scale = torch.tensor(S._scale32(p.p), dtype=torch.float32)
        live = x[:, :, :D] * scale if mutant == "scale_after_rounding" else _round(x[:, :, :D] * scale, tdt)
        x = torch.cat([torch.where(keep != 0, live, torch.zeros(())), x[:, :, D:]], 2)
    X = S.conv_im2col(x)
    if mutant == "taps_reversed":
        X = X.view(n * T, 3, Dp).flip(1).reshape(n * T, 3 * Dp)
    if mutant == "border_from_neighbour":
        flat, z = x.reshape(n * T, Dp), torch.zeros(1, Dp)
        X = torch.cat([torch.cat([z, flat[:-1]]), flat, torch.cat([flat[1:], z])], 1)
    y = _round(X @ p.wpbuf[:N].float().t() + p.bbuf[:N], tdt)
    if mutant == "err_1p5":
        y[0, 0] = float(p.y_ref[0, 0] + 1.5 * H.gemm_layer2_bound(p.y_ref, p.y_S, 3 * D + 1, tdt)[0, 0])
    near = torch.ones(n, dtype=torch.bool)
    if p.skips:                                           # titles farther than 256 / T + 2 from every needed one stay unwritten
        pos, m = torch.arange(n), 256 // T + 2
        near = ((pos[:, None] - pos[None, :]).abs() <= m)[:, p.live].any(1)
    rows = (p.live if p.skips else near).repeat_interleave(T)
    if mutant == "y_row_unwritten":
        rows = rows.clone()
        rows[int(rows.nonzero()[0])] = False
    p.ybuf[:n * T][rows] = y.to(tdt)[rows]
    if c.xr:
        blocks = p.xbuf[:n * (T + 1)].view(n, T + 1, Dp)
        for s in near.nonzero().flatten().tolist():
            blocks[s, 0] = 0
            blocks[s, 1:] = x[s].to(tdt)
            p.xbuf[(s + 1) * (T + 1)] = 0
    dy = p.dybuf[:n * T].float()
    if mutant == "dw_stored":
        p.wbuf[:N] = dy.t() @ X
    else:
        p.wbuf[:N] += dy.t() @ X
    p.dbbuf[:N] += dy.sum(0)


def _check_conv(p):
    if p.c.xr:
        S.conv_check_xrows(p)
    return max(S.conv_check_y(p), *S.conv_check_dw(p))


def _standin_table(p, mutant=None):
    c, n, T, D, N, V, tdt = p.c, p.n, p.c.T, p.c.D, p.c.N, p.c.V, H._tdt(p.c.dt)
    dy = p.dybuf[:n * T].float().view(n, T, N)
    dx = _round(S.conv_im2col(dy) @ p.wtbuf[:D, :3 * N].float().t(), tdt, trunc=mutant == "dx_trunc").view(n, T * D)
    good = (p.ids > 0) & (p.ids < V)
    if mutant == "padding_row_gradient":
        good = (p.ids >= 0) & (p.ids < V)
    if p.flags is not None and mutant != "flagged_zero_contributes":
        good = good & (p.flags != 0)
    if mutant == "drop_occurrence":                       # the 257th occurrence of an id: the first of the scatter's second run
        seen = {}
        for s in good.nonzero().flatten().tolist():
            seen[int(p.ids[s])] = seen.get(int(p.ids[s]), 0) + 1
            if seen[int(p.ids[s])] == 257:
                good[s] = False
    scale = torch.tensor(S._scale32(p.p), dtype=torch.float32)
    contrib = torch.where(p.keep.reshape(n, T * D) != 0, dx * scale, torch.zeros(()))[good]
    acc = torch.zeros(V, T * D).index_add_(0, p.ids[good].long(), contrib)
    hit = torch.zeros(V, dtype=torch.bool)
    hit[p.ids[good].long()] = True
    p.dtable[:V][hit] += acc[hit]


# mutant -> (layer it must fail, layer it runs on, the cases it applies to)
CONV_MUTANTS = {
    "taps_reversed": ("lattice", "lattice", lambda c: c.ids != "zeros" and c.T > 1),
    "border_from_neighbour": ("lattice", "lattice", lambda c: c.ids != "zeros" and c.n > 1),
    "drop_index_dp": (None, "lattice", lambda c: c.p and c.Dp > c.D and c.ids != "zeros" and c.n * c.T > 1),      # x_rows where given, else lattice
    "scale_after_rounding": ("layer2", "layer2", lambda c: c.p and c.dt == "bf16" and not c.xr and c.ids != "zeros" and c.dyp != "zero"),
    "dw_stored": ("lattice", "lattice", lambda c: True),
    "y_row_unwritten": ("sentinel", "lattice", lambda c: True),
    "err_1p5": ("layer2", "layer2", lambda c: c.dt == "f32"),
}
TAB_MUTANTS = {
    "padding_row_gradient": ("sentinel", "lattice", lambda c: c.ids in ("mixed", "strided", "oob", "zeros")),
    "flagged_zero_contributes": ("lattice", "lattice", lambda c: c.nz and c.ids != "zeros"),
    "drop_occurrence": ("lattice", "lattice", lambda c: c.ids == "same" and c.n > 256),
    # sums must leave the 8-bit significand: 2.25 per product, min(T, 3) * N products (T = 1 has the centre tap only)
    "dx_trunc": ("lattice", "lattice", lambda c: c.dt == "bf16" and min(c.T, 3) * c.N >= 128 and c.ids != "zeros"),
}


def _fails(check, p, layer, mutant):
    try:
        check(p)
    except H.GemmCheckError as e:
        assert e.layer == layer, (mutant, p.c, p.layer, e)
        return
    pytest.fail(f"mutant {mutant} passed every check on {p.c} ({p.layer})")


def _reset(p):
    for buf, before in ((p.ybuf, p.ybefore), (p.xbuf, p.xbefore), (p.wbuf, p.wbefore), (p.dbbuf, p.dbbefore)):
        buf.copy_(before)


def test_conv_standin_passes_and_every_mutant_fails_its_layer():
    hit = {m: 0 for m in CONV_MUTANTS}
    skipped_rows = 0
    for c in CONV:
        for layer in ("lattice", "layer2"):
            p = S.conv_problem(c, layer, DEV, n=_n(c))
            _standin_conv(p)
            assert _check_conv(p) <= 1.0
            skipped_rows += int((H._bits(p.ybuf[:p.n * c.T]) == H._bits(p.ybefore[:p.n * c.T])).all(1).sum())
            for m, (fails, runs_on, applies) in CONV_MUTANTS.items():
                if runs_on != layer or not applies(c._replace(n=p.n)) or (p.n * c.T > 300 and hit[m] > 8):
                    continue
                _reset(p)
                _standin_conv(p, m)
                _fails(_check_conv, p, fails or ("x_rows" if c.xr else "lattice"), m)
                hit[m] += 1
    assert all(v >= 2 for v in hit.values()), hit
    assert skipped_rows > 0                               # the "needed" cases did leave rows unwritten, and that passed


def test_table_standin_passes_and_every_mutant_fails_its_layer():
    hit = {m: 0 for m in TAB_MUTANTS}
    for c in TAB:
        for layer in ("lattice", "layer2"):
            p = S.conv_table_problem(c, layer, DEV)
            _standin_table(p)
            assert S.conv_check_dtable(p) <= 1.0
            if c.ids == "zeros":
                assert torch.equal(H._bits(p.tflat), H._bits(p.tbefore))
            for m, (fails, runs_on, applies) in TAB_MUTANTS.items():
                if runs_on != layer or not applies(c):
                    continue
                if m == "flagged_zero_contributes":       # an id whose every title is flagged zero: its row must stay untouched
                    off = (p.ids > 0) & (p.ids < c.V) & (p.flags == 0)
                    fails = "sentinel" if bool((~p.touched[p.ids[off].long()]).any()) else "lattice"
                p.tflat.copy_(p.tbefore)
                _standin_table(p, m)
                _fails(S.conv_check_dtable, p, fails, m)
                hit[m] += 1
    assert all(v >= 2 for v in hit.values()), hit


def test_dtable_bound_needs_its_prefill_term():
    """Without u |pre-fill| the sound stand-in fails: the last addition rounds a sum that holds the value accumulated onto."""
    worst = 0.0
    for c in TAB:
        p = S.conv_table_problem(c, "layer2", DEV)
        _standin_table(p)
        bare = p.bound - H.GEMM_U * p.P.double().abs()
        diff = (p.dtable[:c.V].double() - p.ref).abs()
        worst = max(worst, float(torch.where(diff > 0, diff / bare, torch.zeros_like(diff)).max()))
    assert worst > 1.0, worst


# ------------------------------------------------------------------------------------------ tables, routes, domain
def test_every_label_family_has_two_cases_and_the_tables_hold_the_planned_values():
    count = {f: 0 for f in S.CONV_FAMILIES}
    for c in CONV + TAB:
        want = S.conv_labels(c)
        for label in {l for ls in want.values() if ls for l in ls}:
            count[S.conv_label_family(label)] += 1          # KeyError: a family the plan does not know
    assert all(v >= 2 for v in count.values()), count
    assert len(set(CONV)) == len(CONV) and len(set(TAB)) == len(TAB) and 55 <= len(CONV) + len(TAB) <= 90
    small = S.conv_small_cases()
    assert {c.T for c in small} == {1, 2, 3, 4, 5, 30} and {255, 256, 257} <= {c.n * c.T for c in small}
    assert {(c.D, c.Dp) for c in small} >= {(4, 4), (4, 8), (5, 8), (20, 24), (50, 64), (64, 64), (72, 72), (96, 96), (300, 320)}
    assert {c.N for c in small} == {8, 200, 208, 216, 320, 400} and {c.ids for c in small} == {"mixed", "same", "zeros", "strided"}
    assert {(c.dt, c.xr, c.p) for c in small} == {(d, x, p) for d in ("bf16", "f32") for x in (False, True) for p in (False, True)}
    for c in small:
        assert not S.conv_slab_shape(c) and c.Dp >= c.D and c.Dp % (8 if c.dt == "bf16" else 4) == 0 and c.N % (8 if c.dt == "bf16" else 4) == 0
    slab = [c for c in S.conv_slab_cases() if S.conv_slab_shape(c)]
    assert {(c.T, c.n) for c in slab} == {(32, 512), (32, 513), (30, 560), (8, 2048)} and {(c.Dp, c.N) for c in slab} == {(64, 64), (96, 264), (64, 264), (96, 64)}
    assert {c.dyp for c in slab} == {"all", "zero", "first", "last", "alt"} and {(c.ws, c.nz) for c in slab} == {(False, False), (True, False), (True, True)}
    assert sum(c.needed for c in slab) == 4 and S.conv_labels(S.conv_refused_case())["dw"] is None
    assert {c.D for c in TAB} == {4, 5, 35, 64, 300} and {c.n for c in TAB} >= {1, 300, 1025, 2048} and {c.N for c in TAB} == {8, 56, 64, 72}
    assert {c.ids for c in TAB} == {"mixed", "same", "zeros", "strided", "oob"} and {c.off for c in TAB} == {0, 1}
    for c in TAB:
        ch = 8 if c.dt == "bf16" else 4
        assert c.N % ch == 0 and c.ldwt % ch == 0 and c.ldwt >= 3 * c.N and (c.ids != "same" or c.V >= 2), c
    assert any(c.off and c.D % 4 == 0 for c in TAB) and any(c.T * c.D > 4096 for c in TAB) and any(c.D % 4 and c.T * c.D > 1024 for c in TAB)


def test_lattice_domain_is_exact_in_bf16_and_below_2_pow_24():
    """|x|, |w|, |dy| <= 3, |b| <= 4, |pre-fill| <= 5, scale 2: y <= 2*9*3D + 4, dW <= 2*9*n*T + 5, |dx| <= 27 N (bf16 keeps an
    integer rounded to 8 bits an integer), dtable <= 2 * n * 27 N + 5."""
    for c in CONV:
        assert 18 * 3 * c.D + 4 < 2 ** 24 and 18 * c.n * c.T + 5 < 2 ** 24, c
    for c in TAB:
        assert 2 * c.n * 27 * c.N * 1.01 + 5 < 2 ** 24, c
    p = S.conv_problem(CONV[2], "lattice", DEV)
    for t in (p.tab, p.w, p.dy, p.b, p.P, p.Pb):
        f = t.float()
        assert torch.equal(f, f.to(torch.bfloat16).float()) and torch.equal(f, f.round()) and float(f.abs().max()) <= 5
    assert S._scale32(0.5) == 2.0 and S._scale32(0.0) == 1.0 and abs(S._scale32(0.2) - 1.25) < 1e-6


# ------------------------------------------------------------------------------------------ refusals before the device guard
def _dummy(**over):
    v = dict(n=4, T=5, D=5, Dp=8, N=8, dtype=_lib.NR_BF16, table=0x1000, ids=0x1000, ids_stride=1, w_pack=0x1000, bias=0x1000, ld_rows=8)
    v.update(over)
    return _lib.ConvDesc(**v)


@pytest.mark.parametrize("what,over,y", [("bad dtype", dict(dtype=7), 0x1000), ("bad shape", dict(Dp=4), 0x1000), ("bad shape", dict(Dp=12), 0x1000),
                                          ("multiple of", dict(N=12), 0x1000), ("null operand", dict(ids_stride=0), 0x1000),
                                          ("null operand", dict(bias=0), 0x1000), ("null output", {}, 0)])
def test_forward_refuses_on_the_host(what, over, y):
    """Dummy pointers: each call must fail on a host check, before the device is looked at and before anything is read."""
    d = _dummy(**over)
    assert _lib.lib().nr_conv1d_k3_fwd(C.byref(d), y, None) != 0 and what in _lib.last_error(), _lib.last_error()


def test_backward_refuses_null_outputs_on_the_host():
    d = _dummy()
    for dy, dw, db in ((0, 0x1000, 0x1000), (0x1000, 0, 0x1000), (0x1000, 0x1000, 0)):
        assert _lib.lib().nr_conv1d_k3_bwd(C.byref(d), dy, dw, db, None) != 0 and "null operand" in _lib.last_error()
    assert _lib.lib().nr_conv1d_k3_bwd(C.byref(_dummy(N=12)), 0x1000, 0x1000, 0x1000, None) != 0 and "multiple of" in _lib.last_error()


@pytest.mark.parametrize("what,over,ldwt,dy", [("bad shape", dict(N=12), 48, 0x1000), ("dropout p", dict(p_in=1.0), 32, 0x1000),
                                                ("ldwt", {}, 16, 0x1000), ("ldwt", {}, 28, 0x1000), ("16-byte aligned", {}, 32, 0x1004),
                                                ("table_rows", dict(table_rows=0), 32, 0x1000)])
def test_table_gradient_refuses_on_the_host(what, over, ldwt, dy):
    d = _dummy(**dict(dict(table_rows=19), **over))
    rc = _lib.lib().nr_conv1d_k3_bwd_table(C.byref(d), dy, 0x1000, ldwt, 0x1000, 0x1000, 1 << 40, None)
    assert rc != 0 and what in _lib.last_error(), _lib.last_error()
