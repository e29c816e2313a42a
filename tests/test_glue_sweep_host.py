"""CPU proof of the glue sweep (tests/test_gpu_glue_sweep.py): its case tables, its fp64 references and the power of its
checker (all in the first part of that file).  Nothing here touches a GPU.

  (a) the fp64 references equal torch autograd in fp64: F.cross_entropy(torch.bmm(...)) with an added gscore term,
      x m + pad (1 - m), F.embedding(padding_idx=0), .t() and F.pad;
  (b) the route functions over the case tables put at least two cases in every route, and the lattice sums stay below 2^24;
  (c) an fp32 stand-in that follows the contract (fp32 products and sums, one rounding to the output type, += onto the
      pre-fills) passes every layer of every case on both input layers;
  (d) each mutant of the stand-in fails the layer named, and any bounded result moved to 1.5 times its bound fails its layer;
  (e) the order-dependence of plain fp32 accumulation that keeps the exact fixed-point expectation out of the scatter-add test;
  (f) the argument refusals the library decides before its device guard, with dummy pointers.
"""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_glue_sweep as H
from newsrecommendation_amd import _lib

DEV = "cpu"
CE = {c.name: c for c in H.ce_cases()}
BLEND = {c.name: c for c in H.blend_cases()}
EVAL = {c.name: c for c in H.eval_cases()}
GATHER = {c.name: c for c in H.gather_cases()}
SCATTER = {c.name: c for c in H.scatter_cases()}
PACK = {c.name: c for c in H.pack_cases()}


# ------------------------------------------------------------------------------------------ the stand-ins
def ce_standin(p, mutant=None):
    c = p.c
    B, Cn, N = c.B, c.C, c.N
    cand, user, lab = p.cand.v.view(B, Cn, N), p.user, p.label[:, None]
    score = (cand * user[:, None, :]).sum(-1)
    if mutant == "score_tail":
        score[:, 8 * (Cn // 8):] = float("-inf")
    p.score.v[0] = score.reshape(-1)
    if mutant == "no_max":
        lse = torch.log(torch.exp(score).sum(1))
    else:
        m = score.max(1, keepdim=True).values
        lse = m[:, 0] + torch.log(torch.exp(score - m).sum(1))
    lv = lse - score.gather(1, lab)[:, 0]
    p.lossvec.v[0] = lv
    p.loss.v[0, 0] = lv.sum() if mutant == "loss_sum" else lv.sum() / B
    s = p.score.v.view(B, Cn)
    d = torch.zeros(B, Cn)
    if p.gloss is not None:
        inv_b = torch.tensor(1.0 / (Cn if mutant == "inv_b_c" else B), dtype=torch.float32)
        d = (torch.softmax(s, 1) - F.one_hot(p.label, Cn).float()) * (p.gloss[0] * inv_b)
    if p.gscore is not None and not (mutant == "gscore_dropped" and p.gloss is not None):
        d = d + p.gscore
    p.dcand.v[:] = (d[..., None] * user[:, None, :]).view(B * Cn, N)
    if mutant == "duser_ld":           # the column loop runs to ld_cand: every row spills into the next, the last into the guard
        ld = p.cand.ld
        wide = p.cand.flat[p.cand.start:p.cand.start + B * Cn * ld].view(B, Cn, ld)
        du = (d[..., None] * wide).sum(1)
        for b in range(B):
            p.duser.flat[p.duser.start + b * N:p.duser.start + b * N + ld] = du[b]
    else:
        p.duser.v[:] = (d[..., None] * cand).sum(1)


def blend_standin(p, mutant=None):
    c, tdt = p.c, H.G._tdt(p.c.dt)
    rows, N = c.n * c.L, c.N
    x, m = p.x.v, p.mask
    if m is None:
        v = x
    else:
        mm = m[torch.arange(N) % rows][None, :] if mutant == "mask_by_column" else m[:, None]
        a, b = (1 - mm, mm) if mutant == "swapped" else (mm, 1 - mm)
        v = x * a + p.pad.v[0][None, :] * b
    if mutant == "truncate" and tdt == torch.bfloat16:
        p.out.v[:] = (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(tdt)
    else:
        p.out.v[:] = v.to(tdt)
    d = p.dout.v.float()
    keep = torch.ones(rows, dtype=torch.bool)
    if mutant == "drop_last_group":
        assert H.blend_route(c)[1].startswith("bwd_vec4")
        rl_n = 256 // (N // 4)
        for r0 in range(0, rows, 64):
            r1 = min(rows, r0 + 64)
            keep[r0 + (r1 - r0) // rl_n * rl_n:r1] = False
        assert not bool(keep.all())
    p.dx.v[keep] = (d if m is None else d * m[:, None])[keep]
    if m is not None and p.use_dpad:
        t = ((1 - m)[:, None] * d)[keep].sum(0)
        if c.det:
            t = (torch.round(((1 - m)[:, None] * d)[keep].double() * 2.0 ** 36).sum(0) * 2.0 ** -36).float()
        if mutant == "dpad_overwrite":
            p.dpad.v[0] = t
        else:
            p.dpad.v[0] += t


def eval_standin(p):
    n = p.c.n_cand
    if n:
        p.score.v[0] = (p.news.v[p.cand_ids[:n].long()] * p.user.v[p.imp_of[:n].long()]).sum(1)


def gather_standin(p, mutant=None):
    c = p.c
    if c.n_ids == 0:
        return
    rows = (p.ids[:c.n_ids] if mutant == "ids_unstrided" else p.ids[::c.stride][:c.n_ids]).long()
    val = p.table.v[rows].float().to(p.out.v.dtype)
    k = min(c.cols, 256) if mutant == "second_pass_dropped" else c.cols
    p.out.v[:, :k] = val[:, :k]


def scatter_standin(p, mutant=None):
    ids = p.ids[::p.c.stride][:p.n].long()
    live = torch.ones_like(ids, dtype=torch.bool) if mutant == "row0_gradient" else ids != 0
    p.dtable.v.index_add_(0, ids[live], p.dout.v[live])


def pack_standin(p, mutant=None, late=False):
    c = p.c
    drows, dcols = (c.cols, c.rows) if c.transpose else (c.rows, c.cols)
    out = torch.zeros(drows, p.dst.ld)
    r, col = torch.meshgrid(torch.arange(drows), torch.arange(p.dst.ld), indexing="ij")
    if c.transpose:
        inside = col < (c.cols if mutant == "transpose_bound" else c.rows)
        idx = p.src.start + col * p.src.ld + r
    else:
        inside = col < c.cols
        idx = p.src.start + r * p.src.ld + col
    out[inside] = p.src.flat[idx[inside].clamp(max=p.src.flat.numel() - 1)]
    out = out.to(p.dst.v.dtype)
    written = torch.ones_like(inside)
    if mutant == "padding_not_zeroed":
        written = inside
    if late:                           # the job's blocks start one late: its last block of 1024 elements is never reached
        total = drows * p.dst.ld
        written.view(-1)[(total - 1) // 1024 * 1024:] = False
    p.dst.v[written] = out[written]


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("mode", H.CE_MODES)
def test_ce_reference_is_autograd(mode):
    p = H.ce_problem(H.CeCase("a", 5, 7, 13, 3, mode, "ordinary"), "layer2", DEV)
    cand, user = p.cand.v.view(5, 7, 13).double().requires_grad_(True), p.user.double().requires_grad_(True)
    gl = None if p.gloss is None else p.gloss.double()
    gs = None if p.gscore is None else p.gscore.double()
    score = torch.bmm(cand, user[:, :, None])[..., 0]
    loss = F.cross_entropy(score, p.label)
    total = (loss * gl[0] if gl is not None else 0) + ((score * gs).sum() if gs is not None else 0)
    total.backward()
    s64, lv64, l64 = H.ce_ref64(cand.detach(), user.detach(), p.label)
    assert torch.allclose(s64, score.detach(), rtol=0, atol=1e-13) and abs(float(l64 - loss.detach())) <= 1e-13
    _, dc, du = H.ce_grad64(cand.detach(), user.detach(), p.label, s64, gl, gs)
    assert float((dc - cand.grad).abs().max()) <= 1e-14 and float((du - user.grad).abs().max()) <= 1e-14


def test_blend_reference_is_autograd():
    p = H.blend_problem(BLEND["frac12-f32"], "layer2", DEV)
    x, pad, m = p.x.v.double().requires_grad_(True), p.pad.v[0].double().requires_grad_(True), p.mask.double()
    out = x * m[:, None] + pad * (1 - m[:, None])
    out.backward(p.dout.v.double())
    t = H.blend_terms(p)
    assert torch.equal(t["blend"][2], out.detach()) and torch.equal(t["dx"][2], x.grad)
    assert float((t["dpad"][2] - p.P.double() - pad.grad).abs().max()) <= 1e-12


def test_scatter_reference_is_embedding_backward():
    p = H.scatter_problem(SCATTER["c65-a"], "layer2", DEV)
    ids = p.ids[::p.c.stride][:p.n].long()
    w = torch.zeros(H.SCATTER_V, p.c.cols, dtype=torch.float64, requires_grad=True)
    F.embedding(ids, w, padding_idx=0).backward(p.dout.v.double())
    ref, S, cnt = H.scatter_ref64(p.dout.v.double(), ids, p.P.double())
    assert float((ref - p.P.double() - w.grad).abs().max()) <= 1e-12 and cnt[0] == 0 and int(cnt.sum()) == 200
    assert sorted(cnt.nonzero()[:, 0].tolist()) == list(H.SCATTER_HOT)
    g = H.gather_problem(GATHER["embed-f32-c12-00"] if "embed-f32-c12-00" in GATHER else next(c for c in H.gather_cases() if c.n_ids == 5), "layer2", DEV)
    rows = g.ids[::g.c.stride][:g.c.n_ids].long()
    assert torch.equal(F.embedding(rows, g.table.v.float()), g.table.v[rows].float()) and 0 in rows.tolist() and len(set(rows.tolist())) < 5


@pytest.mark.parametrize("c", [c for c in H.pack_cases() if c.rows <= 200], ids=lambda c: c.name)
def test_pack_reference_is_transpose_and_pad(c):
    p = H.pack_problem(c, c.dt, "layer2", DEV)
    s = p.src.v.t() if c.transpose else p.src.v
    want = F.pad(s, (0, p.dst.ld - s.shape[1]), value=0.0).to(p.dst.v.dtype)
    assert torch.equal(H._bits(H.pack_ref(p)), H._bits(want)) and want.shape == p.dst.v.shape
    assert p.dst.ld >= (c.rows if c.transpose else c.cols) and p.src.ld == c.cols + c.pad_src


# ------------------------------------------------------------------------------------------ (b)
def test_every_route_has_two_cases():
    H._count_routes([H.ce_route(c) for c in H.ce_cases()], H.CE_ROUTES, "score_ce")
    H._count_routes([H.blend_route(c) for c in H.blend_cases()], H.BLEND_ROUTES, "pad_blend")
    H._count_routes([H.eval_route(c) for c in H.eval_cases()], H.EVAL_ROUTES, "score_eval")
    H._count_routes([H.gather_route(c) for c in H.gather_cases()], H.GATHER_ROUTES, "gather")
    H._count_routes([H.scatter_route(c) for c in H.scatter_cases()], H.SCATTER_ROUTES, "scatter")
    H._count_routes([H.pack_route(c) for c in H.pack_cases()], H.PACK_ROUTES, "cast_pad")
    H._count_routes([H.batch_route(jobs) for _, jobs in H.batch_cases().values()], H.BATCH_ROUTES, "cast_pad_batch")
    H._count_routes([H.drop_route(n, p) for n in H.DROP_COUNTS for p in H.DROP_PS], H.DROP_ROUTES, "dropout_mask")
    for dt in ("bf16", "f32"):        # both types on every blend route
        H._count_routes([H.blend_route(c) for c in H.blend_cases() if c.dt == dt] * 2, H.BLEND_ROUTES, "pad_blend " + dt)


def test_the_tables_hold_what_the_issue_lists():
    ce = H.ce_cases()
    assert {c.C for c in ce if c.N == 65} >= {1, 2, 5, 7, 8, 9, 16, 63, 64}
    for Cn in (5, 9):
        assert {c.N for c in ce if c.C == Cn} >= {1, 63, 64, 65, 400}
    assert {c.B for c in ce} == {1, 3, 255, 257} and {c.mode for c in ce} == set(H.CE_MODES)
    assert {(c.pad, c.pad if c.padd is None else c.padd) for c in ce} == {(0, 0), (0, 3), (3, 0), (3, 3)}
    assert {c.regime for c in ce} == set(H.CE_REGIMES)
    for c in ce:
        lab = H.ce_problem(c, "lattice", DEV).label
        assert 0 <= int(lab.min()) and int(lab.max()) <= c.C - 1 and (c.B < 2 or (int(lab[0]) == 0 and int(lab[1]) == c.C - 1))
    bl = H.blend_cases()
    for N in (1, 3, 4, 12, 400, 1024, 1028):
        assert {(c.n, c.L) for c in bl if c.N == N} >= {(1, 1), (3, 5), (7, 50)}, N
    assert any(c.n * c.L * (c.N // 4) > H.GLUE_GRID and c.N % 4 == 0 for c in bl) and any(c.n * c.L == 65 for c in bl)
    assert {c.mask for c in bl} == set(H.BLEND_MASKS) and {c.mis for c in bl} == {"", "x", "out", "pad", "dout", "dx"} and any(c.det for c in bl)
    for c in bl:
        if c.mis in ("x", "out", "pad"):
            assert c.N % 4 == 0 and H.blend_route(c)[0] == "fwd_scalar", c
        if c.mis in ("dout", "dx"):
            assert c.N % 4 == 0 and H.blend_route(c)[1] == "bwd_scalar", c
    assert H.blend_route(BLEND["N1024-n7"])[1].startswith("bwd_vec4") and H.blend_route(BLEND["N1028-n7"]) == ("fwd_vec4", "bwd_scalar")
    assert H.blend_route(BLEND["N12-n7"])[1] == "bwd_vec4_idle" and 256 // (12 // 4) == 85 and 256 - 2 * (400 // 4) == 56
    ev = H.eval_cases()
    assert {c.N for c in ev} == {1, 3, 4, 252, 256, 260, 400, 402} and {c.n_cand for c in ev} == {0, 1, 4, 5, 1027}
    assert {(c.kn, c.ku) for c in ev} >= {(0, 0), (1, 1), (2, 0), (0, 2)} and {c.mis for c in ev} == {"", "news", "user"}
    ga = H.gather_cases()
    for fn, dt in (("embed", "f32"), ("embed", "bf16"), ("cast", "bf16"), ("cast", "f32")):
        own = [c for c in ga if (c.fn, c.dt) == (fn, dt)]
        assert {c.cols for c in own} == {1, 7, 8, 12, 256, 260, 520} and {c.n_ids for c in own} == {0, 1, 5} and {c.kt for c in own} == {c.ko for c in own} == {0, 1, 2}
        assert {c.mis for c in own} == {"", "table", "out"} and {c.stride for c in own} == ({1, 3} if fn == "embed" else {1})
    sc = H.scatter_cases()
    assert {c.cols for c in sc} == {1, 4, 65, 130} and {c.stride for c in sc} == {1, 3} and {c.det for c in sc} == {False, True}
    pk = H.pack_cases()
    assert {(c.rows, c.cols) for c in pk} == {(1, 1), (3, 5), (5, 3), (200, 400), (1100, 1000)} and {c.dt for c in pk} == {"bf16", "f32"}
    for shape in ((1, 1), (3, 5), (5, 3), (200, 400)):
        assert {(c.dt, c.transpose) for c in pk if (c.rows, c.cols) == shape} == {("bf16", 0), ("bf16", 1), ("f32", 0), ("f32", 1)}
        assert {(c.pad_src, c.wide) for c in pk if (c.rows, c.cols) == shape} == {(0, 0), (2, 1), (0, 1), (2, 0)}
    bt = H.batch_cases()
    assert {len(j) for _, j in bt.values()} == {1, 2, 16}
    totals = {(c.cols if c.transpose else c.rows) * H.pack_ld(c)[1] for _, j in bt.values() for c in j}
    assert {1024, 1025} <= totals and all({c.transpose for c in j} == {0, 1} for _, j in bt.values() if len(j) > 1)


def test_lattice_sums_stay_below_2_24():
    assert H.glue_lattice_peak() < 2 ** 24 // 8
    for c in (CE["C64-B257"], CE["C9-N400"]):
        p = H.ce_problem(c, "lattice", DEV)
        for t in (p.cand.v, p.user, p.gscore):
            if t is not None:
                assert bool((t * 4 == (t * 4).round()).all()) and float(t.abs().max()) <= 1.75


# ------------------------------------------------------------------------------------------ (c)
def _ce_checked(c, layer, mutant=None):
    p = H.ce_problem(c, layer, DEV)
    ce_standin(p, mutant)
    w = H.ce_check_fwd(p)
    w.update(H.ce_check_bwd(p))
    return w


def _blend_checked(c, layer, mutant=None, only=None):
    p = H.blend_problem(c, layer, DEV)
    blend_standin(p, mutant)
    for name, fn in (("fwd", H.blend_check_fwd), ("dx", H.blend_check_dx), ("dpad", H.blend_check_dpad)):
        if only in (None, name):
            fn(p)


def _gather_checked(c, layer, mutant=None):
    p = H.gather_problem(c, layer, DEV)
    gather_standin(p, mutant)
    H.gather_check(p)


def _scatter_checked(c, layer, mutant=None):
    p = H.scatter_problem(c, layer, DEV)
    scatter_standin(p, mutant)
    return H.scatter_check(p)


def _pack_checked(c, layer, mutant=None):
    p = H.pack_problem(c, c.dt, layer, DEV)
    pack_standin(p, mutant)
    H.pack_check(p)


def _batch_checked(name, layer, late=False):
    dt, jobs = H.batch_cases()[name]
    ps = [H.pack_problem(c, dt, layer, DEV, salt=k) for k, c in enumerate(jobs)]
    for k, p in enumerate(ps):
        pack_standin(p, late=late and k >= 1)
    for p in ps:
        H.pack_check(p)


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.ce_cases(), ids=lambda c: c.name)
def test_ce_standin_passes(c, layer):
    _ce_checked(c, layer)


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.blend_cases(), ids=lambda c: c.name)
def test_blend_standin_passes(c, layer):
    _blend_checked(c, layer)


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
def test_eval_standin_passes(layer):
    for c in H.eval_cases():
        p = H.eval_problem(c, layer, DEV)
        eval_standin(p)
        H.eval_check(p)


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
def test_gather_scatter_pack_mask_standins_pass(layer):
    for c in H.gather_cases():
        _gather_checked(c, layer)
    for c in H.scatter_cases():
        _scatter_checked(c, layer)
    for c in H.pack_cases():
        _pack_checked(c, layer)
    for name in H.batch_cases():
        _batch_checked(name, layer)
    for count in H.DROP_COUNTS[:4]:
        for prob in H.DROP_PS:
            for seed in H.DROP_SEEDS:
                buf = H.glue_buf(1, count, count, torch.float32, DEV)
                buf.v[0] = H.drop_ref(count, prob, seed)
                H.drop_check(buf, count, prob, seed)


def test_dropout_reference_properties():
    """The restated hash: p = 0 keeps everything, the kept share follows the 2^-16 threshold, seeds differ."""
    n = H.DROP_COUNTS[-1]
    assert bool((H.drop_ref(n, 0.0, 7) == 1).all())
    for prob in (0.2, 0.5):
        keep = float(H.drop_ref(n, prob, 12345).mean())
        assert abs(keep - (1 - prob)) < 5 * (prob * (1 - prob) / n) ** 0.5 + 2.0 ** -16
    assert float(H.drop_ref(n, 0.99999, 0).mean()) < 1e-4
    assert not torch.equal(H.drop_ref(1025, 0.5, 0), H.drop_ref(1025, 0.5, 2 ** 32 - 1))
    assert int(H._mix32(H.np.array([1], dtype=H.np.uint32))[0]) == 0x514E28B7      # murmur3's fmix32 of 1


# ------------------------------------------------------------------------------------------ (d)
CE_MUTANTS = [("score_tail", "C9", "layer2", ("score",)), ("score_tail", "C5-N400", "lattice", ("score",)), ("score_tail", "C63", "layer2", ("score",)),
              ("no_max", "big-C5", "layer2", ("loss",)), ("no_max", "big-C9", "layer2", ("loss",)),
              ("loss_sum", "C9-N400", "layer2", ("loss",)), ("loss_sum", "C64-B257", "layer2", ("loss",)),
              ("inv_b_c", "C64-B257", "layer2", ("dcand",)), ("inv_b_c", "C9-N63", "layer2", ("dcand",)),
              ("gscore_dropped", "C64-B257", "layer2", ("dcand",)), ("gscore_dropped", "C64-B257", "lattice", ("dcand",)),
              ("duser_ld", "C5-N64", "layer2", ("sentinel", "duser")), ("duser_ld", "C7", "lattice", ("sentinel", "duser"))]


@pytest.mark.parametrize("mutant,case,layer,want", CE_MUTANTS)
def test_ce_mutant_fails_its_layer(mutant, case, layer, want):
    c = CE[case]
    if mutant == "duser_ld":
        assert c.pad == 3
    if mutant in ("inv_b_c", "gscore_dropped"):
        assert c.mode == "both" and c.B != c.C
    with pytest.raises(H.GlueCheckError) as ei:
        _ce_checked(c, layer, mutant)
    assert ei.value.layer in want, ei.value


BLEND_MUTANTS = [("swapped", "frac12-f32", "layer2", "fwd", "blend"), ("swapped", "rows65-bf16", "layer2", "fwd", "blend"),
                 ("mask_by_column", "frac12-f32", "layer2", "fwd", "blend"), ("mask_by_column", "frac1028-bf16", "layer2", "fwd", "blend"),
                 ("truncate", "det400-bf16", "layer2", "fwd", "exact"), ("truncate", "stride-bf16", "layer2", "fwd", "exact"),
                 ("dpad_overwrite", "frac12-f32", "layer2", "dpad", "dpad"), ("dpad_overwrite", "det400-bf16", "lattice", "dpad", "dpad"),
                 ("drop_last_group", "rows65-bf16", "layer2", "dx", "dx"), ("drop_last_group", "rows65-bf16", "layer2", "dpad", "dpad"),
                 ("drop_last_group", "rows65-f32", "lattice", "dx", "dx"), ("drop_last_group", "rows65-f32", "layer2", "dpad", "dpad")]


@pytest.mark.parametrize("mutant,case,layer,only,want", BLEND_MUTANTS)
def test_blend_mutant_fails_its_layer(mutant, case, layer, only, want):
    with pytest.raises(H.GlueCheckError) as ei:
        _blend_checked(BLEND[case], layer, mutant, only)
    assert ei.value.layer == want, ei.value


def test_copy_mutants_fail_their_layers():
    def fails(layer, fn, *a, **k):
        with pytest.raises(H.GlueCheckError) as ei:
            fn(*a, **k)
        assert ei.value.layer == layer, ei.value

    strided = [c for c in H.gather_cases() if c.stride == 3 and c.n_ids == 5]
    assert len(strided) >= 4
    for c in strided:
        fails("gather", _gather_checked, c, "layer2", "ids_unstrided")
    looped = [c for c in H.gather_cases() if c.cols > 256 and c.n_ids]
    assert {(c.fn, c.dt) for c in looped} == {("embed", "f32"), ("embed", "bf16"), ("cast", "bf16"), ("cast", "f32")}
    for c in looped:
        fails("nan", _gather_checked, c, "lattice", "second_pass_dropped")
    for c in H.scatter_cases():
        for layer in H.INPUT_LAYERS:
            fails("scatter", _scatter_checked, c, layer, "row0_gradient")
    tall = [c for c in H.pack_cases() if c.transpose and c.rows > c.cols]
    assert len(tall) >= 4
    for c in tall:
        fails("pack", _pack_checked, c, "layer2", "transpose_bound")
    wide = [c for c in H.pack_cases() if H.pack_ld(c)[1] > (c.rows if c.transpose else c.cols)]
    assert len(wide) >= 8
    for c in wide:
        fails("pack", _pack_checked, c, "lattice", "padding_not_zeroed")
    for name in ("two-bf16", "two-f32", "sixteen-bf16", "sixteen-f32"):
        fails("pack", _batch_checked, name, "layer2", late=True)
    for count in H.DROP_COUNTS[1:4]:
        buf = H.glue_buf(1, count, count, torch.float32, DEV)
        buf.v[0] = H.drop_ref(count, 0.5, 12345, swap_halves=True)
        fails("mask", H.drop_check, buf, count, 0.5, 12345)


def _perturbed(terms, name, k):
    """Moves the element of result `name` with the largest bound to k times that bound from its reference."""
    layer, _, got, ref, bound = next(t for t in terms if t[1] == name)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    i = tuple((bound == bound.max()).nonzero()[0].tolist())
    assert float(bound[i]) > 0
    got[i] = float(ref[i] + k * bound[i])
    return layer


@pytest.mark.parametrize("name", ("score", "lossvec", "loss", "dcand", "duser", "out", "dx", "dpad", "eval", "dtable"))
def test_one_and_a_half_times_the_bound_fails(name):
    """One element moved to 1.5 x its bound from the fp64 reference fails its layer; 0.9 x passes where the bound is wider than
    the spacing of fp32 around the value (everything but the single roundings of dcand and dx)."""
    for k in (0.9, 1.5):
        if name in ("score", "lossvec", "loss", "dcand", "duser"):
            p = H.ce_problem(CE["C9-N400"], "layer2", DEV)
            assert p.c.mode == "both"
            ce_standin(p)
            fwd = name in ("score", "lossvec", "loss")
            layer = _perturbed(H.ce_fwd_terms(p) if fwd else H.ce_bwd_terms(p), name, k)
            run = (lambda: H.ce_check_fwd(p)) if fwd else (lambda: H.ce_check_bwd(p))
        elif name in ("out", "dx", "dpad"):
            p = H.blend_problem(BLEND["det12-f32" if name == "dpad" else "frac12-f32"], "layer2", DEV)
            blend_standin(p)
            key = {"out": "blend", "dx": "dx", "dpad": "dpad"}[name]
            layer = _perturbed([(key,) + H.blend_terms(p)[key]], name, k)
            run = {"out": lambda: H.blend_check_fwd(p), "dx": lambda: H.blend_check_dx(p), "dpad": lambda: H.blend_check_dpad(p)}[name]
        elif name == "eval":
            p = H.eval_problem(EVAL["N402-00"], "layer2", DEV)
            eval_standin(p)
            layer = _perturbed(H.eval_terms(p), "score", k)
            run = lambda: H.eval_check(p)
        else:
            p = H.scatter_problem(SCATTER["c65-det"], "layer2", DEV)
            scatter_standin(p)
            layer = _perturbed(H.scatter_terms(p)[0], "dtable", k)
            run = lambda: H.scatter_check(p)
        if k < 1:
            if name not in ("dcand", "dx"):
                run()
        else:
            with pytest.raises(H.GlueCheckError) as ei:
                run()
            assert ei.value.layer == layer, ei.value


# ------------------------------------------------------------------------------------------ (e)
def test_plain_fp32_accumulation_misses_the_fixed_point_sum():
    """What nr_embed_gather_bwd would have to give under a registered range, 30 * 2^-30 per element, and what sequential fp32
    sums of the same 32 addends give: ascending, descending and eight random orders each miss it.  The entry takes no table
    size and registers no range, so its promise (include/nrhip.h, K1) is fp32 atomics in either mode; the GPU test asserts
    that promise, and this is why it cannot assert the exact expectation."""
    fixed, sums = H.scatter_order_demo()
    assert fixed == 30 * 2.0 ** -30 and len(sums) == 10
    assert all(s != fixed for s in sums), sums
    assert len(set(sums)) > 1               # and they do not even agree with each other


# ------------------------------------------------------------------------------------------ (f)
def test_refusals_before_the_device_guard():
    lib, d = _lib.lib(), 64
    for Cn in (0, 65):
        assert lib.nr_score_ce_fwd(d, 8, d, d, d, d, d, 3, Cn, 8, None) == 1 and f"C={Cn} (1..64)" in _lib.last_error(), _lib.last_error()
        assert lib.nr_score_ce_bwd(d, 8, d, d, d, d, None, d, 8, d, 3, Cn, 8, None) == 1 and f"C={Cn} (1..64)" in _lib.last_error(), _lib.last_error()
    assert lib.nr_score_ce_fwd(d, 8, d, d, d, None, d, 3, 5, 8, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_score_ce_bwd(d, 8, d, d, d, d, None, d, 8, None, 3, 5, 8, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_pad_blend_fwd(d, d, None, d, 3, 5, 8, _lib.NR_BF16, None) == 1 and "mask without pad_doc" in _lib.last_error()
    assert lib.nr_pad_blend_fwd(d, None, None, d, 3, 0, 8, _lib.NR_BF16, None) == 1 and "null/empty" in _lib.last_error()
    assert lib.nr_pad_blend_bwd(d, None, None, d, 3, 5, 8, _lib.NR_BF16, None) == 1 and "null/empty" in _lib.last_error()
    assert lib.nr_score_eval(d, 8, None, d, d, 8, d, 4, 8, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_embed_gather_fwd(None, 8, 0, d, 4, 1, 8, d, 8, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_embed_gather_bwd(d, 8, d, 4, 1, 8, None, 8, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_gather_cast_fwd(d, 8, d, 4, 8, d, 8, 7, None) == 1 and "bad dtype 7" in _lib.last_error()
    assert lib.nr_cast_pad(d, 3, 5, 5, d, 4, _lib.NR_BF16, 0, None) == 1 and "leading dimensions too small" in _lib.last_error()
    assert lib.nr_cast_pad(d, 3, 5, 5, d, 2, _lib.NR_BF16, 1, None) == 1 and "leading dimensions too small" in _lib.last_error()
    assert lib.nr_cast_pad(d, 3, 5, 4, d, 8, _lib.NR_BF16, 0, None) == 1 and "leading dimensions too small" in _lib.last_error()
    job = lambda ld_dst=8, tr=0: _lib.CastJob(src=d, dst=d, rows=3, cols=5, ld_src=5, ld_dst=ld_dst, transpose=tr)
    arr = (_lib.CastJob * 17)(*[job() for _ in range(17)])
    assert lib.nr_cast_pad_batch(arr, 17, _lib.NR_BF16, None) == 1 and "1..16 jobs" in _lib.last_error()
    assert lib.nr_cast_pad_batch(arr, 0, _lib.NR_BF16, None) == 1 and "1..16 jobs" in _lib.last_error()
    arr[2] = job(2, 1)
    assert lib.nr_cast_pad_batch(arr, 16, _lib.NR_BF16, None) == 1 and "job 2 leading dimensions too small" in _lib.last_error()
    arr[2] = _lib.CastJob(src=d, dst=d, rows=1 << 15, cols=1 << 15, ld_src=1 << 15, ld_dst=1 << 15, transpose=0)
    assert lib.nr_cast_pad_batch(arr, 16, _lib.NR_BF16, None) == 1 and "job 2 too large" in _lib.last_error()
    assert lib.nr_dropout_mask(None, 4, 0.5, 1, None) == 1 and "null pointer" in _lib.last_error()
