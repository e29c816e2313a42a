"""CPU proof of the step sweep (tests/test_gpu_step_sweep.py): its case tables, its references and the power of its checker
(all in the first part of that file).  Nothing here touches a GPU.

  (a) the Adam reference equals a hand-written fp64 transcription of torch.optim.Adam's update on the same state, and
      torch.optim.Adam itself in fp64 from a zero state;
  (b) the metric reference equals tests/golden/metrics.json where the fixture has no ties, np.argsort(kind="stable")[::-1] on
      ties, and sklearn's roc_auc_score where sklearn imports;
  (c) the route functions put at least two cases in every route, the tables hold what the issue lists, and every intermediate
      value of the exact Adam layer is representable in fp32;
  (d) a stand-in that follows the contract (fp32 Adam with and without fused multiply-adds, the row replay built from it, the
      kernel's counting loops for the metrics in numpy, index arithmetic for the rest) passes every layer of every case but the
      grid-stride tables of Adam, the row kernel and the assembly;
  (e) each of nineteen mutants fails the layer named, and any bounded result moved to 1.5 times its bound fails its layer;
  (f) the argument refusals the library decides before any launch, with dummy pointers.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import test_gpu_step_sweep as H
from newsrecommendation_amd import _lib

DEV = "cpu"
ADAM = {c.name: c for c in H.adam_cases()}
ROWS = {c.name: c for c in H.rows_cases()}
ASM = {c.name: c for c in H.asm_cases()}
STACK = {c.name: c for c in H.stack_cases()}
CHECK = {c.name: c for c in H.check_cases()}
HOST_ADAM = [c for c in H.adam_cases() if c.n < H.ADAM_BIG]                  # the two grid-stride tables stay on the GPU
HOST_ROWS = [c for c in H.rows_cases() if c.script != "all"]
T = lambda x: torch.tensor(x, dtype=torch.float32)


# ------------------------------------------------------------------------------------------ the stand-ins
def _fma(a, b, c, fused):
    """a b + c with one rounding (the product of two fp32 values is exact in fp64) or with two."""
    return (a.double() * b.double() + c.double()).float() if fused else a * b + c


def adam1(p, g, m, v, ss, bc, b1, b2, eps, gs, fused, mutant=None):
    """csrc/nr_adam.h adam1 on fp32 tensors: (p', m', v').  fused: the three places -ffp-contract=fast may contract."""
    gr = g.clone() if mutant == "grad_scale_dropped" else g * T(gs)
    m1 = _fma(T(1.0) - T(b1), gr - m, m, fused)
    v1 = _fma(T(b2), v, (T(1.0) - T(b2)) * gr * gr, fused)
    if mutant == "eps_inside_root":
        denom = torch.sqrt(v1 + T(eps)) / T(bc)
    elif mutant == "bc2_sqrt_dropped":
        denom = torch.sqrt(v1) + T(eps)
    else:
        denom = torch.sqrt(v1) / T(bc) + T(eps)
    q = (m if mutant == "m_after_use" else m1) / denom
    return _fma(-T(ss), q, p, fused), m1, v1


def adam_standin(fused, mutant=None):
    def call(P, step):
        c = P.c
        lr, b1, b2, eps = H.adam_hp(c)
        ss, bc = H.adam_scalars(lr, b1, b2, step)
        p, g, m, v = (b.v[0] for b in (P.p, P.g, P.m, P.v))
        k = c.n // 4 * 4 if mutant == "tail_skipped" else c.n
        pn, mn, vn = adam1(p[:k], g[:k], m[:k], v[:k], ss, bc, b1, b2, eps, c.gs, fused, mutant)
        p[:k], m[:k], v[:k] = pn, mn, vn
        if c.zg and mutant != "zero_grad_ignored":
            g[:k] = 0.0
        for (first, rows, cols, ld), d in zip(c.jobs, P.dst):
            src = p[0 if mutant == "job_ignores_first" else first:][:rows * cols]
            if mutant == "bf16_truncated":
                src = (src.contiguous().view(torch.int32) & -65536).view(torch.float32)
            if mutant == "row_split_by_ld":
                d.flat[d.start:d.start + rows * cols] = src.to(torch.bfloat16)
            else:
                d.v[:] = src.view(rows, cols).to(torch.bfloat16)
    return call


def dense_rows_standin(P, s):
    c, A = P.c, P.A
    lr, b1, b2, eps = H.ROWS_HP
    ss, bc = H.adam_scalars(lr, b1, b2, s)
    pn, mn, vn = adam1(A.p.v, A.g.v, A.m.v, A.v.v, ss, bc, b1, b2, eps, c.gs, True)
    A.p.v[:], A.m.v[:], A.v.v[:] = pn, mn, vn
    A.g.v[:] = 0.0
    if A.pack is not None:
        A.pack.v[:] = pn.reshape(-1, c.pack[0]).to(torch.bfloat16)


def rows_standin(mutant=None):
    def call(P, ids, n_ids, upto, apply):
        c, B = P.c, P.B
        lr, b1, b2, eps = H.ROWS_HP
        rs, sched = P.row_step.v[0], P.sched.v
        named = list(range(c.rows)) if ids is None else ids[::c.stride][:n_ids].tolist()
        target = upto + apply
        if apply:
            sched[upto + 1] = T(H.adam_scalars(lr, b1, b2, upto + 1))
        claimed = {}
        for r in named:
            if 1 <= r < c.rows and int(rs[r]) < target:
                claimed.setdefault(int(rs[r]), []).append(r)
                rs[r] = target
        for old, rows in claimed.items():                                  # rows that are equally far behind, as one batch
            p, g, m, v = (b.v[rows] for b in (B.p, B.g, B.m, B.v))
            for s in range(old + 1, upto + (0 if mutant == "replay_short" and upto - old >= 2 else 1)):      # the replay reads the scalars the earlier call filed
                p, m, v = adam1(p, torch.zeros_like(g), m, v, float(sched[s, 0]), float(sched[s, 1]), b1, b2, eps, c.gs, True)
            if apply:
                p, m, v = adam1(p, g, m, v, float(sched[upto + 1, 0]), float(sched[upto + 1, 1]), b1, b2, eps, c.gs, True)
                B.g.v[rows] = 0.0
            B.p.v[rows], B.m.v[rows], B.v.v[rows] = p, m, v
            if B.pack is not None:
                tpr = c.width // c.pack[0]
                for k, r in enumerate(rows):
                    B.pack.v[r * tpr:(r + 1) * tpr] = p[k].view(tpr, c.pack[0]).to(torch.bfloat16)
        if mutant == "row_outside_the_list" and claimed:
            B.m.v[0, 0] = 1e-3                                             # row 0 is never in a list
    return call


def met_one_standin(s, lab, mutant=None):
    """metrics_kernel's counting loops for one impression in numpy fp64: the row [AUC, MRR, nDCG@5, nDCG@10]."""
    c = len(s)
    pos = (lab == 1) if mutant == "label_2_negative" else (lab != 0)
    npos, nneg = int(pos.sum()), c - int(pos.sum())
    if (npos == 0 or nneg == 0) and mutant != "single_class_scored":
        return [-1.0, 0.0, 0.0, 0.0]
    ix = np.nonzero(pos)[0]
    if mutant == "lanes_beyond_64_dropped":
        ix = ix[ix < 64]
    si, j = s[ix][:, None], np.arange(c)[None, :]
    eq = s[None, :] == si
    tie_side = (j < ix[:, None]) if mutant == "earlier_index_first" else (j > ix[:, None])
    r = (s[None, :] > si).sum(1) + (eq & tie_side).sum(1)
    auc = ((s[None, :] < si) & ~pos[None, :]).sum(1).astype(np.float64) + (0.0 if mutant == "no_half_credit" else 0.5) * (eq & ~pos[None, :]).sum(1)
    gain = 1.0 / np.log2(r + 2.0)
    ideal = 1.0 / np.log2(np.arange(min(npos, 10)) + 2.0)
    with np.errstate(all="ignore"):
        return [float(auc.sum() / max(npos * nneg, 1)), float((1.0 / (r + 1.0)).sum() / max(npos, 1)), float(gain[r < 5].sum() / max(ideal[:5].sum(), 1e-300)),
                float(gain[r < 10].sum() / max(ideal.sum(), 1e-300))]


def met_standin(P, mutant=None):
    cache = {}
    for i, (s, lab) in enumerate(P.imps):
        key = (s.tobytes(), lab.tobytes())
        if key not in cache:
            cache[key] = met_one_standin(s, lab, mutant)
        P.per.v[i] = torch.tensor(cache[key], dtype=torch.float64)
    rows = P.per.v[P.per.v[:, 0] >= 0] if P.n else torch.zeros(0, 4, dtype=torch.float64)
    P.sums.v[0, 0] = float(rows.shape[0])
    P.sums.v[0, 1:] = rows.sum(0)


def asm_standin(P, mutant=None):
    c = P.c
    comb, hist, pos, neg, label = (t.numpy() for t in (P.comb, P.hist, P.pos, P.neg, P.label))
    nbad = 0
    lab = label.copy()
    wrong = (lab < 0) | (lab > c.K)
    nbad += int(wrong.sum())
    lab[wrong] = 0
    j = np.arange(1 + c.K)[None, :]
    negp = np.concatenate([neg, np.zeros((c.B, 1), dtype=neg.dtype)], 1)                  # so that neg[j] exists for j = K
    cut = lab[:, None] + (1 if mutant == "splice_j_le_label" else 0)
    samp = np.where(j < cut, np.take_along_axis(negp, np.minimum(j, c.K) + 0 * cut, 1),
                    np.where(j == cut, pos[:, None], np.take_along_axis(negp, np.maximum(j - 1, 0) + 0 * cut, 1)))
    for ix, out in ((hist, P.history), (samp, P.candidate)):
        wrong = (ix < 0) | (ix >= H.ASM_ROWS)
        nbad += int(wrong.sum()) * (c.F if mutant == "bad_per_feature" else 1)
        out.v[:] = torch.from_numpy(comb[np.where(wrong, 0, ix)].reshape(-1, c.F))
    if P.bad is not None:
        P.bad.v[0, 0] += nbad


def stack_standin(P, mutant=None):
    c = P.c
    if c.ra + c.rb == 0:
        return
    P.out.v[:c.ra], P.out.v[c.ra:] = P.a, P.b
    if P.flags is not None:
        P.flags.v[0, :c.ra] = 1
        if P.mask is None:
            P.flags.v[0, c.ra:] = 1
        else:
            m = P.mask.numpy()
            P.flags.v[0, c.ra:] = torch.from_numpy(((m > 0) if mutant == "mask_positive" else (m != 0)).astype(np.int32))


def check_standin(P, mutant=None):
    c = P.c
    v = (P.buf[::c.stride][:c.count] if c.kind == "ids" else P.buf[:c.count]).numpy().astype(np.int64)
    if mutant == "labels_truncated":
        v = v.astype(np.int32).astype(np.int64)
    P.bad.v[0, 0] += int(((v < 0) | ((v > c.rows) if mutant == "v_gt_rows" else (v >= c.rows))).sum())


# ------------------------------------------------------------------------------------------ (a)
def _same_fp64(r, m, v, p):
    """Two fp64 evaluations of the same update: a few roundings of fp64 apart, relative to the terms each result is made of."""
    for got, want, scale in ((r.m, m, r.m0.abs() + r.gp.abs()), (r.v, v, r.v), (r.p, p, (r.p + r.ss * r.q).abs() + r.ss * (r.m0.abs() + r.gp.abs()) / r.den)):
        assert bool(((got - want).abs() <= 32 * 2.0 ** -53 * scale).all())


@pytest.mark.parametrize("name", ("n1027-chain", "n7-late", "n1027-gzero"))
def test_adam_reference_is_torch_adam_in_fp64(name):
    """_single_tensor_adam of torch/optim/adam.py (no weight decay, no amsgrad), line by line on fp64 tensors."""
    c = ADAM[name]
    P = H.adam_problem(c, DEV)
    lr, beta1, beta2, eps = H.adam_hp(c)
    for step in c.steps:
        param, exp_avg, exp_avg_sq = P.p.v[0].double(), P.m.v[0].double(), P.v.v[0].double()
        grad = H.adam_grad(c, step).double() * H.f32(c.gs)
        r = H.adam_ref64(P.p.v[0], H.adam_grad(c, step), P.m.v[0], P.v.v[0], lr, beta1, beta2, eps, step, H.f32(c.gs))
        exp_avg.lerp_(grad, 1 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(grad, grad.conj(), value=1 - beta2)
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = lr / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        param.addcdiv_(exp_avg, denom, value=-step_size)
        _same_fp64(r, exp_avg, exp_avg_sq, param)


def test_adam_reference_is_the_optimizer_from_a_zero_state():
    c = ADAM["n1027-chain"]
    lr, beta1, beta2, eps = H.adam_hp(c)
    p0, g = H.adam_problem(c, DEV).p.v[0], H.adam_grad(c, 1)
    w = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([w], lr=lr, betas=(beta1, beta2), eps=eps)
    w.grad = g.double() * H.f32(c.gs)
    opt.step()
    r = H.adam_ref64(p0, g, torch.zeros_like(g), torch.zeros_like(g), lr, beta1, beta2, eps, 1, H.f32(c.gs))
    st = opt.state[w]
    _same_fp64(r, st["exp_avg"], st["exp_avg_sq"], w.detach())


def test_adam_scalars_restate_nr_adam_bias():
    lr, b1, b2, _ = H.ROWS_HP
    assert H.adam_scalars(lr, b1, b2, 100000) == (lr, 1.0)
    assert H.adam_scalars(2.0 ** -10, 0.5, 0.75, 1) == (2.0 ** -9, 0.5)
    ss, bc = H.adam_scalars(lr, b1, b2, 3)
    assert abs(ss - lr / (1 - b1 ** 3)) <= 2.0 ** -24 * ss and abs(bc - math.sqrt(1 - b2 ** 3)) <= 2.0 ** -24 * bc and ss == H.f32(ss) and bc == H.f32(bc)


# ------------------------------------------------------------------------------------------ (b)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.json")


def _ref_row(s, lab):
    one = H.met_ref_one([float(x) for x in np.asarray(s, dtype=np.float32)], list(lab))
    return None if one is None else [float(x) for x in one]


def test_metric_reference_equals_the_fixture_where_it_has_no_ties():
    recs = json.load(open(GOLDEN))
    used = 0
    for r in recs:
        s = np.array(r["s"], dtype=np.float32)
        if len(np.unique(s)) < len(s):
            continue
        used += 1
        assert np.abs(np.array(_ref_row(s, r["y"])) - np.array(r["auc_mrr_ndcg5_ndcg10"])).max() < 1e-12
    assert used >= 10


def _argsort_row(s, y):
    """MRR and nDCG from np.argsort(kind="stable")[::-1], the order the header names; a label != 0 has gain 1."""
    yt = (np.asarray(y) != 0).astype(np.float64)[np.argsort(s, kind="stable")[::-1]]
    disc = 1.0 / np.log2(np.arange(len(yt)) + 2.0)
    npos = int(yt.sum())
    return [float((yt / (np.arange(len(yt)) + 1.0)).sum() / npos)] + [float((yt[:k] * disc[:k]).sum() / disc[:min(npos, k)].sum()) for k in (5, 10)]


def _scored_tie_rows():
    for name in ("waves-ties", "ties", "onepos", "n1025"):
        for s, lab in H.met_impressions(name):
            row = _ref_row(s, lab)
            if row is not None:
                yield s, lab, row


def test_metric_reference_on_ties_is_the_stable_argsort_reversed():
    n = 0
    for s, lab, row in _scored_tie_rows():
        n += 1
        assert np.abs(np.array(row[1:]) - np.array(_argsort_row(s, lab))).max() < 1e-12
    assert n > 300


def test_metric_reference_auc_is_sklearn_roc_auc_score():
    """Skipped where sklearn does not import; roc_auc_score refuses infinite scores, so those rows are left to the hand check."""
    roc_auc_score = pytest.importorskip("sklearn.metrics", reason="sklearn does not import here: no comparison with roc_auc_score").roc_auc_score
    n = 0
    for s, lab, row in _scored_tie_rows():
        if np.isfinite(s).all():
            n += 1
            assert abs(row[0] - roc_auc_score(lab != 0, s.astype(np.float64))) < 1e-12
    assert n > 300


def test_metric_reference_by_hand():
    """Four candidates, worked by hand: scores 3 2 2 1, the positives at index 1 and 3.  Descending with the later index first:
    0 2 1 3, so the positives rank 2 and 3; of the negatives (3 and 2) none is below a positive and one ties: AUC = 0.5 / 4."""
    auc, mrr, n5, n10 = H.met_ref_one([3.0, 2.0, 2.0, 1.0], [0, 1, 0, 2])
    assert (auc, mrr) == (H.Fraction(1, 8), H.Fraction(7, 24))
    want = (1 / math.log2(4) + 1 / math.log2(5)) / (1 + 1 / math.log2(3))
    assert abs(n5 - want) < 1e-15 and n5 == n10
    assert H.met_ref_one([0.0, -0.0], [1, 0])[:2] == (H.Fraction(1, 2), H.Fraction(1, 2))          # +0 and -0 tie: the later one first
    assert H.met_ref_one([1.0, 1.0], [1, 1]) is None and H.met_ref_one([], []) is None and H.met_ref_one([1.0], [0]) is None


# ------------------------------------------------------------------------------------------ (c)
def test_every_route_has_two_cases():
    H._count_routes([H.adam_route(c) for c in H.adam_cases()], H.ADAM_ROUTES, "adam_step")
    H._count_routes([H.rows_route(c) for c in H.rows_cases()], H.ROWS_ROUTES, "adam_rows")
    H._count_routes([H.met_route(n) for n in H.MET_CASES], H.MET_ROUTES, "eval_metrics")
    H._count_routes([H.asm_route(c) for c in H.asm_cases()], H.ASM_ROUTES, "assemble_batch")
    H._count_routes([H.stack_route(c) for c in H.stack_cases()], H.STACK_ROUTES, "stack_rows")
    H._count_routes([H.check_route(c) for c in H.check_cases()], H.CHECK_ROUTES, "check_ids / check_labels")


def test_the_tables_hold_what_the_issue_lists():
    ad = H.adam_cases()
    assert {c.n for c in ad} >= set(H.ADAM_SIZES) | {4 * 256 * 8192 + 4 * 256 + 3}
    for n in H.ADAM_SIZES:
        own = [c for c in ad if c.n == n]
        assert {c.steps for c in own} >= {(1, 2, 3), (100000,), (1,)} and {c.zg for c in own} == {0, 1} and {c.kind for c in own} >= {"exact", "gauss"}
    assert {H.f32(c.gs) for c in ad if c.kind != "exact"} == {1.0, 0.5, H.f32(1 / 3)} and {c.kind for c in ad} == set(H.ADAM_KINDS)
    assert all(math.log2(c.gs) == int(math.log2(c.gs)) and c.steps == (1,) for c in ad if c.kind == "exact")
    g = H.adam_grad(ADAM["n1027-chain"], 1).abs()
    assert float(g.min()) < 1e-5 and float(g.max()) > 0.3
    jobs = [c.jobs for c in ad if c.jobs]
    assert {len(j) for j in jobs} == {1, 2, 4} and {(cols, ld - cols) for j in jobs for _, _, cols, ld in j} >= {(4, 0), (4, 4), (4, 316), (300, 0), (300, 4), (300, 20)}
    assert any(j[0][0] > 0 for j in jobs) and any(b[0] > a[0] + a[1] * a[2] for j in jobs for a, b in zip(j, j[1:]))
    assert any(f + r * k == c.n - c.n % 4 and c.n % 4 for c in ad for f, r, k, _ in c.jobs)
    for c in ad:
        for f, r, k, ld in c.jobs:
            assert f % 4 == 0 and k % 4 == 0 and ld % 4 == 0 and ld >= k and f + r * k <= c.n
        for (f, r, k, _), (f2, _, _, _) in zip(c.jobs, c.jobs[1:]):
            assert f + r * k <= f2
    ro = H.rows_cases()
    assert {(c.rows, c.width) for c in ro} >= {(r, w) for r in (2, 5, 300) for w in (4, 8, 1200)} | {(1025, 8192), (H.ROWS_BIG, 8192)}
    assert {c.stride for c in ro} == {1, 3} and (300, 320) in {c.pack for c in ro if c.width == 1200}
    for r in (2, 5, 300):
        for w in (4, 8, 1200):
            assert {None if c.pack is None else c.pack[0] for c in ro if (c.rows, c.width) == (r, w)} >= {None, w, 4}
    sc = H.rows_script(ROWS["r300-w8-nopack"])
    assert {len(x) for x in sc} >= {0, 1, 255, 256, 257, 300} and len(set(sc[0])) == 1 and not [i for i in sc[3] if 1 <= i < 300]
    assert 299 in sc[0] and 299 in sc[6] and not any(299 in x for x in sc[1:6])                 # away for 5 steps, then back
    # id 0 is skipped: 1025 rows own 1024, which fill the capped grid exactly once; the grid-stride cases own more
    assert (1025 - 1) * (8192 // 4) == 8192 * 256 and "apply_grid_stride" not in H.rows_route(ROWS["big-1025"])
    for name in ("big-nopack", "big-pack"):
        assert (ROWS[name].rows - 1) * (8192 // 4) > 8192 * 256 and "apply_grid_stride" in H.rows_route(ROWS[name])
    imps = {n: H.met_impressions(n) for n in H.MET_CASES}
    assert {len(s) for v in imps.values() for s, _ in v} >= {0, 1, 2, 63, 64, 65, 128, 4095, 4096}
    assert {len(v) for v in imps.values()} >= {0, 1, 3, 4, 5, 1023, 1024, 1025, 16385 + 4} and all(len(s) == 2 for s, _ in imps["stride-a"])
    assert {int(x) for v in imps.values() for _, lab in v for x in np.unique(lab)} == {0, 1, 2, -1}
    assert any((s[30:230] == 0.5).all() for s, _ in imps["ties"]) and any(np.signbit(s).any() and (s == 0).all() for s, _ in imps["ties"])
    assert any(np.isinf(s).any() and (np.abs(s[s != 0]) < 1e-38).any() for s, _ in imps["ties"])
    assert any((lab != 0).sum() > 10 for _, lab in imps["waves"]) and any((lab != 0).sum() == 1 and lab[0] for _, lab in imps["onepos"])
    assert any((lab != 0).sum() == 1 and lab[-1] for _, lab in imps["onepos"])
    asm = H.asm_cases()
    assert {(c.B, c.H, c.K) for c in asm} >= {(b, h, k) for b in (1, 3) for h in (0, 1, 50) for k in (0, 1, 4)} and {c.F for c in asm if c.B <= 3} == {1, 7}
    labs = {(x, c.K) for c in asm for x in c.labels}
    assert {(0, 4), (2, 4), (4, 4), (-1, 4), (5, 4), (2 ** 32 + 1, 4)} <= labs and {c.bad for c in asm} == {"prefill", "null"}
    st = H.stack_cases()
    assert {(c.ra == 0, c.rb == 0) for c in st} == {(True, True), (True, False), (False, True), (False, False)} and {c.F for c in st} == {1, 30}
    assert any(c.flags and c.mask and c.rb >= 6 for c in st) and any(not c.flags for c in st) and any(not c.mask and c.rb for c in st)
    ck = H.check_cases()
    for kind in ("ids", "labels"):
        assert {c.count for c in ck if c.kind == kind} >= {0, 1, 255, 256, 257, 1024 * 256 + 77} and {c.rows for c in ck if c.kind == kind} >= {0, 7}
    assert {c.stride for c in ck if c.kind == "ids"} == {1, 3}
    v = H.check_problem(CHECK["labels-257-r7"], DEV).vals.tolist()
    assert {2 ** 32, 2 ** 32 + 1, -2 ** 33, -1, 0, 6, 7} <= set(v)


def test_exact_layer_is_representable():
    """Every intermediate of the exact layer in fp64 survives a round trip through fp32, m' = g'/2, v' = g'^2/4, the quotient is
    +-1/2 and p' = p - sign(g) 2^-10; the packed cases land on bf16 rounding ties."""
    ties = 0
    for c in (c for c in HOST_ADAM if c.kind == "exact"):
        P = H.adam_problem(c, DEV)
        g = H.adam_grad(c, 1)
        assert bool(((g * 4).abs() >= 1).all()) and bool(((g * 4).abs() <= 7).all()) and bool((g * 4 == (g * 4).round()).all())
        assert bool((P.p.v[0] * 1024 == (P.p.v[0] * 1024).round()).all()) and float(P.p.v[0].abs().max()) <= 4.0 + 2.0 ** -9
        r = H.adam_ref64(P.p.v[0], g, P.m.v[0], P.v.v[0], *H.adam_hp(c), 1, H.f32(c.gs))
        assert (r.ss, r.bc) == (2.0 ** -9, 0.5) == H.adam_scalars(*H.adam_hp(c)[:3], 1)
        sq = r.v.sqrt()
        for t in (r.gp, r.gp - r.m0, r.m, (1 - r.b2) * r.gp, (1 - r.b2) * r.gp * r.gp, r.v, sq, sq / r.bc, r.den, r.q, r.ss * r.q, r.p):
            assert torch.equal(t.float().double(), t)
        assert torch.equal(r.m, r.gp / 2) and torch.equal(r.v, r.gp * r.gp / 4) and torch.equal(r.den, r.gp.abs()) and torch.equal(r.q, torch.sign(g).double() / 2)
        assert torch.equal(r.p, P.p.v[0].double() - torch.sign(g).double() * 2.0 ** -10)
        for f, rows, cols, _ in c.jobs:
            ties += int(((r.p[f:f + rows * cols].float().view(torch.int32) & 0xFFFF) == 0x8000).sum())
    assert ties >= 12


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("fused", (True, False), ids=("fma", "no-fma"))
@pytest.mark.parametrize("c", HOST_ADAM, ids=lambda c: c.name)
def test_adam_standin_passes(c, fused):
    w = H.adam_run(c, DEV, adam_standin(fused), twice=False)
    assert all(x <= 1.0 for x in w.values())


@pytest.mark.parametrize("c", HOST_ROWS, ids=lambda c: c.name)
def test_rows_standin_passes(c):
    H.rows_run(c, DEV, dense_rows_standin, rows_standin(), twice=c.rows == 5)


def _met_checked(name, mutant=None):
    P = H.met_problem(name, DEV)
    met_standin(P, mutant)
    return H.met_check(P)


@pytest.mark.parametrize("name", H.MET_CASES)
def test_metrics_standin_passes(name):
    _met_checked(name)


def _asm_checked(c, mutant=None):
    P = H.asm_problem(c, DEV)
    asm_standin(P, mutant)
    return H.asm_check(P)


def _stack_checked(c, mutant=None):
    P = H.stack_problem(c, DEV)
    stack_standin(P, mutant)
    H.stack_check(P)


def _check_checked(c, mutant=None):
    P = H.check_problem(c, DEV)
    check_standin(P, mutant)
    return H.check_check(P)


def test_assemble_stack_and_check_standins_pass():
    for c in H.asm_cases():
        if c.B <= 3:
            _asm_checked(c)
    for c in H.stack_cases():
        _stack_checked(c)
    for c in H.check_cases():
        _check_checked(c)


# ------------------------------------------------------------------------------------------ (e)
def _fails(want, fn, *a, **k):
    with pytest.raises(H.StepCheckError) as ei:
        fn(*a, **k)
    assert ei.value.layer in want, ei.value


ADAM_MUTANTS = [("eps_inside_root", "n1027-chain", ("p",)), ("eps_inside_root", "n5-chain", ("p",)), ("eps_inside_root", "n1023-late", ("p",)),
                ("bc2_sqrt_dropped", "n1027-chain", ("p",)), ("bc2_sqrt_dropped", "n1-chain", ("p",)), ("bc2_sqrt_dropped", "n4-exact", ("exact",)),
                ("grad_scale_dropped", "n1024-chain", ("m",)), ("grad_scale_dropped", "n1024-exact", ("exact",)), ("grad_scale_dropped", "n2-chain", ("m",)),
                ("m_after_use", "n1027-chain", ("p",)), ("m_after_use", "n3-exact", ("exact",)), ("m_after_use", "n1023-late", ("p",)),
                ("tail_skipped", "n1027-chain", ("m", "grad")), ("tail_skipped", "n5-exact", ("exact", "grad")), ("tail_skipped", "n3-gzero", ("m", "grad")),
                ("tail_skipped", "n1-late", ("m", "grad")),
                ("zero_grad_ignored", "n2-chain", ("grad",)), ("zero_grad_ignored", "n5-exact", ("grad",)),
                ("bf16_truncated", "pack1-exact", ("pack",)), ("bf16_truncated", "pack4-gauss", ("pack",)),
                ("job_ignores_first", "pack1-exact", ("pack",)), ("job_ignores_first", "pack4-gauss", ("pack",)), ("job_ignores_first", "pack2-gauss", ("pack",)),
                ("row_split_by_ld", "pack1-exact", ("sentinel",)), ("row_split_by_ld", "pack1-gauss", ("sentinel",)), ("row_split_by_ld", "pack4-exact", ("sentinel",))]


@pytest.mark.parametrize("mutant,case,want", ADAM_MUTANTS)
def test_adam_mutant_fails_its_layer(mutant, case, want):
    c = ADAM[case]
    if mutant == "zero_grad_ignored":
        assert c.zg == 1
    if mutant == "row_split_by_ld":
        assert any(ld != cols for _, _, cols, ld in c.jobs)
    for fused in (True, False):
        _fails(want, H.adam_run, c, DEV, adam_standin(fused, mutant), twice=False)


def test_a_zero_gradient_left_uncleared_is_the_same_bits():
    """Where the checker has nothing to see: with g = +0 a kernel that ignores zero_grad leaves the bits the contract asks for."""
    c = ADAM["n1027-gzero"]
    assert c.kind == "gzero" and c.zg == 1
    H.adam_run(c, DEV, adam_standin(True, "zero_grad_ignored"), twice=False)


def test_a_second_rows_call_that_differs_in_one_bit_fails():
    calls = []

    def call(P, ids, n_ids, upto, apply):
        rows_standin()(P, ids, n_ids, upto, apply)
        calls.append(P)
        if len(calls) == 6 and P.B.pack is not None:
            P.B.pack.v[2, 1] = 77.0
    _fails(("repeat",), H.rows_run, ROWS["r5-w8-c8ld8"] if "r5-w8-c8ld8" in ROWS else next(c for c in HOST_ROWS if c.pack), DEV, dense_rows_standin, call)


def test_a_second_run_that_differs_in_one_bit_fails():
    calls = []

    def call(P, step):
        adam_standin(True)(P, step)
        calls.append(P)
        if len(calls) == 2:
            P.m.v[0, 0] = (P.m.v[0, :1].view(torch.int32) ^ 1).view(torch.float32)[0]
    _fails(("repeat",), H.adam_run, ADAM["n7-late"], DEV, call, twice=True)


@pytest.mark.parametrize("name", ("r2-w4-nopack", "r5-w8-nopack", "r300-w1200-c300ld320", "r300-w8-nopack"))
def test_rows_mutant_fails_its_layer(name):
    c = ROWS[name]
    _fails(("untouched",), H.rows_run, c, DEV, dense_rows_standin, rows_standin("row_outside_the_list"))


def test_rows_checker_sees_a_lagging_row_and_an_unfiled_step():
    """A replay that stops one step short fails `rows`; an empty step that files nothing fails `sched`."""
    def unfiled(P, ids, n_ids, upto, apply):
        if ids is not None and n_ids == 0:
            return
        rows_standin()(P, ids, n_ids, upto, apply)
    _fails(("rows",), H.rows_run, ROWS["r300-w8-nopack"], DEV, dense_rows_standin, rows_standin("replay_short"))
    _fails(("sched",), H.rows_run, ROWS["r5-w4-nopack"], DEV, dense_rows_standin, unfiled)


MET_MUTANTS = [("earlier_index_first", "waves-ties", "metric"), ("earlier_index_first", "onepos", "metric"), ("earlier_index_first", "lds-onepos", "metric"),
               ("no_half_credit", "ties", "metric"), ("no_half_credit", "stride-a", "metric"), ("no_half_credit", "lds", "metric"),
               ("single_class_scored", "waves", "skip"), ("single_class_scored", "n5", "skip"), ("single_class_scored", "lds-onepos", "skip"),
               ("label_2_negative", "waves", ("metric", "skip")), ("label_2_negative", "onepos", ("metric", "skip")), ("label_2_negative", "stride-b", ("metric", "skip")),
               ("lanes_beyond_64_dropped", "waves", "metric"), ("lanes_beyond_64_dropped", "lds", "metric"), ("lanes_beyond_64_dropped", "ties", "metric")]


@pytest.mark.parametrize("mutant,name,want", MET_MUTANTS)
def test_metrics_mutant_fails_its_layer(mutant, name, want):
    _fails((want,) if isinstance(want, str) else want, _met_checked, name, mutant)


def test_feed_and_check_mutants_fail_their_layers():
    spliced = [c for c in H.asm_cases() if c.B <= 3 and c.K >= 1 and any(0 <= x < c.K for x in c.labels[:c.B])]
    assert len(spliced) >= 3
    for c in spliced:
        _fails(("assemble",), _asm_checked, c, "splice_j_le_label")
    counted = [c for c in H.asm_cases() if c.B <= 3 and c.badidx and c.F > 1 and c.bad == "prefill"]
    assert len(counted) >= 2
    for c in counted:
        _fails(("bad",), _asm_checked, c, "bad_per_feature")
    masked = [c for c in H.stack_cases() if c.mask and c.flags and 6 <= c.rb <= 100]
    assert len(masked) >= 2
    for c in masked:
        _fails(("flags",), _stack_checked, c, "mask_positive")
    big = [c for c in H.check_cases() if c.kind == "labels" and c.count >= 255 and c.rows == 7]
    assert len(big) >= 3
    for c in big:
        _fails(("count",), _check_checked, c, "labels_truncated")
    for c in (c for c in H.check_cases() if c.count >= 255):
        _fails(("count",), _check_checked, c, "v_gt_rows")


@pytest.mark.parametrize("name", ("m", "v", "p"))
@pytest.mark.parametrize("case", ("n1027-chain", "n1023-late", "n4-late"))
def test_adam_one_and_a_half_times_the_bound_fails(case, name):
    """The element with the largest bound moved to 1.5 x that bound from fp64 fails its layer; 0.9 x passes (where the bound is
    wider than the spacing of fp32 around the value, which is everywhere but a p whose own rounding dominates)."""
    c = ADAM[case]
    for k in (0.9, 1.5):
        P = H.adam_problem(c, DEV)
        P.g.v[0] = H.adam_grad(c, c.steps[0])
        pre = tuple(b.v[0].clone() for b in H.adam_bufs(P)[:4])
        adam_standin(True)(P, c.steps[0])
        layer, got, ref, bound = next(t for t in H.adam_terms(P, pre, c.steps[0]) if t[0] == name)
        rel = bound / ref.abs().clamp_min(1e-300)                           # widest relative to the value: fp32 can place it there
        i = int(rel.argmax())
        assert float(rel[i]) > 4 * H.U or name == "m"
        got[i] = float(ref[i] + k * bound[i])
        if k > 1:
            _fails((layer,), H.adam_check, P, pre, c.steps[0])
        elif float(rel[i]) > 16 * H.U:
            H.adam_check(P, pre, c.steps[0])


@pytest.mark.parametrize("col", (0, 1, 2, 3, "sums"))
def test_metrics_one_and_a_half_times_the_bound_fails(col):
    for k in (0.9, 1.5):
        P = H.met_problem("waves-ties", DEV)
        met_standin(P)
        ref, bound, skipped = H.met_terms(P)
        if col == "sums":
            rows = P.per.v[~skipped].tolist()
            want = math.fsum(r[1] for r in rows)
            P.sums.v[0, 2] = want + k * (P.n + 2) * 2.0 ** -53 * want
            layer = "sums"
        else:
            i = int(torch.where(skipped, torch.zeros_like(bound[:, col]), bound[:, col]).argmax())
            assert float(bound[i, col]) > 0
            P.per.v[i, col] = float(ref[i, col] + k * bound[i, col])
            met_fix = P.per.v[~skipped]
            P.sums.v[0, 1:] = torch.tensor([math.fsum(r[j] for r in met_fix.tolist()) for j in range(4)], dtype=torch.float64)
            layer = "metric"
        if k > 1:
            _fails((layer,), H.met_check, P)
        else:
            H.met_check(P)


def test_a_touched_guard_fails_sentinel():
    P = H.met_problem("n5", DEV)
    met_standin(P)
    P.per.flat[P.per.start + 5 * 4] = 0.0
    _fails(("sentinel",), H.met_check, P)
    c = ASM["B3-H1-K4"]
    Q = H.asm_problem(c, DEV)
    asm_standin(Q)
    Q.history.flat[Q.history.start - 1] = 7
    _fails(("sentinel",), H.asm_check, Q)


# ------------------------------------------------------------------------------------------ (f)
def test_refusals_before_any_launch():
    lib, d = _lib.lib(), 4096
    job = lambda first=0, count=1200, cols=300, ld=320, dst=d: _lib.PackJob(first, count, cols, ld, dst)
    hp = (3e-4, 0.9, 0.999, 1e-8, 1, 1.0, 1)

    def packed(jobs, n=4096, n_jobs=None):
        arr = (_lib.PackJob * len(jobs))(*jobs)
        return lib.nr_adam_step_packed(d, d, d, d, n, *hp, arr, len(jobs) if n_jobs is None else n_jobs, None)
    assert packed([job(1200 * j) for j in range(5)], 8192) == 1 and "5 pack jobs (at most 4)" in _lib.last_error(), _lib.last_error()
    for bad in (job(first=2), job(count=1202), job(first=3200), job(cols=302, count=1208), job(ld=296), job(ld=322), job(dst=None), job(dst=d + 4),
                job(cols=0, count=0)):
        assert packed([job(), bad], 4096 + 1200 if bad.first < 3000 else 4096) == 1 and "pack job 1" in _lib.last_error(), (_lib.last_error(), bad.first, bad.count)
    assert packed([job()], 4096, -1) == 1 and "pack jobs" in _lib.last_error()
    assert lib.nr_adam_step_packed(d, d, d, d, 4096, *hp, None, 1, None) == 1 and "pack jobs" in _lib.last_error()
    assert lib.nr_adam_step(d, d, d, d, 16, 3e-4, 0.9, 0.999, 1e-8, 0, 1.0, 1, None) == 1 and "hyper-parameters" in _lib.last_error()
    assert lib.nr_adam_step(d, d, d, d, 16, 3e-4, 1.0, 0.999, 1e-8, 1, 1.0, 1, None) == 1 and "hyper-parameters" in _lib.last_error()
    assert lib.nr_adam_step(d, d, d, d, 16, 3e-4, 0.9, 0.999, -1e-8, 1, 1.0, 1, None) == 1 and "hyper-parameters" in _lib.last_error()
    assert lib.nr_adam_step(d, None, d, d, 16, 3e-4, 0.9, 0.999, 1e-8, 1, 1.0, 1, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_adam_step(d, d, d + 4, d, 16, 3e-4, 0.9, 0.999, 1e-8, 1, 1.0, 1, None) == 1 and "16-byte aligned" in _lib.last_error()
    assert lib.nr_adam_step(None, None, None, None, 0, 3e-4, 0.9, 0.999, 1e-8, 1, 1.0, 1, None) == 0            # nothing to do
    assert lib.nr_eval_metrics(d, d, d, 4, 4097, d, 128, d, None) == 1 and "4097 candidates exceeds the limit of 4096" in _lib.last_error()
    assert lib.nr_eval_metrics(d, d, d, 4, -1, d, 128, d, None) == 1 and "exceeds the limit" in _lib.last_error()
    assert lib.nr_eval_metrics(d, d, d, 4, 8, d, 127, d, None) == 1 and "nr_eval_metrics_workspace_bytes" in _lib.last_error()
    assert lib.nr_eval_metrics(d, d, d, 4, 8, d, 128, None, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_eval_metrics(d, d, d, -1, 8, d, 128, d, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_eval_metrics_workspace_bytes(5) == 160 and lib.nr_eval_metrics_workspace_bytes(-1) == 0
    assert lib.nr_assemble_batch(d, 0, 3, d, d, d, d, 2, 2, 2, d, d, d, None) == 1 and "bad sizes" in _lib.last_error()
    assert lib.nr_assemble_batch(d, 5, 0, d, d, d, d, 2, 2, 2, d, d, d, None) == 1 and "bad sizes" in _lib.last_error()
    assert lib.nr_assemble_batch(d, 5, 3, None, d, d, d, 2, 2, 2, d, d, d, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_assemble_batch(d, 5, 3, d, d, None, d, 2, 2, 2, d, d, d, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_assemble_batch(None, 5, 3, None, None, None, None, 0, 2, 2, None, None, None, None) == 0      # B == 0
    assert lib.nr_stack_rows(d, 2, d, 2, 0, d, d, d, None) == 1 and "bad sizes" in _lib.last_error()
    assert lib.nr_stack_rows(None, 2, d, 2, 3, d, d, d, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_stack_rows(d, 2, d, 2, 3, d, None, d, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_stack_rows(None, 0, None, 0, 3, None, None, None, None) == 0
    assert lib.nr_check_ids(d, 4, 0, 7, d, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_check_ids(d, 4, 1, 7, None, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_check_ids(None, 4, 1, 7, d, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_check_ids(None, 0, 1, 7, d, None) == 0
    assert lib.nr_check_labels(d, 4, -1, d, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_check_labels(d, -1, 5, d, None) == 1 and "bad arguments" in _lib.last_error()
    assert lib.nr_check_labels(None, 0, 5, d, None) == 0
