"""CPU proof of the additive-pooling sweep (tests/test_gpu_addpool_sweep.py): its case table, its fp64 stage references and
the power of its checker (all in the first part of that file).  Nothing here touches a GPU.

  (a) the stage-wise fp64 references composed over all stages (pool_ref64) equal torch autograd of oracle.additive_pool in
      fp64 to 1e-12 of the largest element, for every score regime, with the seven mask patterns of helpers.masks;
  (b) every case sits on the routes its table row names, by the dispatch of csrc/nr_api.hip restated in pool_routes (the GPU
      file asserts the labels the library itself reports), and each threshold of the dispatch has a case on either side;
  (c) a sound stand-in passes every check of every case: fp32 torch with the kernels' rounding points (e, dpre and dx stored
      in the compute type, g as bf16 hi + lo on the fused backward, the maximum taken out of the softmax except on the
      fused forward, rows of zero-flag sequences left unwritten where the library may), in two summation orders (as
      written, and with every contraction reversed).  No case runs with fewer sequences than on the GPU;
  (d) each mutant of the stand-in fails the layer named.
"""
import pytest
import torch

import test_gpu_addpool_sweep as H
from oracle import nr_oracle as O

DEV = "cpu"
CASES = {c.name: c for c in H.pool_cases()}


def _mm(a, b, order):
    """a @ b in fp32, the contraction as written or reversed."""
    return a @ b if order == 0 else a.flip(-1) @ b.flip(-2)


def standin(p, o, order=0, mutant=None, fwd=True, bwd=True):
    """Writes what sound kernels (or the named mutant of them) would into o."""
    c, tdt = p.c, p.x.dtype
    n, L, N, q = c.n, c.L, c.N, c.q
    live, rd = p.live, (lambda t: t.to(tdt).float())
    nl = int(live.sum())
    x, W1, b1, w2, b2 = p.x[live].float(), p.W1.float(), p.b1, p.w2, p.b2
    mask = None if p.mask is None else p.mask[live]
    fused_bwd = H.pool_routes(c)[1] == "fused"
    e3, al, out = o.e.view(n, L, q), o.alpha[:n * L].view(n, L), o.outbuf[:n, :N]
    if fwd:
        e = torch.tanh((_mm(x, W1.t(), order) + b1).double()).float()
        e3[live] = e.to(tdt)
        e = rd(e)
        s = _mm(e, w2[:, None], order)[..., 0] + b2
        m = s.max(1, keepdim=True).values
        if H.pool_routes(c)[0] == "fused":                 # the fused kernel takes exp(s) as it is
            m = torch.zeros_like(m)
        ex = torch.exp(s - m)
        if mask is not None:
            ex = ex * mask
        eps = 1e-8 * torch.exp(-m)
        if mutant == "eps_dropped":
            eps = 0.0
        if mutant == "eps_unscaled":
            eps = 1e-8
        a = ex / (_mm(ex[:, None, :], torch.ones(L, 1), order)[:, 0] + eps)
        pooled = _mm(a[:, None, :], x, order)[:, 0]
        if mutant == "leak_next_row":
            pooled = pooled + 1e-3 * x.roll(-1, 0)[:, 0]
        al[:], out[:] = 0.0, 0.0
        al[live], out[live] = a, pooled
    if not bwd:
        return
    e, a, g = e3[live].float(), al[live], p.g[live]
    gk = g
    if fused_bwd or mutant == "g_hi_only":
        hi = g.to(torch.bfloat16).float()
        gk = hi if mutant == "g_hi_only" else hi + (g - hi).to(torch.bfloat16).float()
    dA = _mm(x, gk[:, :, None], order)[..., 0]
    rdot = dA.sum(1, keepdim=True) if mutant == "rd_unweighted" else _mm(a[:, None, :], dA[:, :, None], order)[:, 0]
    ds = a * (dA - rdot)
    dpre = ds[..., None] * w2 * ((1 - e) if mutant == "one_minus_e" else (1 - e * e))
    near = H._near(live, 32 // L + 2) if fused_bwd else torch.ones_like(live)
    dp3 = o.dpre.view(n, L, q)
    dp3[~live & near] = 0
    dp3[live] = dpre.to(tdt)
    if mutant == "nan_row" and nl:
        o.dpre[int(live.nonzero()[-1]) * L + L - 1, q // 2] = float("nan")
    dpre = rd(dpre)
    dsw = ds[:-1] if mutant == "dw2_drop_last" else ds
    o.dw2buf[:q] += _mm(dsw.reshape(1, -1), e[:dsw.shape[0]].reshape(-1, q), order)[0]
    if mutant != "db2_zero":
        o.db2buf[:1] += _mm(ds.reshape(1, -1), torch.ones(ds.numel(), 1), order)[0]
    if c.dx:
        dx = _mm(dpre, W1, order)
        if mutant != "no_alpha_g":
            dx = dx + a[..., None] * g[:, None, :]
        dx3 = o.dx.view(n, L, N)
        far = ~near if (fused_bwd and c.far) else torch.zeros_like(live)
        dx3[~live & ~far] = 0
        dx3[live] = dx.to(tdt)
    dw1 = _mm(dpre.reshape(-1, q).t(), x.reshape(-1, N), order)
    if mutant == "dead_in_dw1":
        assert nl < n and nl
        dw1 = dw1 + 1e-3 * dpre[0, 0][:, None] * p.x[~live][0, 0].float()[None, :]
    o.dw1buf[:q] += dw1
    o.db1buf[:q] += _mm(torch.ones(1, dpre.numel() // q), dpre.reshape(-1, q), order)[0]


def _checked(c, order=0, mutant=None):
    p = H.pool_problem(c, DEV)
    o = H.pool_outputs(p)
    standin(p, o, order, mutant)
    w = H.pool_check_fwd(p, o)
    w.update(H.pool_check_bwd(p, o))
    w.update(H.pool_check_e2e(p, o))
    return w


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("regime", H.REGIMES)
def test_stage_references_compose_to_autograd(regime):
    c = H._c("a", "f32", 14, 8, 12, 8, "core", "core_none", regime=regime, mask=True)
    p = H.pool_problem(c, DEV)
    leaves = [t.double().requires_grad_(True) for t in (p.x, p.W1, p.b1, p.w2.view(1, -1), p.b2)]
    ref = O.additive_pool(*leaves, mask=p.mask.double())
    ref.backward(p.g.double())
    got = H.pool_ref64(p.x.double(), p.W1.double(), p.b1.double(), p.w2.double(), p.b2.double(), p.mask.double(), p.g.double())
    want = dict(out=ref.detach(), dx=leaves[0].grad, dw1=leaves[1].grad, db1=leaves[2].grad, dw2=leaves[3].grad[0], db2=leaves[4].grad)
    assert bool((p.mask.sum(1) == 0).any()) and bool((p.mask.sum(1) == c.L).any())
    # db2 = sum_l ds_l cancels to (1 - sum alpha) x (something) outside the eps regime: its scale is that of its summands
    e = torch.tanh(p.x.double() @ p.W1.double().t() + p.b1.double())
    ds = H.pool_dpre64(p.x.double(), e, H.pool_alpha64(e, p.w2.double(), p.b2.double(), p.mask.double())[2], p.g.double(), p.w2.double())[2]
    for k, b in want.items():
        scale = float(ds.abs().sum()) if k == "db2" else float(b.abs().max())
        assert float((got[k] - b).abs().max()) <= 1e-12 * scale, k


# ------------------------------------------------------------------------------------------ (b)
def test_every_case_sits_on_its_declared_routes():
    for c in CASES.values():
        assert H.pool_routes(c) == (c.fwd, c.core), c
        ldw1, ldw1t, ldo, ldg = H.pool_ld(c)
        assert ldo > c.N and ldg > c.N and ldg % 4 == 0 and c.N % (8 if c.dt == "bf16" else 4) == 0


def test_both_sides_of_every_threshold():
    cs = list(CASES.values())
    has = lambda f: any(f(c) for c in cs)
    for L, fwd in ((23, "core"), (24, "fused"), (32, "fused"), (33, "core")):
        assert has(lambda c: c.L == L and c.fwd == fwd), L
    for N, fwd in ((384, "core"), (392, "fused"), (416, "fused"), (424, "core")):
        assert has(lambda c: c.N == N and c.fwd == fwd), N
    for q, fwd in ((256, "fused"), (264, "core")):
        assert has(lambda c: c.q == q and c.fwd == fwd), q
    for q, core in ((192, "core_g"), (200, "fused"), (224, "fused"), (232, "core_g")):
        assert has(lambda c: c.q == q and c.core == core), q
    assert has(lambda c: c.n * c.L == 4064 and c.fwd == "core") and has(lambda c: c.n * c.L == 4096 and c.fwd == "fused")
    assert has(lambda c: c.n * c.L == 16352 and c.core == "core_none") and has(lambda c: c.n * c.L == 16384 and c.core == "fused")
    for n in (63, 64, 511, 512, 2047, 2048, 2049, 8191, 8192, 8193):
        assert has(lambda c: c.n == n and c.L == 3), n
    assert {c.N for c in cs if c.dt == "bf16"} >= {8, 16, 400, 2048, 2056} and {c.N for c in cs if c.dt == "f32"} >= {4, 12, 400, 1024, 1028}
    assert {c.L for c in cs} >= {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 128} and has(lambda c: c.q == 1024)
    assert {c.flags for c in cs if c.fwd == "fused"} >= {"none", "mixed", "dead", "first", "last"}
    assert {c.flags for c in cs if c.core == "fused"} >= {"none", "mixed", "dead", "one", "ends"} and {c.far for c in cs if c.core == "fused"} == {0, 1}
    for route in ("fused", "core"):
        assert {c.regime for c in cs if c.fwd == route} >= set(H.REGIMES)
    assert {c.regime for c in cs if c.core == "fused"} >= set(H.REGIMES) and {c.regime for c in cs if c.dt == "f32"} >= set(H.REGIMES)
    # the seven mask patterns (the seventh masks every token) on each masked core route: pool_fwd_kernel / pool_bwd_kernel in
    # both types and both tokens-per-lane instantiations, every sequence live
    for dt in ("bf16", "f32"):
        for long in (False, True):
            own = [c for c in cs if c.mask and c.dt == dt and (c.L > 64) == long and c.flags == "none" and c.regime == "ordinary" and c.n >= 7]
            assert own, (dt, long)
            for c in own:
                m = H.pool_problem(c, DEV).mask.sum(1)
                assert bool((m == 0).any()) and bool((m == c.L).any()), c
    kinds = set()
    for c in cs:
        kinds |= {lb.split("[")[0] + ("," + lb.split("epi=")[1][0] if "epi=" in lb else "") for lb in H.pool_fwd_labels(c) | H.pool_bwd_labels(c)}
    assert kinds >= {"pool_fused_fwd", "pool_fused_fwd_needed", "pool_core_fwd", "pool_fused_bwd", "pool_core_bwd", "gemm_tn3_live", "gemm_tn3",
                     "gemm_tn2", "gemm_tn", "gemm_nt_wreg,3", "gemm_nt_wreg_needed,3", "gemm_nt_dma,3", "gemm_nt_dma_needed,3", "gemm_nt_wide,3",
                     "gemm_nt,3", "gemm_nt_wreg,1", "gemm_nt_wreg_needed,1", "gemm_nt_dma,1", "gemm_nt_wide,1", "gemm_nt,1"}, kinds


# ------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("c", H.pool_cases(), ids=H.pool_case_id)
def test_sound_standin_passes(c, order):
    _checked(c, order)


# ------------------------------------------------------------------------------------------ (d)
MUTANTS = [("eps_dropped", "eps-f32", "alpha"), ("eps_unscaled", "eps-f32", "alpha"),
           ("leak_next_row", "fc1-f32", "out"), ("leak_next_row", "ff-L24", "out"), ("rd_unweighted", "fc1-f32", "dpre"),
           ("one_minus_e", "fc1-f32", "dpre"), ("one_minus_e", "fb-32", "dpre"), ("dw2_drop_last", "n63", "dw2"), ("dw2_drop_last", "n64", "dw2"),
           ("db2_zero", "eps-f32", "db2"), ("db2_zero", "eps-fb", "db2"), ("no_alpha_g", "fc1-f32", "dx"), ("no_alpha_g", "fb-32", "dx"),
           ("g_hi_only", "fb-32", "dpre"), ("g_hi_only", "fb-24", "dpre"), ("dead_in_dw1", "fc1-wregn", "dw1"), ("dead_in_dw1", "fb-24", "dw1"),
           ("nan_row", "fc1-f32", "nan"), ("nan_row", "fb-32", "nan")]


@pytest.mark.parametrize("mutant,case,layer", MUTANTS)
def test_mutant_fails_its_layer(mutant, case, layer):
    with pytest.raises(H.PoolCheckError) as ei:
        _checked(CASES[case], 0, mutant)
    assert ei.value.layer == layer, ei.value


def test_db2_forced_to_zero_passes_the_ordinary_regime():
    """With ordinary scores sum alpha = 1 and db2 is rounding noise: only the eps-dominated regime sees the mutant."""
    _checked(CASES["fc1-f32"], 0, "db2_zero")


@pytest.mark.parametrize("stage", ("alpha", "out", "dpre", "dx", "dw2", "db2", "dw1", "db1"))
def test_one_and_a_half_times_the_bound_fails(stage):
    """One element moved to 1.5 x its bound away from the fp64 reference fails that stage (0.9 x passes)."""
    for case in ("fc1-f32", "eps-core", "det-f32"):       # det-f32: the M 2^-36 term of deterministic mode is in the bound
        for k, ok in ((0.9, True), (1.5, False)):
            p = H.pool_problem(CASES[case], DEV)
            o = H.pool_outputs(p)
            standin(p, o)
            c = p.c
            e, a = H.pool_stage_inputs(p, o)
            x, g = p.x.double(), p.g.double()
            if stage == "alpha":
                ref, bound, _, _ = H.pool_alpha_bound(p, e)
                o.alpha[:c.n * c.L].view(c.n, c.L)[1, 2] = float(ref[1, 2] + k * bound[1, 2])
                o.outbuf[1, :c.N] = (o.alpha[c.L:2 * c.L, None] * p.x[1].float()).sum(0)       # out follows the stored alpha
                run = lambda: H.pool_check_fwd(p, o)
            elif stage == "out":
                ref, bound = (a[..., None] * x).sum(1), (c.L + 2) * H.U * (a[..., None] * x.abs()).sum(1)
                o.outbuf[1, 3] = float(ref[1, 3] + k * bound[1, 3])
                run = lambda: H.pool_check_fwd(p, o)
            elif stage == "dpre":
                ref, bound, _, _ = H.pool_dpre_bound(p, e, a, False)
                if c.dt == "bf16":
                    continue                  # the perturbed value would be rounded to bf16 again: covered by the fp32 case
                o.dpre.view(c.n, c.L, c.q)[1, 2, 3] = float(ref[1, 2, 3] + k * bound[1, 2, 3])
                run = lambda: H.pool_check_bwd(p, o)
            elif stage == "dx":
                if c.dt == "bf16":
                    continue
                dp = o.dpre.view(c.n, c.L, c.q).double()
                W1 = p.W1.double()
                ref = dp @ W1 + a[..., None] * g[:, None, :]
                bound = H.G.gemm_layer2_bound(ref, dp.abs() @ W1.abs() + a[..., None] * g.abs()[:, None, :], c.q + 1, p.x.dtype)
                o.dx.view(c.n, c.L, c.N)[1, 2, 3] = float(ref[1, 2, 3] + k * bound[1, 2, 3])
                run = lambda: H.pool_check_bwd(p, o)
            elif stage in ("dw1", "db1"):                # the TN bound with the pre-fill in S
                dp, M = o.dpre.view(c.n, c.L, c.q).double(), c.n * c.L
                det = M * 2.0 ** -36 if c.det else 0.0
                if stage == "dw1":
                    ref = p.P1.double() + torch.einsum("nlq,nlc->qc", dp, x)
                    S = p.P1.double().abs() + torch.einsum("nlq,nlc->qc", dp.abs(), x.abs())
                    bound = H.G.gemm_layer2_bound(ref, S, M, torch.float32) + det
                    o.dw1buf[3, 2] = float(ref[3, 2] + k * bound[3, 2])
                else:
                    ref, S = p.Pb1.double() + dp.sum((0, 1)), p.Pb1.double().abs() + dp.abs().sum((0, 1))
                    bound = H.G.gemm_layer2_bound(ref, S, M, torch.float32) + det
                    o.db1buf[3] = float(ref[3] + k * bound[3])
                run = lambda: H.pool_check_bwd(p, o)
            else:
                _, _, ds, E_ds = H.pool_dpre_bound(p, e, a, False)
                M = c.n * c.L
                if stage == "dw2":
                    ref = p.P2.double() + (ds[..., None] * e).sum((0, 1))
                    bound = (E_ds[..., None] * e.abs()).sum((0, 1)) + (M + 2) * H.U * (ds.abs()[..., None] * e.abs()).sum((0, 1)) + H.U * p.P2.abs()
                    o.dw2buf[3] = float(ref[3] + k * bound[3])
                else:
                    ref = p.Pb2.double() + ds.sum()
                    bound = E_ds.sum() + (M + 2) * H.U * ds.abs().sum() + H.U * p.Pb2.abs().double()
                    o.db2buf[0] = float(ref[0] + k * bound[0])
                run = lambda: H.pool_check_bwd(p, o)
            if ok:
                run()
            else:
                with pytest.raises(H.PoolCheckError) as ei:
                    run()
                assert ei.value.layer == stage, ei.value
