"""GPU: the balanced walk of the fused pooling kernels (csrc/nr_gemm.hip, pool_balanced_walk).  With flags, workgroup b0 of G
walks the flagged sequences of RANK b0, b0 + G, ... instead of the flagged ones among the sequences b0, b0 + G, ...: every
flagged sequence must still be computed exactly once, in whatever workgroup it lands, and every other one must get its zeros.

Same reference, poison, label assertions and tolerances as test_fused_pooling_forward_against_the_two_kernel_path
(tests/test_gpu_gemm_wreg.py): the two-kernel path (`NO_POOL_FUSED` = 1) and AttentionPooling in fp64; 1e30 in the x rows of
unneeded sequences; bf16 outputs to 2^-7 of the reference's largest value, fp32 weight gradients to 2e-3 of it, db2 (analytically
zero) to 1e-4 of dw2's scale; exact zeros in the `out` rows of unneeded sequences.

Flag patterns, chosen where a rank walk can go wrong on a device of G workgroups (G = the CU count, 256 on MI355X; the patterns
are written for that G and stay valid checks for any other): all flagged sequences on ONE workgroup of the old partition
(index = 0 mod 256), T > G with wrapping ranks (the first 300), T = G exactly and T = G + 1 (a seeded permutation), a single
flagged sequence at the very end (every wave but the last counts zero), a seeded 55 % draw, none, all, and no flags at all.
n = 1088, L = 30 is 32 640 rows -- a multiple of 32 and >= 16 384, so the fused forward AND the fused backward run, and 17
ballots of 64 flags over 8 waves leave the last waves with a short or empty run; n = 160 (< G: one workgroup per sequence, 3
ballots, five waves with none) runs the fused forward only.

Large n (test_balanced_walk_at_large_n): a wave keeps the first 64 ballots of its run in a register and forms the later ones
again from the flags, so n = 40 000 (79 ballots per wave) drives that second route through both kernels, and n = 140 000 is a
launcher-level check that the walk needs no LDS that grows with n beyond the list: the fused forward must still launch there.
"""
import pytest
import torch

from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, Q = 400, 200


def _bf(x):
    return x.to(torch.bfloat16)


class _opt:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _lib.get_option(self.name)
        _lib.set_option(self.name, self.value)

    def __exit__(self, *a):
        _lib.set_option(self.name, self.old)


def _pool_ref(x, w1, b1, w2, b2):
    """AttentionPooling.forward, src/model/model_utils.py:13-31 (no mask), in fp64 on the given (bf16-representable) inputs."""
    x = x.double()
    e = torch.tanh(x @ w1.double().t() + b1.double())
    alpha = torch.exp(e @ w2.double().reshape(-1, 1) + b2.double())
    alpha = alpha / (alpha.sum(1, keepdim=True) + 1e-8)
    return (x * alpha).sum(1)


def _keep(pattern, n):
    """-> bool [n] on the device, or None for "no flags"."""
    k = torch.zeros(n, dtype=torch.bool)
    cpu = torch.Generator().manual_seed(1000 + n)
    if pattern == "mod256":
        k[::256] = True
    elif pattern == "first300":
        k[:300] = True
    elif pattern in ("perm256", "perm257"):
        k[torch.randperm(n, generator=cpu)[:int(pattern[4:])]] = True
    elif pattern == "last":
        k[n - 1] = True
    elif pattern == "draw55":
        k = torch.rand(n, generator=cpu) < 0.55
    elif pattern == "none_set":
        pass
    elif pattern == "all_set":
        k[:] = True
    else:
        assert pattern == "no_flags"
        return None
    return k.to(DEV)


_inputs = {}


def _case_inputs(n, L):
    """x and the pooling weights of a shape: drawn once, shared by every flag pattern, never modified."""
    if (n, L) not in _inputs:
        g = torch.Generator(device=DEV).manual_seed(n * L + Q)
        x = _bf(torch.randn(n, L, N, device=DEV, generator=g) * 0.5)
        w1 = torch.randn(Q, N, device=DEV, generator=g) * 0.05
        b1 = torch.randn(Q, device=DEV, generator=g) * 0.05
        w2 = torch.randn(1, Q, device=DEV, generator=g) * 0.1
        b2 = torch.randn(1, device=DEV, generator=g) * 0.1
        gout = torch.randn(n, N, device=DEV, generator=g)
        _inputs[(n, L)] = (x, w1, b1, w2, b2, gout)
    return _inputs[(n, L)]


MAIN = ["mod256", "first300", "perm256", "perm257", "last", "draw55", "none_set", "all_set", "no_flags"]


@pytest.mark.parametrize("n,L,pattern", [(1088, 30, p) for p in MAIN] + [(160, 30, "draw55"), (160, 30, "last")])
def test_fused_pooling_with_rank_balanced_walk(n, L, pattern):
    x0, w1_0, b1_0, w2_0, b2_0, gout0 = _case_inputs(n, L)
    w1, b1, w2, b2 = (t.clone().requires_grad_(True) for t in (w1_0, b1_0, w2_0, b2_0))
    keep = _keep(pattern, n)
    x = x0.clone()
    if keep is None:
        needed, keep = None, torch.ones(n, dtype=torch.bool, device=DEV)
    else:
        needed = ops.needed_flags(keep)
        x[~keep] = 1e30        # rides along in the neighbours' stages and must not leak
    gout = gout0 * keep.float().unsqueeze(1)                 # zero on the unflagged rows
    fused_bwd = (n * L) % 32 == 0 and n * L >= 16384

    def run():
        xx = x.clone().requires_grad_(True)
        for p in (w1, b1, w2, b2):
            p.grad = None
        _lib.prof_enable(1)
        try:
            _lib.prof_collect()
            out = ops.additive_pool(xx, w1, b1, w2, b2, ops.NR_BF16, needed=needed)
            out.backward(gout)
            torch.cuda.synchronize()
            labels = set(_lib.prof_collect().keys())
        finally:
            _lib.prof_enable(0)
        dx = xx.grad.detach().float()
        return labels, dx[~keep], (out.detach(), dx[keep], w1.grad.clone(), b1.grad.clone(), w2.grad.clone(), b2.grad.clone())

    lab1, dx_dead, got = run()
    _, _, again = run()
    with _opt("NO_POOL_FUSED", 1):
        lab0, _, old = run()
    has = lambda labs, p: any(l.startswith(p) for l in labs)
    assert has(lab1, "pool_fused_fwd") and not has(lab1, "pool_core_fwd")
    assert has(lab0, "pool_core_fwd") and not has(lab0, "pool_fused_fwd") and not has(lab0, "pool_fused_bwd")
    if fused_bwd:
        assert has(lab1, "pool_fused_bwd") and not has(lab1, "pool_core_bwd")
    else:
        assert has(lab1, "pool_core_bwd") and not has(lab1, "pool_fused_bwd")
    for nm, a, b in zip(["out", "dx", "dw1", "db1", "dw2", "db2"], got, old):
        assert torch.isfinite(a).all(), nm
        if a.numel() == 0:
            continue
        scale = b.abs().max().item()
        tol = (2.0 ** -7 if nm in ("out", "dx") else 2e-3) * scale + 1e-6
        if nm == "db2":      # analytically 0 (the softmax weights sum to 1): rounding noise
            tol = 1e-4 * old[4].abs().max().item() + 1e-6
        err = (a - b).abs().max().item()
        print(f"{pattern} n={n} {nm}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (nm, err, scale)
    if keep.any():
        xr = torch.where(keep[:, None, None], x, torch.zeros_like(x))
        ref = _pool_ref(xr, _bf(w1.detach()), b1.detach(), w2.detach(), b2.detach())
        assert (got[0][keep].double() - ref[keep]).abs().max().item() <= 1e-2 * ref[keep].abs().max().item() + 1e-4
    if (~keep).any():
        assert got[0][~keep].abs().max().item() == 0.0
        if fused_bwd:
            assert dx_dead.abs().max().item() == 0.0          # their dX rows: zeros, written by the strided prologue partition
    # the assignment depends on the flags alone and `out` has one writer per element: two runs agree bit for bit
    assert torch.equal(got[0], again[0])


@pytest.mark.parametrize("n,backward", [(40000, True), (140000, False)])
def test_balanced_walk_at_large_n(n, backward):
    """Against the two-kernel path at the tolerances above (no fp64 pass at this size); a seeded 55 % draw, 1e30 in the rest."""
    L = 30
    g = torch.Generator(device=DEV).manual_seed(n)
    x = (torch.randn(n, L, N, device=DEV, generator=g, dtype=torch.float32) * 0.5).to(torch.bfloat16)
    w1 = (torch.randn(Q, N, device=DEV, generator=g) * 0.05).requires_grad_(True)
    b1 = (torch.randn(Q, device=DEV, generator=g) * 0.05).requires_grad_(True)
    w2 = (torch.randn(1, Q, device=DEV, generator=g) * 0.1).requires_grad_(True)
    b2 = (torch.randn(1, device=DEV, generator=g) * 0.1).requires_grad_(True)
    keep = (torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.55).to(DEV)
    needed = ops.needed_flags(keep)
    x[~keep] = 1e30
    gout = torch.randn(n, N, device=DEV, generator=g) * keep.float().unsqueeze(1)

    def run():
        xx = x.clone().requires_grad_(backward)
        for p in (w1, b1, w2, b2):
            p.grad = None
        _lib.prof_enable(1)
        try:
            _lib.prof_collect()
            with torch.set_grad_enabled(backward):
                out = ops.additive_pool(xx, w1, b1, w2, b2, ops.NR_BF16, needed=needed)
            if backward:
                out.backward(gout)
            torch.cuda.synchronize()
            labels = set(_lib.prof_collect().keys())
        finally:
            _lib.prof_enable(0)
        res = [("out", out.detach())]
        if backward:
            res += [("dx", xx.grad[keep]), ("dx_dead", xx.grad[~keep]), ("dw1", w1.grad.clone()), ("dw2", w2.grad.clone())]
        return labels, res

    lab1, got = run()
    with _opt("NO_POOL_FUSED", 1):
        lab0, old = run()
    has = lambda labs, p: any(l.startswith(p) for l in labs)
    assert has(lab1, "pool_fused_fwd") and not has(lab1, "pool_core_fwd")
    assert has(lab0, "pool_core_fwd") and not has(lab0, "pool_fused_fwd")
    if backward:
        assert has(lab1, "pool_fused_bwd") and not has(lab1, "pool_core_bwd")
    for (nm, a), (_, b) in zip(got, old):
        assert torch.isfinite(a).all(), nm
        if nm == "dx_dead":
            assert a.abs().max().item() == 0.0
            continue
        scale = b.abs().max().item()
        tol = (2.0 ** -7 if nm in ("out", "dx") else 2e-3) * scale + 1e-6
        err = (a.float() - b.float()).abs().max().item()
        print(f"large n={n} {nm}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (nm, err, scale)
    assert got[0][1][~keep].abs().max().item() == 0.0
    assert got[0][1][keep].abs().max().item() > 0.0
