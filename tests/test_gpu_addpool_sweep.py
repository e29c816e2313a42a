"""GPU: every route of additive pooling (nr_additive_pool_fwd / nr_additive_pool_bwd, csrc/nr_api.hip) against fp64, stage
by stage.  The case tables, the route function, the inputs, the fp64 stage references and the checker are the first part of
this file ("additive-pooling sweep"; plain torch, no GPU needed); tests/test_addpool_sweep_host.py imports them and proves on
the CPU that this checker passes a sound stand-in and fails each of twelve subtly wrong ones.  The NT / TN bounds are those of
tests/test_gpu_gemm_sweep.py, imported.

Per call the library is called directly with a PoolDesc (ops.additive_pool cannot express the strides, the pre-fills or
dx == nullptr): `out` and `g` are views with ld > N (sentinel / NaN in the slack), e, alpha, out, dpre and dx start as NaN,
the four weight gradients as small integers, `partial` as 0xff bytes, the x rows of sequences flagged unneeded hold 1e30.
Checked: the exact profiler label set, sentinels bit for bit, no NaN where the contract says written, rows the library may
leave unwritten hold their initial bits or an exact zero, every stage inside its elementwise bound against fp64 computed
from the kernel's own stored inputs to that stage, the whole against oracle.additive_pool autograd in fp64, the forward
bit-equal across two runs, the backward bit-equal across two runs in deterministic mode.

Routes, bounds and measured figures: DESIGN.md "Additive pooling: routes as verified and the sweep".
"""
import collections
import ctypes as C
import math
import sys
from types import SimpleNamespace

import pytest
import torch

import helpers
import test_gpu_gemm_sweep as G
from oracle import nr_oracle as O
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {"bf16": ops.NR_BF16, "f32": ops.NR_F32}


# ------------------------------------------------------------------------------------------ additive-pooling sweep
# Stage bounds (u = 2^-24; r = 2^-8 for bf16 storage, 0 for fp32; every stage from the kernel's own stored inputs):
#   1 e      tanh(x W1^T + b1): the NT-tanh bound of the GEMM sweep (G.gemm_layer2_bound, N products)
#   2 alpha  s = e.w2 + b2, m = max_l s:  |a - a64| <= a64 (2 delta + 2 eta + (L + 4) u) + 2^-126
#              delta = max_l (q + 2) u (|e|.|w2| + |b2|)          the logit, a q-term fp32 dot product
#              eta   = max((|t_l| + 4) u over live l, (|m| + 4) u) + POOL_EXP_EXCESS        t = s - m   (pool_fwd_kernel)
#                      max((|t_l| + 4) u over live l) + POOL_EXP_EXCESS                     t = s       (pool_fused_fwd_kernel)
#                      the device exponential at the arguments it is given (u |t| for the product with log2 e, 4 u for the
#                      hardware exp2 and the roundings); the denominator's error is a weighted mean of the tokens' and, on
#                      pool_fwd_kernel, of the rescaled 1e-8 exp(-m), hence the maximum; 2^-126: a result below the normal
#                      range is flushed to zero.  (The maximum with |m| and the 2^-126 are derived from what the device
#                      computes, 1e-8f * __expf(-m) at |m| up to 95 and flushed subnormals; the fp32 stand-in of the host
#                      file, whose exponential is torch's, stays inside the bound without them.)  The fused kernel subtracts no maximum (exp(s) / (sum + 1e-8) as the model
#                      writes it), so scores beyond the fp32 range of exp (s > 88.7) are outside its contract: the "beyond"
#                      regime runs there with the scores of the "high" regime (DESIGN.md has the measurement behind this)
#   3 out    (L + 2) u sum_l |a_l| |x_l|
#   4 dpre   A_l = sum_c |g_c| |x_lc|, E_dA = ((N + 2) u + rho) A, E_rd = sum_u a_u E_dA,u + (L + 2) u sum_u a_u |dA_u|,
#            E_ds,l = a_l (E_dA,l + E_rd) + 3 u a_l (|dA_l| + |rd|)
#            |dpre - ref| <= E_ds |w2_j| (1 - e^2) + (4 u + r) |ref| + u |ds w2_j| e^2
#              rho = POOL_RHO on the fused backward (g enters the matrix cores as bf16 hi + lo: hi = bf16(g) leaves at most
#              2^-9 |g|, lo = bf16(g - hi) leaves at most 2^-9 of that: 2^-18 |g| per element), 0 on pool_bwd_kernel
#              last term: e * e rounded on its own (fp32 e, no fused multiply-add) is off by u e^2, which (1 - e^2) does not
#              scale down; the stand-in of the host file needs it at |e| near 1, the 4 u |ref| term alone does not cover it
#   5 dw2    sum E_ds |e| + (M + 2) u sum |ds| |e| + u |pre-fill|        db2: the same with |e| = 1
#   6 dx     dpre W1 + a g: the NT bound with the rank-1 term as one more summand, (q + 3) u S + r |ref|, S = |dpre| |W1| + a |g|
#   7 dw1 / db1   the TN bound of the GEMM sweep, M products, the pre-fill in S
#   8 all    oracle.additive_pool autograd in fp64 at the bounds of test_long_additive_pool_against_fp64
#   deterministic mode adds (products) * 2^-36 to stages 5 and 7: every addend is rounded onto the 2^-36 fixed-point grid
U = G.GEMM_U
POOL_RHO = 2.0 ** -18
# Relative error of the device __expf beyond (|t| + 4) u: four times the worst excess measured over the sweep on the MI355X,
# 0 when there is none (DESIGN.md "Additive pooling: routes as verified and the sweep" holds the measurement).
POOL_EXP_EXCESS = 0.0
POOL_SENTINEL = G.GEMM_SENTINEL
NAN_BITS = {torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000}
REGIMES = ("ordinary", "eps", "onehot", "high", "beyond")

# fwd: "fused" | "core";  core: "fused" | "core_g" (flags computed from g) | "core_needed" (the caller's flags) | "core_none"
PoolCase = collections.namedtuple("PoolCase", "name dt n L N q fwd core flags regime mask dx far det")


class PoolCheckError(AssertionError):
    """A failed check of the sweep; `.layer` names it: sentinel, nan, unwritten, zero, exact, e, alpha, out, dpre, dw2, db2,
    dx, dw1, db1, e2e."""

    def __init__(self, layer, msg):
        super().__init__(f"[{layer}] {msg}")
        self.layer = layer


def _c(name, dt, n, L, N, q, fwd, core, flags="none", regime="ordinary", mask=False, dx=True, far=0, det=False):
    return PoolCase(name, dt, n, L, N, q, fwd, core, flags, regime, mask, dx, far, det)


def pool_ld(c):
    """(ldw1, ldw1t, ld_out, ld_g): W1 [q, ldw1] and W1^T [N, ldw1t] zero padded to 32 columns for bf16 (ops.pack)."""
    if c.dt == "bf16":
        return G._rup(c.N, 32), G._rup(c.q, 32), c.N + 4, c.N + 4
    return c.N, c.q, c.N + 4, c.N + 4


def pool_has_flags(c):
    """pool_has_flags (csrc/nr_api.hip): the backward computes per-sequence flags from g and contracts live slabs."""
    M = c.n * c.L
    return c.dt == "bf16" and M % 32 == 0 and c.L <= 32 and M >= 16384 and c.q >= 8 and c.N >= 8


def pool_routes(c):
    """(forward route, backward core route) by the dispatch of nr_additive_pool_fwd / _bwd, restated."""
    ldw1, ldw1t, _, ldg = pool_ld(c)
    window = c.dt == "bf16" and 24 <= c.L <= 32 and 384 < c.N <= 416 and c.N % 8 == 0 and c.q % 8 == 0 and c.n * c.L >= 4096
    fwd = "fused" if window and 8 <= c.q <= 256 and ldw1 >= 416 and not c.mask else "core"
    if pool_has_flags(c):
        fused = c.dx and not c.det and window and 192 < c.q <= 224 and ldw1t >= 224 and ldg % 4 == 0
        return fwd, "fused" if fused else "core_g"
    return fwd, "core_needed" if c.flags != "none" else "core_none"


def _nt_label(c, M, N, K, ldb, epi, seq_nz):
    """Label of nr_launch_gemm_nt for the two NT calls of the pooling (dense rows, ldc == N, output in the compute type):
    epi 3 = fc1 + tanh (tile skipping with flags), epi 1 = dX with the alpha g epilogue."""
    dims = f"N={N},K={K}"
    if c.dt == "bf16" and K >= 192 and ldb >= G._rup(K, 32):
        skip = epi == 3 and seq_nz
        wreg = N % 8 == 0 and M >= 64
        if epi == 3:
            wreg = wreg and 384 < K <= 416 and N <= 256 and (not skip or c.L >= 16)
        else:
            wreg = wreg and 192 < K <= 224 and N <= 512 and c.L >= 16 and M % 4 == 0
        if wreg:
            return f"gemm_nt_wreg{'_needed' if seq_nz else ''}[bf16,epi={epi},{'Mmax' if seq_nz else 'M'}={M},{dims}]"
        return f"gemm_nt_dma{'_needed' if skip else ''}[bf16,epi={epi},{'Mmax' if skip else 'M'}={M},{dims},gap=0]"
    if c.dt == "bf16" and N <= 208:
        return f"gemm_nt_wide[bf16,epi={epi},M={M},{dims}]"
    return f"gemm_nt[{c.dt},rows=0,epi={epi},M={M},{dims}]"


def pool_fwd_labels(c):
    dims, M = f"n={c.n},L={c.L},N={c.N},q={c.q}", c.n * c.L
    if pool_routes(c)[0] == "fused":
        return {f"pool_fused_fwd{'_needed' if c.flags != 'none' else ''}[bf16,{dims}]"}
    return {_nt_label(c, M, c.q, c.N, pool_ld(c)[0], 3, c.flags != "none"), f"pool_core_fwd[{dims}]"}


def pool_bwd_labels(c):
    dims, M = f"n={c.n},L={c.L},N={c.N},q={c.q}", c.n * c.L
    core, flags = pool_routes(c)[1], pool_has_flags(c)
    if flags:
        tn = f"gemm_tn3_live[bf16,Mmax={M},N={c.q},K={c.N},gap=0]"
    else:
        t = G.TNCase("", c.dt, M, c.q, c.N, 0, 0, 0, True)
        tn = G.gemm_tn_label(t._replace(route=G.gemm_tn_route(t)))
    if core == "fused":
        return {f"pool_fused_bwd[bf16,{dims}]", tn}
    out = {f"pool_core_bwd[{dims}]", tn}
    if c.dx:
        out.add(_nt_label(c, M, c.N, c.q, pool_ld(c)[1], 1, flags or c.flags != "none"))
    return out


def pool_cases():
    """The sweep: the smallest shapes that cross each boundary of the dispatch (DESIGN.md lists what each row is for)."""
    cs = [
        # ---- fused forward: L x N x q rotated, n * L just above 4096 and no multiple of 32 where L allows, every flag pattern
        _c("ff-L24", "bf16", 171, 24, 392, 8, "fused", "core_none"),
        _c("ff-L25", "bf16", 164, 25, 400, 136, "fused", "core_needed", "mixed"),
        _c("ff-L31", "bf16", 133, 31, 416, 200, "fused", "core_needed", "dead"),
        _c("ff-L32", "bf16", 128, 32, 392, 256, "fused", "core_needed", "first"),
        _c("ff-n520", "bf16", 520, 30, 400, 200, "fused", "core_needed", "last"),
        _c("ff-L24b", "bf16", 171, 24, 416, 136, "fused", "core_needed", "one"),
        # ---- just outside the fused forward: the GEMM + pool_core_fwd pair
        _c("out-L23", "bf16", 179, 23, 400, 200, "core", "core_none"),
        _c("out-L33", "bf16", 125, 33, 400, 200, "core", "core_none"),
        _c("out-N384", "bf16", 128, 32, 384, 200, "core", "core_none"),
        _c("out-N424", "bf16", 128, 32, 424, 200, "core", "core_none"),
        _c("out-q264", "bf16", 128, 32, 400, 264, "core", "core_none"),
        _c("out-M4064", "bf16", 127, 32, 400, 200, "core", "core_none"),
        _c("out-mask", "bf16", 128, 32, 400, 200, "core", "core_none", mask=True),
        # ---- one shape per fc1 kernel (with and without flags), the L, N and q lists, both branches of the weighted sum
        _c("fc1-wide", "bf16", 13, 5, 16, 8, "core", "core_needed", "mixed"),
        _c("fc1-wide0", "bf16", 7, 64, 8, 8, "core", "core_none", mask=True),
        _c("fc1-tiled", "bf16", 9, 2, 16, 1024, "core", "core_none"),
        _c("fc1-tiledn", "bf16", 9, 2, 16, 1024, "core", "core_needed", "mixed"),
        _c("fc1-dman", "bf16", 13, 5, 400, 200, "core", "core_needed", "mixed"),
        _c("fc1-wregn", "bf16", 9, 16, 400, 200, "core", "core_needed", "mixed"),
        _c("fc1-f32", "f32", 5, 31, 400, 200, "core", "core_none"),
        _c("fc1-f32n", "f32", 14, 31, 400, 200, "core", "core_needed", "mixed", mask=True),
        _c("mask-f32", "f32", 7, 31, 400, 200, "core", "core_none", mask=True),
        _c("N2048", "bf16", 3, 3, 2048, 8, "core", "core_none"),
        _c("N2056", "bf16", 7, 4, 2056, 8, "core", "core_none", mask=True),
        _c("N1024f", "f32", 5, 1, 1024, 4, "core", "core_none"),
        _c("N1028f", "f32", 7, 63, 1028, 4, "core", "core_none", mask=True),
        _c("L65", "bf16", 7, 65, 16, 200, "core", "core_none", mask=True),
        _c("L128f", "f32", 7, 128, 12, 200, "core", "core_none", mask=True),
        _c("q1024f", "f32", 5, 3, 4, 1024, "core", "core_none"),
        # ---- fused backward: (L, n) x q x N rotated, every pattern of zero gradient rows, dx_far_unwritten 0 and 1
        _c("fb-32", "bf16", 512, 32, 400, 200, "fused", "fused"),
        _c("fb-24", "bf16", 684, 24, 392, 208, "fused", "fused", "mixed", far=1),
        _c("fb-30", "bf16", 560, 30, 416, 224, "fused", "fused", "dead"),
        _c("fb-one", "bf16", 512, 32, 416, 200, "fused", "fused", "one", far=1),
        _c("fb-ends", "bf16", 684, 24, 400, 224, "fused", "fused", "ends", far=1),
        _c("fb-mix0", "bf16", 560, 30, 392, 200, "fused", "fused", "mixed"),
        _c("fb-mask", "bf16", 512, 32, 400, 200, "core", "fused", mask=True),
        # ---- flags from g, fused backward refused
        _c("fg-q192", "bf16", 512, 32, 400, 192, "fused", "core_g", "mixed"),
        _c("fg-q232", "bf16", 512, 32, 400, 232, "fused", "core_g", "mixed"),
        _c("fg-nodx", "bf16", 512, 32, 400, 200, "fused", "core_g", "mixed", dx=False),
        _c("fg-det", "bf16", 512, 32, 400, 200, "fused", "core_g", "mixed", det=True),
        # ---- no flags: M just below 16 384, L > 32 (dense tn3), fp32
        _c("M16352", "bf16", 511, 32, 400, 200, "fused", "core_none"),
        _c("L64-tn3", "bf16", 256, 64, 400, 200, "core", "core_none"),
    ]
    # ---- pool_spb (n = 2048, 8192), ysplit (64 and 512 partial rows) and the short last workgroup, at L = 3 and the smallest dims
    for i, n in enumerate((1, 63, 64, 511, 512, 2047, 2048, 2049, 8191, 8192, 8193)):
        dt = ("bf16", "f32")[i % 2]
        d = 8 if dt == "bf16" else 4
        fl = ("none", "mixed")[(i // 2) % 2] if n > 1 else "none"
        cs.append(_c(f"n{n}", dt, n, 3, d, d, "core", "core_needed" if fl != "none" else "core_none", fl))
    cs += [_c("mind-L1", "bf16", 9, 1, 400, 200, "core", "core_none"),
           _c("mind-L33", "f32", 9, 33, 400, 200, "core", "core_none"),
           _c("mind-L64", "bf16", 9, 64, 400, 200, "core", "core_none", mask=True),
           _c("det-f32", "f32", 9, 5, 12, 8, "core", "core_none", det=True)]
    # ---- score regimes on one shape per core route (the backward of the first three runs pool_bwd_kernel)
    for rg in REGIMES[1:]:
        cs += [_c(f"{rg}-ff", "bf16", 171, 24, 400, 200, "fused", "core_none", regime=rg),
               _c(f"{rg}-core", "bf16", 9, 31, 400, 200, "core", "core_none", regime=rg),
               _c(f"{rg}-f32", "f32", 5, 31, 400, 200, "core", "core_none", regime=rg),
               _c(f"{rg}-fb", "bf16", 512, 32, 400, 200, "fused", "fused", regime=rg)]
    # ---- exact layer: W1 = 0, b1 = b2 = 0, small integers, 1 .. 64 live tokens through the mask: alpha = 1 / live exactly
    cs += [_c("exact-bf16", "bf16", 14, 64, 16, 8, "core", "core_none", regime="exact", mask=True),
           _c("exact-f32", "f32", 14, 64, 12, 8, "core", "core_none", regime="exact", mask=True),
           _c("exact-ff", "bf16", 128, 32, 400, 200, "fused", "core_none", regime="exact"),
           _c("exact-fb", "bf16", 512, 32, 400, 200, "fused", "fused", "mixed", regime="exact")]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def pool_case_id(c):
    return f"{c.name}-{c.dt}-n{c.n}-L{c.L}-N{c.N}-q{c.q}-{c.fwd}.{c.core}"


def pool_live(c, g):
    """[n] bool: sequences the caller needs = sequences with a non-zero pooled gradient."""
    n = c.n
    live = torch.zeros(n, dtype=torch.bool)
    if c.flags == "none":
        live[:] = True
    elif c.flags == "mixed":
        live = torch.rand(n, generator=g) < 0.6
        live[n // 2], live[(n // 2 + 1) % n] = True, False
        if n >= 64:
            live[n // 4:n // 4 + 24] = False         # a stretch whose middle is out of reach of every live sequence
    elif c.flags == "first":
        live[0] = True
    elif c.flags == "last":
        live[-1] = True
    elif c.flags == "one":
        live[n // 2] = True
    elif c.flags == "ends":
        live[0] = live[-1] = True
    else:
        assert c.flags == "dead"
    return live


def pool_problem(c, dev, seed=0):
    """Inputs (as the kernels read them), pre-filled outputs and their initial copies for one case."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * c.n + 13 * c.L + 17 * c.N + 19 * c.q + len(c.name))
    tdt = G._tdt(c.dt)
    rd = lambda t: t.to(tdt).float()
    n, L, N, q = c.n, c.L, c.N, c.q
    M = n * L
    ldw1, ldw1t, ldo, ldg = pool_ld(c)
    live = pool_live(c, g)
    mask = None
    if c.regime == "exact":
        x = torch.randint(-3, 4, (n, L, N), generator=g).float()
        W1, b1, w2, b2 = torch.zeros(q, N), torch.zeros(q), torch.randn(q, generator=g), torch.zeros(1)
        gg = torch.randint(-3, 4, (n, N), generator=g).float()
        if c.mask:
            cnt = torch.tensor([k for k in (1, 2, 4, 8, 16, 32, 64) if k <= L])[torch.arange(n) % 7 % sum(k <= L for k in (1, 2, 4, 8, 16, 32, 64))]
            order = torch.rand(n, L, generator=g).argsort(1).argsort(1)
            mask = (order < cnt[:, None]).float()
    else:
        x = rd(torch.randn(n, L, N, generator=g) * 0.5)
        W1, b1 = rd(torch.randn(q, N, generator=g) / N ** 0.5), torch.randn(q, generator=g) * 0.1
        w2, b2 = torch.randn(q, generator=g) / q ** 0.5, torch.randn(1, generator=g) * 0.1
        gg = torch.randn(n, N, generator=g) / n ** 0.5
        if c.regime == "eps":                      # sum exp(s) ~ 2e-8: sum alpha ~ 2/3 and db2 a number of the size of dw2
            w2, b2 = w2 * 0.25, torch.full((1,), math.log(2e-8 / L))
            gg = gg + 2.0 * x.mean(1) / n ** 0.5   # <g, pooled x> of one sign in every sequence: db2 = sum rd (1 - sum alpha) does not cancel
        elif c.regime == "high":                   # finite in fp32 without a maximum subtracted
            b2 = torch.full((1,), 60.0)
        elif c.regime == "beyond":                 # exp(s) itself overflows fp32; the fused forward is asserted up to "high" only
            b2 = torch.full((1,), 60.0 if pool_routes(c)[0] == "fused" else 95.0)
        elif c.regime == "onehot":                 # token i % L of sequence i at s = +20, every other token near -20
            x0 = rd(torch.randn(N, generator=g) * 0.5)
            e0 = torch.tanh(W1.double() @ x0.double() + b1.double())
            w2 = (20.0 * torch.sign(e0) / e0.abs().sum()).float()
            x = rd(-x0 + 0.02 * torch.randn(n, L, N, generator=g))
            x[torch.arange(n), torch.arange(n) % L] = x0
        if c.mask:
            mask = helpers.masks(n, L, g)[0]
    gg[~live] = 0.0
    if c.flags != "none":
        x[~live] = float(rd(torch.tensor(1e30)))
    p = SimpleNamespace(c=c, live=live.to(dev), mask=None if mask is None else mask.to(dev), x=x.to(tdt).to(dev), W1=W1.to(tdt).to(dev),
                        b1=b1.to(dev), w2=w2.to(dev), b2=b2.to(dev), needed=live.to(torch.int32).to(dev) if c.flags != "none" else None)
    p.w1p = torch.zeros(q, ldw1, dtype=tdt, device=dev)
    p.w1p[:, :N] = p.W1
    p.w1t = torch.zeros(N, ldw1t, dtype=tdt, device=dev)
    p.w1t[:, :q] = p.W1.t()
    p.gbuf = torch.full((n + 1, ldg), float("nan"), device=dev)
    p.gbuf[:n, :N] = gg.to(dev)
    p.g = p.gbuf[:n, :N]
    ri = lambda *s: torch.randint(-5, 6, s, generator=g).float().to(dev)
    p.P1, p.Pb1, p.P2, p.Pb2 = ri(q, N), ri(q), ri(q), ri(1)
    return p


def pool_outputs(p):
    """The output buffers in their initial state: NaN where the library writes, integers where it accumulates, the sentinel
    in the slack columns of `out`, in one trailing row and in the tails of the one-dimensional outputs."""
    c, dev, tdt = p.c, p.x.device, p.x.dtype
    n, L, N, q = c.n, c.L, c.N, c.q
    M, ldo, nan = n * L, pool_ld(c)[2], float("nan")
    o = SimpleNamespace(e=torch.full((M, q), nan, dtype=tdt, device=dev), dpre=torch.full((M, q), nan, dtype=tdt, device=dev),
                        dx=torch.full((M, N), nan, dtype=tdt, device=dev) if c.dx else None,
                        alpha=torch.full((M + 4,), POOL_SENTINEL, device=dev), outbuf=torch.full((n + 1, ldo), POOL_SENTINEL, device=dev),
                        dw1buf=torch.full((q + 1, N), POOL_SENTINEL, device=dev), db1buf=torch.full((q + 4,), POOL_SENTINEL, device=dev),
                        dw2buf=torch.full((q + 4,), POOL_SENTINEL, device=dev), db2buf=torch.full((4,), POOL_SENTINEL, device=dev))
    o.alpha[:M] = nan
    o.outbuf[:n, :N] = nan
    o.dw1buf[:q], o.db1buf[:q], o.dw2buf[:q], o.db2buf[:1] = p.P1, p.Pb1, p.P2, p.Pb2
    o.init = {k: getattr(o, k).clone() for k in ("alpha", "outbuf", "dw1buf", "db1buf", "dw2buf", "db2buf")}
    return o


def pool_alpha64(e, w2, b2, mask):
    """fp64 softmax weights from e [n, L, q]: (s, m, alpha), alpha = exp(s) mask / (sum exp(s) mask + 1e-8), the maximum taken
    out of numerator and denominator so that the beyond-fp32 regime has a reference."""
    s = e @ w2 + b2
    m = s.max(1, keepdim=True).values
    ex = torch.exp(s - m)
    if mask is not None:
        ex = ex * mask
    return s, m, ex / (ex.sum(1, keepdim=True) + 1e-8 * torch.exp(-m))


def pool_dpre64(x, e, alpha, g, w2):
    """fp64 backward core: (dA, rd, ds, dpre)."""
    dA = torch.einsum("nlc,nc->nl", x, g)
    rdot = (alpha * dA).sum(1, keepdim=True)
    ds = alpha * (dA - rdot)
    return dA, rdot, ds, ds[..., None] * w2 * (1 - e * e)


def pool_ref64(x, W1, b1, w2, b2, mask, g):
    """The stage references composed, each stage fed the one before: what the host file compares with autograd."""
    e = torch.tanh(x @ W1.t() + b1)
    _, _, alpha = pool_alpha64(e, w2, b2, mask)
    out = (alpha[..., None] * x).sum(1)
    _, _, ds, dpre = pool_dpre64(x, e, alpha, g, w2)
    dx = dpre @ W1 + alpha[..., None] * g[:, None, :]
    return dict(out=out, dx=dx, dw1=torch.einsum("nlq,nlc->qc", dpre, x), db1=dpre.sum((0, 1)), dw2=(ds[..., None] * e).sum((0, 1)),
                db2=ds.sum().reshape(1))


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _sentinels(name, buf, before, rows, cols=None):
    changed = _bits(buf) != _bits(before)
    if buf.dim() == 1:
        changed[:rows] = False
    else:
        changed[:rows, :cols] = False
    if bool(changed.any()):
        raise PoolCheckError("sentinel", f"{name}: {int(changed.sum())} elements outside the output changed, first at {changed.nonzero()[0].tolist()}")


def _no_nan(name, t):
    if bool(torch.isnan(t).any()):
        raise PoolCheckError("nan", f"{name}: {int(torch.isnan(t).sum())} NaN where the contract says written, first at {torch.isnan(t).nonzero()[0].tolist()}")


def _zeros(name, t):
    if t.numel() and not bool((t == 0).all()):
        bad = t != 0
        raise PoolCheckError("zero", f"{name}: {int(bad.sum())} elements of zero-flag or all-masked sequences are not exact zeros, first at "
                                     f"{bad.nonzero()[0].tolist()}: {float(t[tuple(bad.nonzero()[0].tolist())])}")


def _unwritten(name, t, also=None):
    """Every element holds its initial bit pattern (the NaN of the pre-fill) or an exact zero (or satisfies `also`)."""
    ok = ((_bits(t).int() & 0xFFFFFFFF if t.dtype == torch.float32 else _bits(t).int() & 0xFFFF) == NAN_BITS[t.dtype]) | (t == 0)
    if also is not None:
        ok = ok | also(t)
    if t.numel() and not bool(ok.all()):
        raise PoolCheckError("unwritten", f"{name}: {int((~ok).sum())} elements of rows the library may leave unwritten hold neither their initial "
                                          f"bits nor zero, first at {(~ok).nonzero()[0].tolist()}")


def _within(layer, got, ref, bound):
    """got inside ref +- bound elementwise; returns the worst |error| / bound."""
    _no_nan(layer, got)
    if not got.numel():
        return 0.0
    diff = (got.double() - ref).abs()
    ratio = torch.where(diff > 0, diff / bound, torch.zeros_like(diff))
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise PoolCheckError(layer, f"|error| / bound = {worst:.3g} at {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}, bound {float(bound[i]):.3g}")
    return worst


def _near(live, reach):
    """[n] bool: a live sequence lies within `reach` sequences."""
    n = live.numel()
    idx = torch.arange(n, device=live.device)
    cum = torch.cat([torch.zeros(1, dtype=torch.long, device=live.device), live.long().cumsum(0)])
    return (cum[(idx + reach + 1).clamp(max=n)] - cum[(idx - reach).clamp(min=0)]) > 0


def pool_stage_inputs(p, o):
    """What the later stages read, as stored: e and alpha of the live sequences in fp64."""
    c = p.c
    e = o.e.view(c.n, c.L, c.q)[p.live].double()
    a = o.alpha[:c.n * c.L].view(c.n, c.L)[p.live].double()
    return e, a


def pool_alpha_bound(p, e):
    """(a64, bound, t, m) of stage 2 for the live sequences."""
    c, w2, b2 = p.c, p.w2.double(), p.b2.double()
    mask = None if p.mask is None else p.mask[p.live].double()
    s, m, a64 = pool_alpha64(e, w2, b2, mask)
    delta = ((c.q + 2) * U * (e.abs() @ w2.abs() + b2.abs())).max(1, keepdim=True).values
    fused = pool_routes(c)[0] == "fused"
    t = s.abs() if fused else (s - m).abs()
    if mask is not None:
        t = t * mask
    t = t.max(1, keepdim=True).values
    eta = (t if fused else torch.maximum(t, m.abs())) * U + 4 * U + POOL_EXP_EXCESS
    return a64, a64 * (2 * delta + 2 * eta + (c.L + 4) * U) + 2.0 ** -126, s, m


def pool_dpre_bound(p, e, a, fused):
    """(ref, bound, ds, E_ds) of stage 4 for the live sequences, from stored e, alpha and g."""
    c, w2 = p.c, p.w2.double()
    r = 2.0 ** -8 if c.dt == "bf16" else 0.0
    x, g = p.x[p.live].double(), p.g[p.live].double()
    dA, rdot, ds, ref = pool_dpre64(x, e, a, g, w2)
    A = torch.einsum("nlc,nc->nl", x.abs(), g.abs())
    E_dA = ((c.N + 2) * U + (POOL_RHO if fused else 0.0)) * A
    E_rd = (a * E_dA).sum(1, keepdim=True) + (c.L + 2) * U * (a * dA.abs()).sum(1, keepdim=True)
    E_ds = a * (E_dA + E_rd) + 3 * U * a * (dA.abs() + rdot.abs())
    e2 = e * e
    bound = E_ds[..., None] * w2.abs() * (1 - e2) + (4 * U + r) * ref.abs() + U * (ds[..., None] * w2).abs() * e2
    return ref, bound, ds, E_ds


def pool_check_fwd(p, o):
    """Every check of one forward call; returns {stage: worst |error| / bound}."""
    c = p.c
    n, L, N, q = c.n, c.L, c.N, c.q
    M, tdt, live, w = n * L, p.x.dtype, p.live, {}
    _sentinels("out", o.outbuf, o.init["outbuf"], n, N)
    _sentinels("alpha", o.alpha, o.init["alpha"], M)
    e3, al, out = o.e.view(n, L, q), o.alpha[:M].view(n, L), o.outbuf[:n, :N]
    # e rows of unneeded sequences.  On the routes that skip (the fused kernel, the LDS-DMA and weights-in-registers fc1
    # kernels: the "_needed" labels): initial bits or zero where no row tile of any kernel (32 .. 256 rows, aligned) can hold
    # a needed row; elsewhere, and on the wide / tiled / fp32 fc1 kernels, which compute every row, they may also have been
    # computed (a tanh of whatever x held)
    rows_live = live.repeat_interleave(L)
    win = torch.nn.functional.pad(rows_live, (0, (-M) % 256)).view(-1, 256).any(1).repeat_interleave(256)[:M]
    if not any("_needed" in lb for lb in pool_fwd_labels(c)):
        win = torch.ones_like(win)
    _unwritten("e", o.e[~win])
    _unwritten("e", o.e[~rows_live & win], also=lambda t: t.abs() <= 1)
    _zeros("alpha", al[~live])
    _zeros("out", out[~live])
    if not bool(live.any()):
        return w
    x, W1, b1 = p.x[live].double(), p.W1.double(), p.b1.double()
    _no_nan("e", e3[live])
    ref = torch.tanh(x @ W1.t() + b1)
    S = x.abs() @ W1.abs().t() + b1.abs()
    w["e"] = _within("e", e3[live], ref, G.gemm_layer2_bound(ref, S, N, tdt, G.GEMM_TANH_ABS))
    e, a = pool_stage_inputs(p, o)
    a64, bound, s, m = pool_alpha_bound(p, e)
    if p.mask is None and c.regime == "eps":
        assert bool(((a64.sum(1) > 0.3) & (a64.sum(1) < 0.9)).all()), "eps regime: sum alpha of the reference outside (0.3, 0.9)"
    if c.regime == "onehot":
        top = a64.max(1, keepdim=True).values
        assert bool((top > 1 - 1e-12).all()) and bool((a64[a64 < top] < 1e-15).all()), "one-hot regime: reference is not one-hot"
    w["alpha"] = _within("alpha", al[live], a64, bound)
    if p.mask is not None:
        dead = p.mask[live].sum(1) == 0
        _zeros("alpha", al[live][dead])
        _zeros("out", out[live][dead])
    w["out"] = _within("out", out[live], (a[..., None] * x).sum(1), (L + 2) * U * (a[..., None] * x.abs()).sum(1))
    if c.regime == "exact":
        cnt = p.mask[live].sum(1, keepdim=True) if p.mask is not None else torch.full((int(live.sum()), 1), float(L), device=x.device)
        ea = ((1.0 / cnt) * (p.mask[live] if p.mask is not None else 1.0)).expand(-1, L)
        if not (torch.equal(al[live], ea.float()) and torch.equal(out[live], (ea[..., None].double() * x).sum(1).float())):
            raise PoolCheckError("exact", "alpha != 1 / live or out != sum x / live bit for bit")
    return w


def pool_check_bwd(p, o):
    """Every check of one backward call (on the e and alpha that o holds); returns {stage: worst |error| / bound}."""
    c = p.c
    n, L, N, q = c.n, c.L, c.N, c.q
    M, tdt, live, w = n * L, p.x.dtype, p.live, {}
    fused = pool_routes(c)[1] == "fused"
    for k, rows in (("dw1buf", q), ("db1buf", q), ("dw2buf", q), ("db2buf", 1)):
        _sentinels(k, getattr(o, k), o.init[k], rows, N)
    det = (2.0 ** -36) if c.det else 0.0
    dp3 = o.dpre.view(n, L, q)
    near = _near(live, 32 // L + 2) if fused else torch.ones_like(live)
    _zeros("dpre", dp3[~live & near])
    _unwritten("dpre", dp3[~live & ~near])
    if c.dx:
        dx3 = o.dx.view(n, L, N)
        far = ~near if (fused and c.far) else torch.zeros_like(live)
        _zeros("dx", dx3[~live & ~far])
        _unwritten("dx", dx3[~live & far])
    nl = int(live.sum())
    x, g, W1 = p.x[live].double(), p.g[live].double(), p.W1.double()
    e, a = pool_stage_inputs(p, o)
    if nl:
        ref, bound, ds, E_ds = pool_dpre_bound(p, e, a, fused)
        w["dpre"] = _within("dpre", dp3[live], ref, bound)
        if p.mask is not None:                 # an all-masked sequence: alpha = 0, so dpre and dx are exact zeros
            dead = p.mask[live].sum(1) == 0
            _zeros("dpre", dp3[live][dead])
            if c.dx:
                _zeros("dx", dx3[live][dead])
    else:
        ds = E_ds = torch.zeros(0, L, dtype=torch.float64, device=x.device)
    P2, Pb2 = p.P2.double(), p.Pb2.double()
    acc2, accb = (ds[..., None] * e).sum((0, 1)), ds.sum().reshape(1)
    b2w = (E_ds[..., None] * e.abs()).sum((0, 1)) + (M + 2) * U * (ds.abs()[..., None] * e.abs()).sum((0, 1)) + U * P2.abs() + M * det
    b2b = E_ds.sum().reshape(1) + (M + 2) * U * ds.abs().sum().reshape(1) + U * Pb2.abs() + M * det
    if c.regime == "eps" and p.mask is None and nl:
        assert float(accb.abs()) >= 0.1 * float(acc2.abs().max()), "eps regime: reference db2 below 10 % of max |dw2|"
    w["dw2"] = _within("dw2", o.dw2buf[:q], P2 + acc2, b2w)
    w["db2"] = _within("db2", o.db2buf[:1], Pb2 + accb, b2b)
    dp = dp3[live].double()
    if c.dx and nl:
        ref = dp @ W1 + a[..., None] * g[:, None, :]
        S = dp.abs() @ W1.abs() + a[..., None] * g.abs()[:, None, :]
        w["dx"] = _within("dx", dx3[live], ref, G.gemm_layer2_bound(ref, S, q + 1, tdt))
    P1, Pb1 = p.P1.double(), p.Pb1.double()
    ref, S = P1 + torch.einsum("nlq,nlc->qc", dp, x), P1.abs() + torch.einsum("nlq,nlc->qc", dp.abs(), x.abs())
    w["dw1"] = _within("dw1", o.dw1buf[:q], ref, G.gemm_layer2_bound(ref, S, M, torch.float32) + M * det)
    ref, S = Pb1 + dp.sum((0, 1)), Pb1.abs() + dp.abs().sum((0, 1))
    w["db1"] = _within("db1", o.db1buf[:q], ref, G.gemm_layer2_bound(ref, S, M, torch.float32) + M * det)
    if c.regime == "exact":
        if not torch.equal(_bits(o.dw2buf[:q]), _bits(p.P2)):
            raise PoolCheckError("exact", "dw2 != its pre-fill bit for bit (e = 0)")
        if c.dx and nl and not torch.equal(dx3[live], (a[..., None] * g[:, None, :]).to(tdt)):
            raise PoolCheckError("exact", "dx != g / live bit for bit (W1 = 0)")
    return w


def pool_check_e2e(p, o):
    """Stage 8: the whole against oracle.additive_pool autograd in fp64 over the live sequences (the others hold exact zeros and
    add nothing, checked stage by stage), at the bounds of test_long_additive_pool_against_fp64."""
    c = p.c
    n, L, N, q = c.n, c.L, c.N, c.q
    live, w = p.live, {}
    if not bool(live.any()) or c.regime == "exact":      # (the exact layer has its own, bit-for-bit checks: its integer dA of
        return w                                         #  order 100 make dpre, stored as bf16, a test of bf16 and of nothing else)
    leaves = [t.double().requires_grad_(True) for t in (p.x[live], p.W1, p.b1, p.w2.view(1, q), p.b2)]
    ref = O.additive_pool(*leaves, mask=None if p.mask is None else p.mask[live].double())
    ref.backward(p.g[live].double())
    got = [o.outbuf[:n, :N][live], o.dx.view(n, L, N)[live] if c.dx else None, o.dw1buf[:q] - p.P1, o.db1buf[:q] - p.Pb1,
           (o.dw2buf[:q] - p.P2).view(1, q), o.db2buf[:1] - p.Pb2]
    want = [ref.detach()] + [t.grad for t in leaves]
    for i, (name, a, b) in enumerate(zip(("out", "dx", "dw1", "db1", "dw2", "db2"), got, want)):
        if a is None:
            continue
        err, mx = float((a.double() - b).abs().max()), float(b.abs().max())
        tol = 1e-4 if c.dt == "f32" else ((2e-2 * mx + 1e-3) if i == 0 else (3e-2 * mx + 1e-2))
        w["e2e_" + name] = err / tol
        if not err <= tol:
            raise PoolCheckError("e2e", f"{name}: max |error| {err:.3g} above {tol:.3g}")
    return w


H = sys.modules[__name__]          # the tests below (and the host file) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
def _profiled(call):
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        rc = call()
        torch.cuda.synchronize()
        return rc, set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)


def _desc(c, p):
    return _lib.PoolDesc(n=c.n, L=c.L, N=c.N, q=c.q, dtype=CODE[c.dt], x=p.x.data_ptr(), mask=_lib.ptr(p.mask), w1=p.w1p.data_ptr(),
                         ldw1=p.w1p.shape[1], b1=p.b1.data_ptr(), w2=p.w2.data_ptr(), b2=p.b2.data_ptr(), seq_needed=_lib.ptr(p.needed),
                         dx_far_unwritten=int(c.far))


def _fwd_call(c, p, o, e_ptr=None):
    d = _desc(c, p)
    return lambda: _lib.lib().nr_additive_pool_fwd(C.byref(d), e_ptr or o.e.data_ptr(), o.alpha.data_ptr(), o.outbuf.data_ptr(), H.pool_ld(c)[2],
                                                   ops._stream())


def _bwd_call(c, p, o):
    d = _desc(c, p)
    nbytes = int(_lib.lib().nr_pool_workspace_bytes(C.byref(d)))
    o.partial = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    o.partial_bytes = d.partial_bytes = nbytes
    return lambda: _lib.lib().nr_additive_pool_bwd(C.byref(d), o.e.data_ptr(), o.alpha.data_ptr(), p.gbuf.data_ptr(), H.pool_ld(c)[3],
                                                   p.w1t.data_ptr(), p.w1t.shape[1], o.dpre.data_ptr(), o.partial.data_ptr(), o.dw1buf.data_ptr(),
                                                   o.db1buf.data_ptr(), o.dw2buf.data_ptr(), o.db2buf.data_ptr(), _lib.ptr(o.dx), ops._stream())


_FWD_KEYS, _BWD_KEYS = ("e", "alpha", "outbuf"), ("dpre", "dx", "dw1buf", "db1buf", "dw2buf", "db2buf")


def _snapshot(o, keys):
    return {k: H._bits(getattr(o, k)).clone() for k in keys if getattr(o, k) is not None}


def _run(c):
    """Forward twice, backward (twice in deterministic mode), every check.  Returns {stage: worst |error| / bound}."""
    p = H.pool_problem(c, DEV)
    o = H.pool_outputs(p)
    gbefore = H._bits(p.gbuf).clone()
    rc, labels = _profiled(_fwd_call(c, p, o))
    _lib.check(rc, "nr_additive_pool_fwd")
    assert labels == H.pool_fwd_labels(c), (labels, H.pool_fwd_labels(c))
    w = H.pool_check_fwd(p, o)
    first, o2 = _snapshot(o, _FWD_KEYS), H.pool_outputs(p)
    _lib.check(_fwd_call(c, p, o2)(), "nr_additive_pool_fwd")
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], H._bits(getattr(o2, k))) for k in _FWD_KEYS), "two forward runs differ"
    if c.det:
        ops.set_deterministic(True, elements=1 << 20)
    try:
        rc, labels = _profiled(_bwd_call(c, p, o))
        _lib.check(rc, "nr_additive_pool_bwd")
        if c.det:
            o2.e, o2.alpha = o.e, o.alpha
            _lib.check(_bwd_call(c, p, o2)(), "nr_additive_pool_bwd")
            torch.cuda.synchronize()
    finally:
        if c.det:
            ops.set_deterministic(False)
    want = H.pool_bwd_labels(c)
    assert labels == want, (labels, want)
    assert bool((o.partial[o.partial_bytes:] == 0xFF).all()), "bytes behind the workspace changed"
    assert torch.equal(H._bits(p.gbuf), gbefore), "g changed"
    w.update(H.pool_check_bwd(p, o))
    if c.det:
        second = _snapshot(o2, _BWD_KEYS)
        assert all(torch.equal(v, second[k]) for k, v in _snapshot(o, _BWD_KEYS).items()), "two deterministic backward runs differ"
    w.update(H.pool_check_e2e(p, o))
    return w


@pytest.mark.parametrize("c", H.pool_cases(), ids=H.pool_case_id)
def test_route(c):
    w = _run(c)
    print("\nPOOL " + H.pool_case_id(c) + " " + c.regime + " " + " ".join(f"{k}={v:.4f}" for k, v in w.items()))


def test_q_above_1024_is_refused():
    """q = 1032: the library's own message, before any pooling kernel (the fc1 GEMM has run: e is its output alone)."""
    c = H._c("q1032", "f32", 3, 3, 4, 1032, "core", "core_none")
    p = H.pool_problem(c, DEV)
    o = H.pool_outputs(p)
    rc, labels = _profiled(_fwd_call(c, p, o))
    assert rc != 0 and "q <= 1024" in _lib.last_error() and not any(k.startswith("pool_") for k in labels), (rc, _lib.last_error(), labels)
    assert torch.equal(H._bits(o.alpha), H._bits(o.init["alpha"])) and torch.equal(H._bits(o.outbuf), H._bits(o.init["outbuf"]))
    o.e.zero_(), o.alpha.zero_()
    rc, labels = _profiled(_bwd_call(c, p, o))
    assert rc != 0 and "<= 1024" in _lib.last_error() and labels == set(), (rc, _lib.last_error(), labels)
    assert all(torch.equal(H._bits(getattr(o, k)), H._bits(o.init[k])) for k in ("dw1buf", "db1buf", "dw2buf", "db2buf"))


def test_misaligned_e_is_refused():
    """e one element into its buffer: no route takes it (the fused kernel, the fc1 GEMM and pool_core_fwd all ask for 16 bytes)."""
    c = H._c("e-off", "bf16", 128, 32, 400, 200, "fused", "core_none")
    p = H.pool_problem(c, DEV)
    o = H.pool_outputs(p)
    big = torch.full((c.n * c.L * c.q + 8,), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc, labels = _profiled(_fwd_call(c, p, o, e_ptr=big.data_ptr() + 2))
    assert rc != 0 and _lib.last_error() and labels == set(), (rc, labels)
    assert bool(torch.isnan(big).all()) and torch.equal(H._bits(o.outbuf), H._bits(o.init["outbuf"]))
