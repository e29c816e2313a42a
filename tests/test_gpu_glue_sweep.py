"""GPU: every route of the second half of csrc/nr_pool.hip against fp64 or bit for bit: the scorer with its cross entropy
(nr_score_ce_fwd / _bwd), the pad-doc blend (nr_pad_blend_fwd / _bwd), the eval scorer (nr_score_eval), the row gathers
(nr_embed_gather_fwd, nr_gather_cast_fwd), the scatter-add (nr_embed_gather_bwd), the operand packers (nr_cast_pad,
nr_cast_pad_batch) and nr_dropout_mask.  The case tables, one route function per entry point (its dispatch restated), the
input builders, the fp64 references and the checker are the first part of this file ("glue sweep"; plain torch, no GPU
needed); tests/test_glue_sweep_host.py imports them and proves on the CPU that the checker passes a sound fp32 stand-in and
fails each of nineteen subtly wrong ones.  The second part calls the C ABI directly (the ops wrappers cannot express
strides, offsets or null arguments).

Every buffer is one flat allocation: [offset][front guard][rows x ld][back guard].  Outputs start as NaN, accumulated
outputs as small integers, slack columns and guards as the sentinel; a "misaligned" buffer starts one element (4 bytes fp32,
2 bytes bf16) into its 16-byte-aligned allocation.  After the call the sentinels are compared bit for bit, the forward is
run twice and compared bit for bit, and every case runs on two input layers:
  lattice  values k 2^-2 with |k| <= 7 (gradients |k| <= 3 on 2^-1), masks exactly 0 or 1: every sum stays far below 2^24
           on its grid (glue_lattice_peak, asserted by the host file), so whatever involves no exp or log equals fp64
  layer2   seeded Gaussians (rounded to the type the kernel reads), checked against the bounds below
Copies (gather, pack, the blend under a binary mask or none) are bit-equal to torch's own rounding on both layers and
carry bf16 rounding ties, +-0, fp32 subnormals and values that round to the largest bf16 or to inf.

Bounds (u = 2^-24; r = 2^-8 for a bf16 result, 0 for fp32), each from the fp64 reference of the same inputs:
  score    (N + 2) u sum_c |cand_c| |user_c|  =: E_s               an N-term fp32 dot product (fma chain, then a wave tree)
  lossvec  2 max_j E_s + (C + 4) u + u |lse| + GLUE_EXP_EXCESS
             lse is 1-Lipschitz in the scores in the max norm and the label's score enters once more: 2 max E_s.  From the
             stored scores: exp(s - max) <= 1 carries a relative error of a few u, the C-term sum (C - 1) u, and the
             logarithm turns the relative error of its argument into an absolute one: (C + 4) u; max + log rounds once:
             u |lse|.  The rounding of lse - s_label, u |loss| <= u (|lse| + |s_label|), is covered by the slack of E_s
             (2 u sum |c| |u| >= 2 u |s| per score, taken twice).  GLUE_EXP_EXCESS: the device expf / logf beyond that.
  loss     mean_b (lossvec bound) + (B + 2) u mean_b |lossvec|      a B-term sum and one division
  dcand / duser (from the score the forward stored, which the backward reads): with t = s - max, p = softmax(s),
             rel_j = ((|t_j| + 4) + sum_k p_k (|t_k| + 4) + (C + 2)) u + GLUE_EXP_EXCESS      exp of a rounded t_j over a
                     C-term sum whose relative error is the p-weighted mean of its terms', one division
             E_d   = |gloss / B| (p rel + 2^-126) + 5 u |(p - 1_label) gloss / B| + u |d|
                     (p - 1, 1 / B, gloss / B, the product, the sum with gscore); without gloss d = gscore exactly: E_d = 0
             dcand = d user:           E_d |user| + u |d user|
             duser = sum_j d_j cand_j: sum_j E_d,j |cand_j| + (C + 2) u sum_j |d_j| |cand_j|
  blend    fractional mask: 3 u (|x m| + |pad (1 - m)|) + r |ref|   (two products, 1 - m, one sum; one rounding to the type)
  dx       fractional mask: u |dout m|                              one product
  dpad     (rows + 2) u sum_r |(1 - m_r) dout_r| + u |pre-fill| (+ rows 2^-36 in deterministic mode: every addend of a
           registered output is rounded onto the 2^-36 grid)
  eval     (N + 2) u sum |news| |user|
  scatter  (count + 1) u (|pre-fill| + sum |dout|) per element: count additions onto the pre-fill, in any order
Layers of GlueCheckError: sentinel, nan, exact, score, loss, dcand, duser, blend, dx, dpad, gather, scatter, pack, mask.
`nan` is scanned where a bound follows (scorer) and on the gathers' outputs; elsewhere a NaN left behind fails the bit
comparison of its own layer.

Routes, derivations, measured figures and what stays uncovered: DESIGN.md "Scorer, blend, gather and packing kernels:
routes as verified and the sweep".
"""
import collections
import math
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_gemm_sweep as G
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------ glue sweep
U = G.GEMM_U
GLUE_SENTINEL = G.GEMM_SENTINEL
# Error of the device expf / logf beyond the analytic part of the lossvec and softmax bounds: four times the worst excess
# measured over the sweep on the MI355X against fp64, 0 when there is none (DESIGN.md holds the measurement).
GLUE_EXP_EXCESS = 0.0
GLUE_GRID = 256 * 16 * 256          # threads of the largest grid of the grid-stride kernels (grid_for, csrc/nr_pool.hip)
LAYERS = ("sentinel", "nan", "exact", "score", "loss", "dcand", "duser", "blend", "dx", "dpad", "gather", "scatter", "pack", "mask")
INPUT_LAYERS = ("lattice", "layer2")
NAN = float("nan")
# fp32 values whose bf16 rounding goes wrong first: ties to even (down, up, negative), just above a tie, +-0, fp32
# subnormals, the smallest bf16 subnormal, half of it (a tie to zero) and three halves (a tie upwards), 3.39e38 (rounds to
# the largest bf16, 3.3895e38), 3.4e38 (rounds to inf) and their negatives
GLUE_SPECIALS = (0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 1e-40, -1e-40, 2.0 ** -133,
                 2.0 ** -134, 3 * 2.0 ** -134, -(2.0 ** -149), 3.39e38, -3.39e38, 3.4e38, -3.4e38, 255.5, 256.5)


class GlueCheckError(AssertionError):
    """A failed check of the sweep; `.layer` is one of LAYERS."""

    def __init__(self, layer, msg):
        assert layer in LAYERS, layer
        super().__init__(f"[{layer}] {msg}")
        self.layer = layer


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def glue_buf(rows, cols, ld, tdt, dev, off=0, fill=NAN):
    """[off elements][front guard: ld rounded up to 8][rows x ld][back guard: ld]; .v is the [rows, cols] view, .ptr its
    address, .own marks its elements, .init is the initial state of the whole allocation."""
    ld = max(ld, 1)
    start = off + G._rup(ld, 8)
    flat = torch.full((start + rows * ld + ld,), GLUE_SENTINEL, dtype=tdt, device=dev)
    v = flat[start:start + rows * ld].view(rows, ld)[:, :cols]
    if isinstance(fill, torch.Tensor):
        v.copy_(fill.reshape(rows, cols))
    else:
        v.fill_(fill)
    own = torch.zeros(flat.numel(), dtype=torch.bool, device=dev)
    own[start:start + rows * ld].view(rows, ld)[:, :cols] = True
    return SimpleNamespace(flat=flat, v=v, own=own, init=flat.clone(), ld=ld, start=start, rows=rows, cols=cols,
                           ptr=flat.data_ptr() + start * flat.element_size())


def _sentinels(name, b):
    changed = (_bits(b.flat) != _bits(b.init)) & ~b.own
    if bool(changed.any()):
        raise GlueCheckError("sentinel", f"{name}: {int(changed.sum())} elements outside the output changed, first at flat index "
                                         f"{int(changed.nonzero()[0])} (output starts at {b.start}, ld {b.ld})")


def _untouched(layer, name, b):
    if not torch.equal(_bits(b.flat), _bits(b.init)):
        raise GlueCheckError(layer, f"{name}: changed by a call that must not write it")


def _no_nan(name, t):
    if bool(torch.isnan(t).any()):
        raise GlueCheckError("nan", f"{name}: {int(torch.isnan(t).sum())} NaN where the contract says written, first at {torch.isnan(t).nonzero()[0].tolist()}")


def _same(layer, name, got, ref):
    """Bit for bit (ref in got's type)."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = _bits(got) != _bits(ref)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise GlueCheckError(layer, f"{name}: {int(bad.sum())} elements differ bit for bit, first at {i}: got {float(got[i])!r}, want {float(ref[i])!r}")


def _equal64(layer, name, got, ref):
    """The fp32 result equals the fp64 reference as a number (lattice inputs; +0 == -0)."""
    bad = ~(got.double() == ref)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise GlueCheckError(layer, f"{name}: {int(bad.sum())} elements differ from fp64 on the lattice, first at {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}")


def _within(layer, name, got, ref, bound):
    """got inside ref +- bound elementwise (a NaN is outside); returns the worst |error| / bound."""
    if not got.numel():
        return 0.0
    diff = (got.double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=diff.device).expand_as(diff)
    bad = ~(diff <= bound)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise GlueCheckError(layer, f"{name}: {int(bad.sum())} elements outside the bound, first at {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}, "
                                    f"bound {float(bound[i]):.3g}")
    return float(torch.where(diff > 0, diff / bound, torch.zeros_like(diff)).max())


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _lat(shape, g, kmax=7, s=2):
    return torch.randint(-kmax, kmax + 1, shape, generator=g).float() * 2.0 ** -s


def _specials(t, shift):
    """Overwrites the head of t (fp32, any shape) with as many GLUE_SPECIALS as fit, rotated by `shift`."""
    k = min(t.numel(), len(GLUE_SPECIALS))
    sp = torch.tensor(GLUE_SPECIALS, dtype=torch.float32).roll(-(shift % len(GLUE_SPECIALS)))
    t.view(-1)[:k] = sp[:k]
    return t


def _count_routes(routes, universe, what):
    cnt = collections.Counter(r for rs in routes for r in rs)
    assert set(cnt) <= set(universe), (what, set(cnt) - set(universe))
    short = {r: cnt[r] for r in universe if cnt[r] < 2}
    assert not short, f"{what}: routes with fewer than two cases: {short}"


def glue_lattice_peak():
    """The largest |sum| the lattice layer can reach in any case, in units of its grid (products of two 2^-2 values: 2^-4)."""
    peak = max(49 * c.N for c in ce_cases())                               # score: N products of |k| <= 7
    peak = max(peak, max(4 * 3 * 2 * 7 * c.C for c in ce_cases()))         # duser: C products gscore (2^-1, 3) x cand on 2^-3
    peak = max(peak, max(49 * c.N for c in eval_cases()))
    peak = max(peak, max(4 * (7 * c.n * c.L + 5 * 4) for c in blend_cases()))   # dpad: rows values on 2^-2 plus the pre-fill
    peak = max(peak, max(4 * (7 * len(scatter_ids(c)) + 5 * 4) for c in scatter_cases()))
    return peak


# ---------------------------------------------------------------------------------------- 1 scorer + cross entropy
CeCase = collections.namedtuple("CeCase", "name B C N pad mode regime padd", defaults=(None,))      # pad: ld_cand - N; padd: ld_dcand - N (None: the same)
CE_MODES = ("gloss", "gscore", "both")
CE_REGIMES = ("ordinary", "big", "equal", "dominant")
CE_ROUTES = ("c_below_8", "c_whole_8", "c_tail_8", "c_64", "n_below_64", "n_whole_64", "n_tail_64", "mean_one_pass", "mean_loop", "ld_dense", "ld_padded",
             "ldd_dense", "ldd_padded")


def ce_cases():
    cs, Bs = [], (1, 3, 255, 257)
    for i, Cn in enumerate((1, 2, 5, 7, 8, 9, 16, 63, 64)):
        cs.append(CeCase(f"C{Cn}", Bs[i % 4], Cn, 65, 3 * (i % 2), CE_MODES[i % 3], "ordinary"))
    for Cn in (5, 9):
        for i, N in enumerate((1, 63, 64, 65, 400)):
            cs.append(CeCase(f"C{Cn}-N{N}", Bs[(i + Cn) % 4], Cn, N, 3 * ((i + 1) % 2), CE_MODES[(i + 1) % 3], "ordinary", 3 * (i % 2)))
    for i, rg in enumerate(CE_REGIMES[1:]):
        cs += [CeCase(f"{rg}-C5", 3, 5, 65, 3, CE_MODES[i % 3], rg), CeCase(f"{rg}-C9", 257, 9, 64, 0, "both", rg),
               CeCase(f"{rg}-C64", 255, 64, 63, 3, "gloss", rg)]
    cs += [CeCase("C64-B257", 257, 64, 65, 0, "both", "ordinary"), CeCase("C1-B1", 1, 1, 1, 0, "both", "ordinary")]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def ce_route(c):
    """score_ce_fwd_kernel has one body; its loop structure by shape: the 8-candidate blocks and their tail, the 64-lane
    column loop and its tail, mean_kernel's 256-thread loop over B, the leading dimensions."""
    return ("c_64" if c.C == 64 else "c_below_8" if c.C < 8 else "c_whole_8" if c.C % 8 == 0 else "c_tail_8",
            "n_below_64" if c.N < 64 else "n_whole_64" if c.N % 64 == 0 else "n_tail_64",
            "mean_one_pass" if c.B <= 256 else "mean_loop", "ld_padded" if c.pad else "ld_dense", "ldd_padded" if (c.pad if c.padd is None else c.padd) else "ldd_dense")


def ce_problem(c, layer, dev):
    g = _gen(1, c.B, c.C, c.N, c.pad, CE_MODES.index(c.mode), CE_REGIMES.index(c.regime), layer == "lattice")
    B, Cn, N = c.B, c.C, c.N
    lab = torch.randint(0, Cn, (B,), generator=g)
    lab[0] = Cn - 1 if B == 1 else 0
    if B > 1:
        lab[1] = Cn - 1
    if layer == "lattice":
        cand, user = _lat((B, Cn, N), g), _lat((B, N), g)
        gscore, gloss = _lat((B, Cn), g, 3, 1), torch.tensor([0.5])
    else:
        user = torch.randn(B, N, generator=g) * 0.5
        cand = torch.randn(B, Cn, N, generator=g) * 0.5
        unit = (user / (user * user).sum(1, keepdim=True).clamp_min(1e-3))[:, None, :]       # <unit, user> = 1
        if c.regime == "big":        # |score| in [80, 90]: beyond 88.7 an exponential taken without the maximum overflows fp32
            tgt = (80 + 10 * torch.rand(B, Cn, generator=g)) * (1 - 2 * ((torch.arange(Cn)[None, :] + torch.arange(B)[:, None]) % 2).float())
            tgt[torch.arange(B) % 3 == 2] = -tgt[torch.arange(B) % 3 == 2].abs()             # whole rows near -80 .. -90 too
            cand = 0.01 * cand + tgt[..., None] * unit
        elif c.regime == "equal":    # every candidate of an impression the same vector: loss = log C
            cand = cand[:, :1].expand(B, Cn, N).clone()
        elif c.regime == "dominant":  # candidate b % C stands 30 above the others; every second label names it
            dom = torch.arange(B) % Cn
            cand[torch.arange(B), dom] += 30 * unit[:, 0]
            lab = torch.where(torch.arange(B) % 2 == 0, dom, (dom + 1) % Cn)
        gscore, gloss = torch.randn(B, Cn, generator=g) * 0.1, torch.tensor([0.7])
    p = SimpleNamespace(c=c, layer=layer, label=lab.to(dev), user=user.to(dev).contiguous(), gloss=gloss.to(dev) if c.mode != "gscore" else None,
                        gscore=gscore.to(dev).contiguous() if c.mode != "gloss" else None)
    p.cand = glue_buf(B * Cn, N, N + c.pad, torch.float32, dev, fill=cand.to(dev))
    p.score, p.lossvec, p.loss = (glue_buf(1, k, k, torch.float32, dev) for k in (B * Cn, B, 1))
    p.dcand = glue_buf(B * Cn, N, N + (c.pad if c.padd is None else c.padd), torch.float32, dev)
    p.duser = glue_buf(B, N, N, torch.float32, dev)
    return p


def ce_ref64(cand, user, label):
    """fp64: (score, lossvec, loss)."""
    score = torch.einsum("bjc,bc->bj", cand, user)
    lossvec = torch.logsumexp(score, 1) - score.gather(1, label[:, None])[:, 0]
    return score, lossvec, lossvec.mean()


def ce_grad64(cand, user, label, score, gloss, gscore):
    """fp64 backward from `score`: (d, dcand, duser), d = (softmax - onehot) gloss / B + gscore."""
    B, Cn = score.shape
    d = torch.zeros_like(score)
    if gloss is not None:
        d = (torch.softmax(score, 1) - torch.nn.functional.one_hot(label, Cn).double()) * (gloss / B)
    if gscore is not None:
        d = d + gscore
    return d, d[..., None] * user[:, None, :], torch.einsum("bj,bjc->bc", d, cand)


def ce_fwd_terms(p):
    """[(layer, name, result view, fp64 reference, bound)] of the forward, and the fp64 scores."""
    c = p.c
    B, Cn, N = c.B, c.C, c.N
    cand, user = p.cand.v.view(B, Cn, N).double(), p.user.double()
    s64, lv64, l64 = ce_ref64(cand, user, p.label)
    Es = (N + 2) * U * torch.einsum("bjc,bc->bj", cand.abs(), user.abs())
    Elv = 2 * Es.max(1).values + (Cn + 4) * U + U * torch.logsumexp(s64, 1).abs() + GLUE_EXP_EXCESS
    return [("score", "score", p.score.v.view(B, Cn), s64, Es), ("loss", "lossvec", p.lossvec.v[0], lv64, Elv),
            ("loss", "loss", p.loss.v[0], l64.reshape(1), (Elv.mean() + (B + 2) * U * lv64.abs().mean()).reshape(1))]


def ce_check_fwd(p):
    c = p.c
    B, Cn = c.B, c.C
    w = {}
    for k in ("score", "lossvec", "loss"):
        _sentinels(k, getattr(p, k))
    terms = ce_fwd_terms(p)
    s64, lv64 = terms[0][3], terms[1][3]
    if p.layer == "layer2" and c.regime == "equal":
        assert float((lv64 - math.log(Cn)).abs().max()) <= 1e-12 * max(1.0, math.log(Cn)), "equal regime: reference loss is not log C"
    if p.layer == "layer2" and c.regime == "dominant" and Cn > 1:
        right = p.label == (torch.arange(B, device=p.label.device) % Cn)
        assert bool((lv64[right] < 1e-6).all()) and bool((lv64[~right] > 20).all()), "dominant regime: reference losses not near 0 / the gap"
    if p.layer == "layer2" and c.regime == "big":
        assert float(s64.abs().max()) > 88.8 and float(s64.abs().min()) > 79, "big regime: scores not in +-[80, 90]"
    for layer, name, got, ref, bound in terms:
        _no_nan(name, got)
        if name == "score" and p.layer == "lattice":
            _equal64("score", "score", got, ref)
        w[name] = _within(layer, name, got, ref, bound)
    return w


def ce_grad_bounds(p):
    """(d64, dcand64, duser64, E_dcand, E_duser) from the stored score."""
    c = p.c
    B, Cn, N = c.B, c.C, c.N
    cand, user, s = p.cand.v.view(B, Cn, N).double(), p.user.double(), p.score.v.view(B, Cn).double()
    gl = None if p.gloss is None else p.gloss.double()
    gs = None if p.gscore is None else p.gscore.double()
    d, dc, du = ce_grad64(cand, user, p.label, s, gl, gs)
    Ed = torch.zeros_like(d)
    if gl is not None:
        t = (s - s.max(1, keepdim=True).values).abs()
        pr = torch.softmax(s, 1)
        rel = ((t + 4) + (pr * (t + 4)).sum(1, keepdim=True) + (Cn + 2)) * U + GLUE_EXP_EXCESS
        ce = (pr - torch.nn.functional.one_hot(p.label, Cn).double()) * (gl / B)
        Ed = (gl / B).abs() * (pr * rel + 2.0 ** -126) + 5 * U * ce.abs() + U * d.abs()
    Edc = Ed[..., None] * user.abs()[:, None, :] + U * dc.abs()
    Edu = torch.einsum("bj,bjc->bc", Ed, cand.abs()) + (Cn + 2) * U * torch.einsum("bj,bjc->bc", d.abs(), cand.abs())
    return d, dc, du, Edc, Edu


def ce_bwd_terms(p):
    c = p.c
    d, dc, du, Edc, Edu = ce_grad_bounds(p)
    return [("dcand", "dcand", p.dcand.v.view(c.B, c.C, c.N), dc, Edc), ("duser", "duser", p.duser.v, du, Edu)]


def ce_check_bwd(p):
    _sentinels("dcand", p.dcand)
    _sentinels("duser", p.duser)
    w = {}
    for layer, name, got, ref, bound in ce_bwd_terms(p):
        _no_nan(name, got)
        if p.layer == "lattice" and p.c.mode == "gscore":
            _equal64(layer, name, got, ref)
        w[name] = _within(layer, name, got, ref, bound)
    return w


# ---------------------------------------------------------------------------------------- 2 pad-doc blend
BlendCase = collections.namedtuple("BlendCase", "name dt n L N mask mis det")
BLEND_MASKS = ("none", "binary", "frac", "nodpad")      # frac: layer2 only (binary on the lattice); nodpad: binary, dpad == NULL
BLEND_ROUTES = ("fwd_vec4", "fwd_scalar", "fwd_vec4_stride", "bwd_vec4", "bwd_vec4_idle", "bwd_scalar")


def blend_cases():
    cs, i = [], 0
    for N in (1, 3, 4, 12, 400, 1024, 1028):
        for n, L in ((1, 1), (3, 5), (7, 50)):
            cs.append(BlendCase(f"N{N}-n{n}", ("bf16", "f32")[i % 2], n, L, N, BLEND_MASKS[(i // 2) % 4], "", False))
            i += 1
    for dt in ("bf16", "f32"):
        cs += [BlendCase(f"stride-{dt}", dt, 2700, 1, 1600, "binary", "", False),      # rows N/4 above the grid: the forward loops
               BlendCase(f"rows65-{dt}", dt, 13, 5, 400, "frac", "", False),           # the second workgroup holds one row
               BlendCase(f"rows65s-{dt}", dt, 13, 5, 3, "frac", "", False),            # scalar backward: the third workgroup holds one row
               BlendCase(f"frac12-{dt}", dt, 7, 50, 12, "frac", "", False),
               BlendCase(f"frac1028-{dt}", dt, 3, 5, 1028, "frac", "", False),
               BlendCase(f"det12-{dt}", dt, 7, 50, 12, "frac", "", True),
               BlendCase(f"det400-{dt}", dt, 13, 5, 400, "binary", "", True),
               BlendCase(f"det1028-{dt}", dt, 3, 5, 1028, "frac", "", True)]
        for mis in ("x", "out", "pad", "dout", "dx"):
            cs.append(BlendCase(f"mis-{mis}-{dt}", dt, 3, 5, 400 if dt == "bf16" else 12, "binary" if mis in ("pad", "out") else "frac", mis, False))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def blend_route(c):
    """nr_pad_blend_fwd: 4 columns per thread when N % 4 == 0 and x, out and pad are 16-byte aligned (pad == NULL counts as
    aligned), one pass unless rows N/4 exceeds the grid.  nr_pad_blend_bwd: 4 columns per thread when N % 4 == 0, N / 4 <= 256
    and dout and dx are aligned; 256 / (N/4) rows side by side, idle threads when N/4 does not divide 256."""
    rows = c.n * c.L
    fv = c.N % 4 == 0 and c.mis not in ("x", "out") and not (c.mis == "pad" and c.mask != "none")
    bv = c.N % 4 == 0 and c.N // 4 <= 256 and c.mis not in ("dout", "dx")
    return ("fwd_scalar" if not fv else "fwd_vec4_stride" if rows * (c.N // 4) > GLUE_GRID else "fwd_vec4",
            "bwd_scalar" if not bv else "bwd_vec4_idle" if 256 % (c.N // 4) else "bwd_vec4")


def blend_problem(c, layer, dev):
    g = _gen(2, c.n, c.L, c.N, BLEND_MASKS.index(c.mask), len(c.mis), c.det, c.dt == "bf16", layer == "lattice")
    tdt, rows, N = G._tdt(c.dt), c.n * c.L, c.N
    frac = c.mask == "frac" and layer == "layer2"
    if layer == "lattice":
        x, pad, dout = _lat((rows, N), g), _lat((N,), g), _lat((rows, N), g)
    else:
        x, pad, dout = torch.randn(rows, N, generator=g), torch.randn(N, generator=g), torch.randn(rows, N, generator=g).to(tdt).float()
    mask = None
    if c.mask != "none":
        mask = torch.rand(rows, generator=g)
        if not frac:
            mask = (mask < 0.6).float()
            mask[0] = float(N % 2) if rows == 1 else 1.0
            if rows > 1:
                mask[1] = 0.0
    if not frac:                      # copies: the values whose rounding goes wrong first
        _specials(x, c.n + N)
        _specials(pad, c.L + N + 5)
    p = SimpleNamespace(c=c, layer=layer, frac=frac, mask=None if mask is None else mask.to(dev))
    off = lambda k: int(c.mis == k)
    p.x = glue_buf(rows, N, N, torch.float32, dev, off("x"), x.to(dev))
    p.pad = glue_buf(1, N, N, torch.float32, dev, off("pad"), pad.to(dev)) if mask is not None else None
    p.out = glue_buf(rows, N, N, tdt, dev, off("out"))
    p.dout = glue_buf(rows, N, N, tdt, dev, off("dout"), dout.to(tdt).to(dev))
    p.dx = glue_buf(rows, N, N, torch.float32, dev, off("dx"))
    p.P = torch.randint(-5, 6, (N,), generator=g).float().to(dev)
    p.dpad = glue_buf(1, N, N, torch.float32, dev, 0, p.P)
    p.use_dpad = c.mask != "nodpad"
    return p


def blend_ref64(x, mask, pad):
    if mask is None:
        return x
    return x * mask[:, None] + pad[None, :] * (1 - mask[:, None])


def blend_terms(p):
    """{layer: (name, result view, fp64 reference, bound or None where the comparison is bit for bit)}."""
    c, rows = p.c, p.c.n * p.c.L
    x, m = p.x.v.double(), None if p.mask is None else p.mask.double()
    pad = None if m is None else p.pad.v[0].double()
    ref = blend_ref64(x, m, pad)
    r = 2.0 ** -8 if c.dt == "bf16" else 0.0
    out = {"blend": ("out", p.out.v, ref, 3 * U * ((x * m[:, None]).abs() + (pad[None, :] * (1 - m[:, None])).abs()) + r * ref.abs() if p.frac else None)}
    d = p.dout.v.double()
    dref = d if m is None else d * m[:, None]
    out["dx"] = ("dx", p.dx.v, dref, U * dref.abs() if p.frac else None)
    if m is not None and p.use_dpad:
        t = (1 - m)[:, None] * d
        out["dpad"] = ("dpad", p.dpad.v[0], p.P.double() + t.sum(0),
                       (rows + 2) * U * t.abs().sum(0) + U * p.P.double().abs() + (rows * 2.0 ** -36 if c.det else 0.0))
    return out


def blend_check_fwd(p):
    _sentinels("out", p.out)
    name, got, ref, bound = blend_terms(p)["blend"]
    if bound is None:                # the selected operand, exactly (fp64 -> fp32 is exact here), rounded once as torch rounds
        _same("exact", name, got, ref.float().to(got.dtype))
        return {}
    return {"blend": _within("blend", name, got, ref, bound)}


def blend_check_dx(p):
    _sentinels("dx", p.dx)
    name, got, ref, bound = blend_terms(p)["dx"]
    if bound is None:
        _same("dx", name, got, ref.float())
        return {}
    return {"dx": _within("dx", name, got, ref, bound)}


def blend_check_dpad(p):
    _sentinels("dpad", p.dpad)
    t = blend_terms(p).get("dpad")
    if t is None:
        _untouched("dpad", "dpad", p.dpad)
        return {}
    name, got, ref, bound = t
    if p.layer == "lattice":
        _equal64("dpad", name, got, ref)
    return {"dpad": _within("dpad", name, got, ref, bound)}


# ---------------------------------------------------------------------------------------- 3 eval scorer
EvalCase = collections.namedtuple("EvalCase", "name N kn ku mis n_cand")
EVAL_ROUTES = ("vec4", "vec4_loop", "scalar", "scalar_loop", "empty")
EVAL_V, EVAL_U = 9, 4


def _ld_kind(cols, k, m=4):
    """0: dense; 1: the next multiple of m above cols; 2: cols + 1."""
    return (cols, G._rup(cols + 1, m), cols + 1)[k]


def eval_cases():
    cs, ncs, i = [], (0, 1, 4, 5, 1027), 0
    for N in (1, 3, 4, 252, 256, 260, 400, 402):
        for kn, ku in ((0, 0), (1, 1), (2, 0), (0, 2), (1, 0)):
            cs.append(EvalCase(f"N{N}-{kn}{ku}", N, kn, ku, "", ncs[(i + 1) % 5]))
            i += 1
    for N in (4, 256, 260, 400):
        cs += [EvalCase(f"mis-news-N{N}", N, 1, 0, "news", 5), EvalCase(f"mis-user-N{N}", N, 0, 1, "user", 1027)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def eval_route(c):
    """score_eval_kernel: 16-byte loads when N, ld_news and ld_user are multiples of 4 and both bases are aligned (a second
    pass of the 64 lanes above N = 256), dword loads otherwise (a second pass above N = 64); n_cand == 0 launches nothing."""
    if c.n_cand == 0:
        return ("empty",)
    vec = (c.N | _ld_kind(c.N, c.kn) | _ld_kind(c.N, c.ku)) % 4 == 0 and not c.mis
    return (("vec4_loop" if c.N > 256 else "vec4") if vec else ("scalar_loop" if c.N > 64 else "scalar"),)


def eval_problem(c, layer, dev):
    g = _gen(3, c.N, c.kn, c.ku, len(c.mis), c.n_cand, layer == "lattice")
    mk = (lambda *s: _lat(s, g)) if layer == "lattice" else (lambda *s: torch.randn(*s, generator=g))
    p = SimpleNamespace(c=c, layer=layer)
    p.news = glue_buf(EVAL_V, c.N, _ld_kind(c.N, c.kn), torch.float32, dev, int(c.mis == "news"), mk(EVAL_V, c.N).to(dev))
    p.user = glue_buf(EVAL_U, c.N, _ld_kind(c.N, c.ku), torch.float32, dev, int(c.mis == "user"), mk(EVAL_U, c.N).to(dev))
    n = max(c.n_cand, 1)
    p.cand_ids = torch.randint(0, EVAL_V, (n,), generator=g, dtype=torch.int32).to(dev)      # 9 rows: repeats from n_cand = 4 on
    p.imp_of = torch.randint(0, EVAL_U, (n,), generator=g, dtype=torch.int32).to(dev)
    if c.n_cand >= 4:
        p.cand_ids[1], p.imp_of[1] = p.cand_ids[0], p.imp_of[0]
    p.score = glue_buf(1, c.n_cand, c.n_cand, torch.float32, dev)
    return p


def eval_terms(p):
    c = p.c
    a, b = p.news.v.double()[p.cand_ids[:c.n_cand].long()], p.user.v.double()[p.imp_of[:c.n_cand].long()]
    return [("score", "score", p.score.v[0], (a * b).sum(1), (c.N + 2) * U * (a.abs() * b.abs()).sum(1))]


def eval_check(p):
    _sentinels("score", p.score)
    if p.c.n_cand == 0:
        return {}
    (layer, name, got, ref, bound), = eval_terms(p)
    _no_nan(name, got)
    if p.layer == "lattice":
        _equal64(layer, name, got, ref)
    return {"score": _within(layer, name, got, ref, bound)}


# ---------------------------------------------------------------------------------------- 4 gathers
GatherCase = collections.namedtuple("GatherCase", "name fn dt cols kt ko mis stride n_ids")
GATHER_ROUTES = tuple(f"{k}_{r}" for k in ("embed_f32", "embed_bf16", "cast_bf16") for r in ("vec", "vec_loop", "scalar", "scalar_loop")) + ("empty",)
GATHER_V = 7


def gather_cases():
    """fn embed: nr_embed_gather_fwd from a table of type dt (fp32 out); fn cast: nr_gather_cast_fwd from an fp32 table to dt."""
    cs, kinds, i = [], ((0, 0), (1, 1), (2, 0), (0, 2), (1, 0), (0, 1)), 0
    for fn, dt in (("embed", "f32"), ("embed", "bf16"), ("cast", "bf16"), ("cast", "f32")):
        for cols in (1, 7, 8, 12, 256, 260, 520):
            for j in range(3):
                kt, ko = kinds[(i + 2 * j) % 6]
                cs.append(GatherCase(f"{fn}-{dt}-c{cols}-{kt}{ko}", fn, dt, cols, kt, ko, "", (1, 3)[(i + j) % 2] if fn == "embed" else 1,
                                     5 if j == 0 else (0, 1, 5)[(i + j) % 3]))
            i += 1
        for cols in (8, 520):
            cs += [GatherCase(f"{fn}-{dt}-c{cols}-mis-table", fn, dt, cols, 1, 1, "table", 1, 5),
                   GatherCase(f"{fn}-{dt}-c{cols}-mis-out", fn, dt, cols, 0, 0, "out", 3 if fn == "embed" else 1, 5),
                   GatherCase(f"{fn}-{dt}-c{cols}-vec", fn, dt, cols, 0, 1, "", 3 if fn == "embed" else 1, 5)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def gather_route(c):
    """gather_fwd_kernel<T>: 16-byte chunks (CH = 4 fp32 / 8 bf16 elements) when cols and ld_table are multiples of CH, ld_out
    of 4, and table and out are aligned; gather_cast_kernel (fp32 -> bf16): 8 elements per lane when cols % 8 == 0,
    ld_table % 4 == 0, ld_out % 8 == 0 and both aligned.  nr_gather_cast_fwd to fp32 IS nr_embed_gather_fwd with ids_stride 1.
    The 64 lanes take a second pass above 64 CH (vector) or 64 (scalar) columns."""
    if c.n_ids == 0:
        return ("empty",)
    ldt, ldo = _ld_kind(c.cols, c.kt, 8), _ld_kind(c.cols, c.ko, 8)
    if c.fn == "cast" and c.dt == "bf16":
        kind, ch, vec = "cast_bf16", 8, c.cols % 8 == 0 and ldt % 4 == 0 and ldo % 8 == 0
    else:
        tab = c.dt if c.fn == "embed" else "f32"
        kind, ch = "embed_" + tab, 4 if tab == "f32" else 8
        vec = c.cols % ch == 0 and ldt % ch == 0 and ldo % 4 == 0
    vec = vec and not c.mis
    return (f"{kind}_{'vec' if vec else 'scalar'}{'_loop' if c.cols > 64 * (ch if vec else 1) else ''}",)


def gather_ids(c):
    real = {0: [], 1: [0] if c.cols % 2 else [2], 5: [3, 0, 3, GATHER_V - 1, 1]}[c.n_ids]
    ids = torch.full((max(c.n_ids * c.stride, 1),), GATHER_V - 2, dtype=torch.int32)         # between the strides: a row nobody asks for
    if real:
        ids[::c.stride][:c.n_ids] = torch.tensor(real, dtype=torch.int32)
    return ids


def gather_problem(c, layer, dev):
    g = _gen(4, c.fn == "cast", c.dt == "bf16", c.cols, c.kt, c.ko, len(c.mis), c.stride, c.n_ids, layer == "lattice")
    tab_dt = G._tdt(c.dt) if c.fn == "embed" else torch.float32
    out_dt = torch.float32 if c.fn == "embed" else G._tdt(c.dt)
    t = _lat((GATHER_V, c.cols), g) if layer == "lattice" else torch.randn(GATHER_V, c.cols, generator=g)
    if layer == "layer2":
        for r in range(GATHER_V):
            _specials(t[r], 3 * r + c.cols)
        if tab_dt == torch.bfloat16:
            t[t.abs() > 3.395e38] = 3.0e38         # a bf16 table holds finite values
    p = SimpleNamespace(c=c, layer=layer, ids=gather_ids(c).to(dev))
    p.table = glue_buf(GATHER_V, c.cols, _ld_kind(c.cols, c.kt, 8), tab_dt, dev, int(c.mis == "table"), t.to(tab_dt).to(dev))
    p.out = glue_buf(c.n_ids, c.cols, _ld_kind(c.cols, c.ko, 8), out_dt, dev, int(c.mis == "out"))
    return p


def gather_check(p):
    c = p.c
    _sentinels("out", p.out)
    if c.n_ids == 0:
        return
    _no_nan("out", p.out.v)
    rows = p.ids[::c.stride][:c.n_ids].long()
    _same("gather", "out", p.out.v, p.table.v[rows].float().to(p.out.v.dtype))


# ---------------------------------------------------------------------------------------- 5 scatter-add
ScatterCase = collections.namedtuple("ScatterCase", "name cols kd kt stride det")
SCATTER_ROUTES = ("one_pass", "lane_loop", "plain", "det_mode")
SCATTER_V = 12
SCATTER_HOT = (1, 2, 5, 7, 9, 11)


def scatter_cases():
    cs = []
    for i, cols in enumerate((1, 4, 65, 130)):
        cs += [ScatterCase(f"c{cols}-a", cols, i % 3, (i + 1) % 3, (1, 3)[i % 2], False),
               ScatterCase(f"c{cols}-b", cols, (i + 2) % 3, i % 3, (3, 1)[i % 2], False),
               ScatterCase(f"c{cols}-det", cols, (i + 1) % 3, (i + 2) % 3, (1, 3)[i % 2], True)]
    return cs


def scatter_route(c):
    """gather_bwd_kernel: one wave per row, the 64 lanes loop above 64 columns; fp32 atomics with and without deterministic
    mode (the entry registers no range: include/nrhip.h K1)."""
    return ("lane_loop" if c.cols > 64 else "one_pass", "det_mode" if c.det else "plain")


def scatter_ids(c):
    """8 rows of id 0 (no gradient), then 200 rows over 6 ids; rows 3, 4, 6, 8, 10 of the table are never named."""
    g = _gen(5, c.cols, c.stride)
    hot = torch.tensor(SCATTER_HOT)[torch.randint(0, 6, (200,), generator=g)]
    return torch.cat([torch.zeros(8, dtype=torch.long), hot]).to(torch.int32)


def scatter_problem(c, layer, dev):
    g = _gen(6, c.cols, c.kd, c.kt, c.stride, c.det, layer == "lattice")
    real = scatter_ids(c)
    n = real.numel()
    ids = torch.full((n * c.stride,), 3, dtype=torch.int32)
    ids[::c.stride] = real
    d = _lat((n, c.cols), g) if layer == "lattice" else torch.randn(n, c.cols, generator=g)
    p = SimpleNamespace(c=c, layer=layer, ids=ids.to(dev), n=n, P=torch.randint(-5, 6, (SCATTER_V, c.cols), generator=g).float().to(dev))
    p.dout = glue_buf(n, c.cols, _ld_kind(c.cols, c.kd), torch.float32, dev, 0, d.to(dev))
    p.dtable = glue_buf(SCATTER_V, c.cols, _ld_kind(c.cols, c.kt), torch.float32, dev, 0, p.P)
    return p


def scatter_ref64(d, ids, P):
    """F.embedding(padding_idx=0) backward onto P: (sum, sum of |addends| with the pre-fill, count) per table row."""
    live = ids != 0
    ref = P.clone().index_add_(0, ids[live], d[live])
    S = P.abs().index_add_(0, ids[live], d[live].abs())
    cnt = torch.zeros(P.shape[0], dtype=torch.float64, device=P.device).index_add_(0, ids[live], torch.ones(int(live.sum()), dtype=torch.float64, device=P.device))
    return ref, S, cnt


def scatter_terms(p):
    ids = p.ids[::p.c.stride][:p.n].long()
    ref, S, cnt = scatter_ref64(p.dout.v.double(), ids, p.P.double())
    return [("scatter", "dtable", p.dtable.v, ref, (cnt[:, None] + 1) * U * S)], cnt == 0


def scatter_check(p):
    _sentinels("dtable", p.dtable)
    ((layer, name, got, ref, bound),), idle = scatter_terms(p)
    assert bool(idle[0]) and int(idle.sum()) >= 2
    _same("scatter", "dtable rows without gradient", got[idle], p.P[idle])
    if p.layer == "lattice":
        _equal64(layer, name, got, ref)
    return {"scatter": _within(layer, name, got, ref, bound)}


def scatter_order_demo():
    """Why the exact fixed-point expectation is not asserted of nr_embed_gather_bwd.  Per id one +1.0, thirty 2^-30, one -1.0:
    a sum in 2^-36 fixed point gives 30 * 2^-30 exactly; sequential fp32 sums of the same addends, ascending, descending and
    in eight seeded random orders.  Returns (expected, [results])."""
    add = torch.tensor([1.0] + [2.0 ** -30] * 30 + [-1.0])
    fixed = float(torch.round(add.double() * 2.0 ** 36).sum() * 2.0 ** -36)
    orders = [add.sort().values, add.sort(descending=True).values] + [add[torch.randperm(32, generator=_gen(7, k))] for k in range(8)]
    out = []
    for o in orders:
        acc = torch.zeros((), dtype=torch.float32)
        for v in o:
            acc = acc + v
        out.append(float(acc))
    return fixed, out


# ---------------------------------------------------------------------------------------- 6 packers
PackCase = collections.namedtuple("PackCase", "name dt rows cols pad_src wide transpose")
PACK_ROUTES = ("one_pass", "stride", "plain", "transposed")
BATCH_ROUTES = ("one_block_job", "whole_blocks_job", "tail_block_job", "plain", "transposed")


def pack_ld(c):
    m = c.rows if c.transpose else c.cols
    return c.cols + c.pad_src, G._rup(m, 32) if c.wide else m


def pack_cases():
    cs, i = [], 0
    for rows, cols in ((1, 1), (3, 5), (5, 3), (200, 400)):
        for tr in (0, 1):
            for pad_src, wide in ((0, 0), (2, 1), (0, 1), (2, 0)):
                cs.append(PackCase(f"{rows}x{cols}-t{tr}-s{pad_src}w{wide}", ("bf16", "f32")[i % 2], rows, cols, pad_src, wide, tr))
                i += 1
    cs += [PackCase("big-bf16", "bf16", 1100, 1000, 0, 1, 0), PackCase("big-f32t", "f32", 1100, 1000, 2, 0, 1)]
    return cs


def pack_route(c):
    drows = c.cols if c.transpose else c.rows
    return ("stride" if drows * pack_ld(c)[1] > GLUE_GRID else "one_pass", "transposed" if c.transpose else "plain")


def batch_cases():
    """{name: (dtype, [PackCase, ...])}: 1, 2 and 16 jobs; 32 x 32 fills exactly one 1024-element block, 64 x 32 two, 25 x 41 =
    1025 spills one element into a second block."""
    j = lambda rows, cols, pad_src, wide, tr: PackCase("", "", rows, cols, pad_src, wide, tr)
    sixteen = [j(1 + 3 * k, 40 - 2 * k, 2 * (k % 2), (k // 2) % 2, k % 2) for k in range(16)]
    sixteen[5], sixteen[6], sixteen[7], sixteen[15] = j(32, 32, 0, 0, 1), j(25, 41, 2, 0, 0), j(32, 64, 2, 0, 1), j(41, 25, 0, 0, 1)
    return {"one-bf16": ("bf16", [j(25, 41, 0, 0, 0)]), "one-f32": ("f32", [j(32, 32, 2, 0, 0)]),
            "two-bf16": ("bf16", [j(64, 32, 0, 0, 0), j(3, 5, 2, 1, 1)]), "two-f32": ("f32", [j(200, 400, 0, 1, 0), j(41, 25, 2, 0, 1)]),
            "sixteen-bf16": ("bf16", sixteen), "sixteen-f32": ("f32", sixteen[::-1])}


def batch_route(jobs):
    out = set()
    for c in jobs:
        total = (c.cols if c.transpose else c.rows) * pack_ld(c)[1]
        out |= {"one_block_job" if total <= 1024 else "whole_blocks_job" if total % 1024 == 0 else "tail_block_job", "transposed" if c.transpose else "plain"}
    return tuple(sorted(out))


def pack_problem(c, dt, layer, dev, salt=0):
    g = _gen(8, c.rows, c.cols, c.pad_src, c.wide, c.transpose, dt == "bf16", layer == "lattice", salt)
    ld_src, ld_dst = pack_ld(c)
    s = _lat((c.rows, c.cols), g) if layer == "lattice" else _specials(torch.randn(c.rows, c.cols, generator=g), c.rows + salt)
    p = SimpleNamespace(c=c, dt=dt, layer=layer)
    p.src = glue_buf(c.rows, c.cols, ld_src, torch.float32, dev, 0, s.to(dev))
    p.dst = glue_buf(c.cols if c.transpose else c.rows, ld_dst, ld_dst, G._tdt(dt), dev)
    return p


def pack_ref(p):
    """include/nrhip.h: dst[r, c] = src[r, c] (transpose 0), dst[c, r] = src[r, c] (transpose 1), zero up to ld_dst."""
    s = p.src.v.t() if p.c.transpose else p.src.v
    return torch.nn.functional.pad(s, (0, p.dst.ld - s.shape[1])).to(p.dst.v.dtype)


def pack_check(p):
    _sentinels("dst", p.dst)
    _same("pack", "dst", p.dst.v, pack_ref(p))


# ---------------------------------------------------------------------------------------- 7 dropout mask
DROP_COUNTS = (1, 2, 3, 1025, 1100000)
DROP_PS = (0.0, 0.2, 0.5, 0.99999)
DROP_SEEDS = (0, 12345, 2 ** 32 - 1)
DROP_ROUTES = ("one_pass", "stride", "off", "on")


def drop_route(count, p):
    return ("stride" if count > GLUE_GRID else "one_pass", "on" if p > 0 else "off")


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def drop_ref(count, p, seed, swap_halves=False):
    """nr_drop_key / nr_pair_hash / nr_keep (csrc/nr_common.h) in numpy uint32: 1.0 where element i is kept."""
    with np.errstate(over="ignore"):
        key = _mix32(np.array([seed], dtype=np.uint32) * np.uint32(0x9E3779B9) + np.uint32(0x7F4A7C15))[0]
        thresh = 0
        if np.float32(p) > 0:
            t = float(np.float32(p)) * 65536.0 + 0.5
            thresh = 65535 if t >= 65535.0 else int(t)
        idx = np.arange(count, dtype=np.uint32)
        h = _mix32((idx >> np.uint32(1)) ^ key)
    odd = (idx & np.uint32(1)).astype(bool) != swap_halves
    half = np.where(odd, h >> np.uint32(16), h & np.uint32(0xFFFF))
    return torch.from_numpy(((thresh == 0) | (half >= thresh)).astype(np.float32))


def drop_check(buf, count, p, seed):
    _sentinels("mask", buf)
    _same("mask", "mask", buf.v[0], drop_ref(count, p, seed).to(buf.v.device))


H = sys.modules[__name__]          # the tests below (and the host file) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
def _L():
    return _lib.lib()


def _ok(rc, what):
    _lib.check(rc, what)
    torch.cuda.synchronize()


def _flats(p, keys):
    return [H._bits(getattr(p, k).flat).clone() for k in keys]


def _report(tag, c, layer, w):
    print(f"\nGLUE {tag} {getattr(c, 'name', c)} {layer} " + " ".join(f"{k}={v:.4f}" for k, v in w.items()))


def _ce_fwd(p):
    c = p.c
    return _L().nr_score_ce_fwd(p.cand.ptr, p.cand.ld, p.user.data_ptr(), p.label.data_ptr(), p.score.ptr, p.loss.ptr, p.lossvec.ptr, c.B, c.C, c.N,
                                ops._stream())


def _ce_bwd(p):
    c = p.c
    return _L().nr_score_ce_bwd(p.cand.ptr, p.cand.ld, p.user.data_ptr(), p.label.data_ptr(), p.score.ptr, _lib.ptr(p.gloss), _lib.ptr(p.gscore),
                                p.dcand.ptr, p.dcand.ld, p.duser.ptr, c.B, c.C, c.N, ops._stream())


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.ce_cases(), ids=lambda c: c.name)
def test_score_ce(c, layer):
    p, p2 = H.ce_problem(c, layer, DEV), H.ce_problem(c, layer, DEV)
    _ok(_ce_fwd(p), "nr_score_ce_fwd")
    w = H.ce_check_fwd(p)
    _ok(_ce_bwd(p), "nr_score_ce_bwd")
    w.update(H.ce_check_bwd(p))
    _ok(_ce_fwd(p2), "nr_score_ce_fwd")
    _ok(_ce_bwd(p2), "nr_score_ce_bwd")
    keys = ("score", "lossvec", "loss", "dcand", "duser")
    assert all(torch.equal(a, b) for a, b in zip(_flats(p, keys), _flats(p2, keys))), "two runs differ"
    _report("ce", c, layer, w)


@pytest.mark.parametrize("Cn", (0, 65))
def test_score_ce_refuses_C_outside_1_64(Cn):
    p = H.ce_problem(H.CeCase("r", 3, 5, 65, 3, "both", "ordinary"), "lattice", DEV)
    for fn in (_ce_fwd, _ce_bwd):
        p.c = p.c._replace(C=Cn)
        assert fn(p) == 1 and "(1..64)" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    for k in ("score", "lossvec", "loss", "dcand", "duser"):
        H._untouched("sentinel", k, getattr(p, k))


def _blend_fwd(p):
    c = p.c
    return _L().nr_pad_blend_fwd(p.x.ptr, _lib.ptr(p.mask), p.pad.ptr if p.pad is not None else 0, p.out.ptr, c.n, c.L, c.N, _lib.NR_BF16 if c.dt == "bf16" else _lib.NR_F32,
                                 ops._stream())


def _blend_bwd(p):
    c = p.c
    return _L().nr_pad_blend_bwd(p.dout.ptr, _lib.ptr(p.mask), p.dx.ptr, p.dpad.ptr if p.use_dpad else 0, c.n, c.L, c.N,
                                 _lib.NR_BF16 if c.dt == "bf16" else _lib.NR_F32, ops._stream())


class _Deterministic:
    """Deterministic mode with a scratch of this test's own, which must be zero filled again afterwards."""

    def __init__(self, on, elements=1 << 16):
        self.scratch = torch.zeros(elements, dtype=torch.int64, device=DEV) if on else None

    def __enter__(self):
        if self.scratch is not None:
            _lib.check(_L().nr_set_deterministic(self.scratch.data_ptr(), self.scratch.numel() * 8), "nr_set_deterministic")
        return self

    def __exit__(self, *exc):
        if self.scratch is not None:
            _lib.check(_L().nr_set_deterministic(None, 0), "nr_set_deterministic")
            torch.cuda.synchronize()
            if exc[0] is None:
                assert not bool(self.scratch.any()), "deterministic mode left its scratch non-zero"


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.blend_cases(), ids=lambda c: c.name)
def test_pad_blend(c, layer):
    p, p2 = H.blend_problem(c, layer, DEV), H.blend_problem(c, layer, DEV)
    _ok(_blend_fwd(p), "nr_pad_blend_fwd")
    w = H.blend_check_fwd(p)
    _ok(_blend_fwd(p2), "nr_pad_blend_fwd")
    assert torch.equal(*_flats(p, ("out",)), *_flats(p2, ("out",))), "two forward runs differ"
    with _Deterministic(c.det):
        _ok(_blend_bwd(p), "nr_pad_blend_bwd")
        _ok(_blend_bwd(p2), "nr_pad_blend_bwd")
    w.update(H.blend_check_dx(p))
    w.update(H.blend_check_dpad(p))
    keys = ("dx", "dpad") if c.det or layer == "lattice" else ("dx",)
    assert all(torch.equal(a, b) for a, b in zip(_flats(p, keys), _flats(p2, keys))), "two backward runs differ"
    _report("blend", c, layer, w)


def _eval_call(p):
    c = p.c
    return _L().nr_score_eval(p.news.ptr, p.news.ld, p.cand_ids.data_ptr(), p.imp_of.data_ptr(), p.user.ptr, p.user.ld, p.score.ptr, c.n_cand, c.N,
                              ops._stream())


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.eval_cases(), ids=lambda c: c.name)
def test_score_eval(c, layer):
    p, p2 = H.eval_problem(c, layer, DEV), H.eval_problem(c, layer, DEV)
    _ok(_eval_call(p), "nr_score_eval")
    w = H.eval_check(p)
    _ok(_eval_call(p2), "nr_score_eval")
    assert torch.equal(*_flats(p, ("score",)), *_flats(p2, ("score",))), "two runs differ"
    _report("eval", c, layer, w)


def _gather_call(p):
    c = p.c
    code = _lib.NR_BF16 if c.dt == "bf16" else _lib.NR_F32
    if c.fn == "embed":
        return _L().nr_embed_gather_fwd(p.table.ptr, p.table.ld, code, p.ids.data_ptr(), c.n_ids, c.stride, c.cols, p.out.ptr, p.out.ld, ops._stream())
    return _L().nr_gather_cast_fwd(p.table.ptr, p.table.ld, p.ids.data_ptr(), c.n_ids, c.cols, p.out.ptr, p.out.ld, code, ops._stream())


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.gather_cases(), ids=lambda c: c.name)
def test_gather(c, layer):
    p, p2 = H.gather_problem(c, layer, DEV), H.gather_problem(c, layer, DEV)
    _ok(_gather_call(p), "gather")
    H.gather_check(p)
    _ok(_gather_call(p2), "gather")
    assert torch.equal(*_flats(p, ("out",)), *_flats(p2, ("out",))), "two runs differ"


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.scatter_cases(), ids=lambda c: c.name)
def test_scatter_add(c, layer):
    """Exact on the lattice and inside the fp32 bound with and without deterministic mode, whose scratch stays zero: the
    stand-alone entry accumulates with fp32 atomics in either mode (include/nrhip.h, K1)."""
    p = H.scatter_problem(c, layer, DEV)
    with _Deterministic(c.det):
        _ok(_L().nr_embed_gather_bwd(p.dout.ptr, p.dout.ld, p.ids.data_ptr(), p.n, c.stride, c.cols, p.dtable.ptr, p.dtable.ld, ops._stream()),
            "nr_embed_gather_bwd")
    _report("scatter", c, layer, H.scatter_check(p))
    before = H._bits(p.dtable.flat).clone()
    _ok(_L().nr_embed_gather_bwd(p.dout.ptr, p.dout.ld, p.ids.data_ptr(), 0, c.stride, c.cols, p.dtable.ptr, p.dtable.ld, ops._stream()), "nr_embed_gather_bwd")
    assert torch.equal(before, H._bits(p.dtable.flat)), "n_ids == 0 wrote"


def _job(p):
    c = p.c
    return _lib.CastJob(src=p.src.ptr, dst=p.dst.ptr, rows=c.rows, cols=c.cols, ld_src=p.src.ld, ld_dst=p.dst.ld, transpose=c.transpose)


def _code(dt):
    return _lib.NR_BF16 if dt == "bf16" else _lib.NR_F32


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("c", H.pack_cases(), ids=lambda c: c.name)
def test_cast_pad(c, layer):
    p = H.pack_problem(c, c.dt, layer, DEV)
    _ok(_L().nr_cast_pad(p.src.ptr, c.rows, c.cols, p.src.ld, p.dst.ptr, p.dst.ld, _code(c.dt), c.transpose, ops._stream()), "nr_cast_pad")
    H.pack_check(p)


@pytest.mark.parametrize("layer", H.INPUT_LAYERS)
@pytest.mark.parametrize("name", sorted(H.batch_cases()))
def test_cast_pad_batch(name, layer):
    dt, jobs = H.batch_cases()[name]
    ps = [H.pack_problem(c, dt, layer, DEV, salt=k) for k, c in enumerate(jobs)]
    arr = (_lib.CastJob * len(ps))(*[_job(p) for p in ps])
    _ok(_L().nr_cast_pad_batch(arr, len(ps), _code(dt), ops._stream()), "nr_cast_pad_batch")
    for p in ps:
        H.pack_check(p)


def test_cast_pad_batch_refusals():
    ps = [H.pack_problem(H.PackCase("", "", 3, 5, 0, 0, k % 2), "bf16", "lattice", DEV, salt=k) for k in range(17)]
    arr = (_lib.CastJob * 17)(*[_job(p) for p in ps])
    assert _L().nr_cast_pad_batch(arr, 17, _lib.NR_BF16, ops._stream()) == 1 and "1..16 jobs" in _lib.last_error(), _lib.last_error()
    arr[1].ld_dst = 2          # transposed 3 x 5: the destination rows hold 3 elements
    assert _L().nr_cast_pad_batch(arr, 2, _lib.NR_BF16, ops._stream()) == 1 and "job 1 leading dimensions too small" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    for p in ps:
        H._untouched("sentinel", "dst", p.dst)


@pytest.mark.parametrize("prob", H.DROP_PS)
@pytest.mark.parametrize("count", H.DROP_COUNTS)
def test_dropout_mask(count, prob):
    for seed in H.DROP_SEEDS:
        buf = H.glue_buf(1, count, count, torch.float32, DEV)
        _ok(_L().nr_dropout_mask(buf.ptr, count, prob, seed, ops._stream()), "nr_dropout_mask")
        H.drop_check(buf, count, prob, seed)
