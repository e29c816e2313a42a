"""Shared helpers for the GPU parity tests (CPU side: fixtures + the oracle as checker)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import nr_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(tag):
    z = np.load(os.path.join(GOLDEN, tag + ".npz"))
    cfg = SimpleNamespace(**json.loads(str(z["cfg_json"])))
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    return z, cfg, sd


def table_key(tag):
    return "news_encoder.embedding_matrix.weight" if tag.startswith("nrms") else "news_encoder.title_embeddings.weight"


def build_model(tag, compute_dtype="fp32", train=False, device="cuda"):
    """Our drop-in Model loaded with the reference's state_dict of a golden case."""
    from newsrecommendation_amd.model import NAML, NRMS
    z, cfg, sd = load_case(tag)
    args = SimpleNamespace(**vars(cfg), compute_dtype=compute_dtype)
    if tag.startswith("naml"):
        # The [V, T*D] title-embedding table stays frozen on this path (src/demo.sh:12):
        # every other gradient is independent of that flag, so the golden case is still fully checked.
        args.freeze_embedding = True
    table = sd[table_key(tag)].numpy()
    if tag.startswith("nrms"):
        m = NRMS.Model(args, table)
    else:
        n_cat = sd["news_encoder.category_emb.weight"].shape[0] - 1 if "news_encoder.category_emb.weight" in sd else 0
        n_sub = sd["news_encoder.subcategory_emb.weight"].shape[0] - 1 if "news_encoder.subcategory_emb.weight" in sd else 0
        m = NAML.Model(args, table, n_cat, n_sub)
    missing = m.load_state_dict(sd, strict=True)
    m = m.to(device)
    m.train(train)
    return m, z, cfg, sd


def batch_of(z, device="cuda"):
    return tuple(torch.from_numpy(z[k]).to(device) for k in ("hist", "mask", "cand", "label"))


def oracle_run(tag, z, cfg, sd, keep=None):
    """Oracle forward + backward on CPU; returns (loss, score, grads dict)."""
    fwd = O.nrms_forward if tag.startswith("nrms") else O.naml_forward
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    hist, mask, cand, label = (torch.from_numpy(z[k]) for k in ("hist", "mask", "cand", "label"))
    loss, score = fwd(hist, mask, cand, label, sdo, cfg, keep=keep)
    loss.backward()
    return loss.detach(), score.detach(), {k: v.grad for k, v in sdo.items() if v.grad is not None}


def max_err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max()) if a.numel() else 0.0


def assert_close(a, b, atol, rtol=0.0, name=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if a.numel() == 0:
        return
    tol = atol + rtol * float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= tol, f"{name}: max|diff|={err:.3e} > {tol:.3e} (ref max {float(b.abs().max()):.3e})"


def metric_row_as_device(labels, s):
    """[AUC, MRR, nDCG@5, nDCG@10] of one impression, ranked as the device kernel (ops.eval_metrics) ranks it, on the scores `s`
    it produced.  Rank metrics are discontinuous in the scores (near-ties), so both implementations are compared on the SAME
    scores.  Duplicate candidates of an impression have EQUAL scores; numpy's default argsort (src/metrics.py:6,20) leaves their
    order unspecified, the device kernel uses the stable order reversed -- restated here.  Without ties the row must be exactly
    the reference's functions (checked).  Returns (row, tie_free)."""
    order = np.argsort(s, kind="stable")[::-1]
    yt = labels[order]
    dcg = lambda k: np.sum((2 ** yt[:k] - 1) / np.log2(np.arange(len(yt[:k])) + 2))
    row = [O.auc_score(labels, s), np.sum(yt / (np.arange(len(yt)) + 1)) / yt.sum(), dcg(5) / O.dcg_score(labels, labels, 5),
           dcg(10) / O.dcg_score(labels, labels, 10)]
    tie_free = len(np.unique(s)) == len(s)
    if tie_free:
        assert np.allclose(row, [O.auc_score(labels, s), O.mrr_score(labels, s), O.ndcg_score(labels, s, 5),
                                 O.ndcg_score(labels, s, 10)], atol=1e-12)
    return row, tie_free


# ------------------------------------------------------------------------------------------ key-mask patterns
MASKS = ("ones", "front", "back", "middle", "holes", "single", "none_valid")


def masks(n, L, g):
    """[n, L] 0/1 key masks, pattern i % 7 of MASKS for sequence i; returns (mask, pattern index per sequence)."""
    pos = torch.arange(L)[None, :]
    kind = torch.arange(n) % len(MASKS)
    ln = torch.randint(1, L + 1, (n,), generator=g)
    start = (torch.rand(n, generator=g) * (L - ln + 1)).long().clamp(max=L - ln)
    run = (pos >= start[:, None]) & (pos < (start + ln)[:, None])
    front = pos >= (L - ln)[:, None]
    back = pos < ln[:, None]
    holes = (torch.rand(n, L, generator=g) < 0.6) & front
    holes[:, -1] = True
    single = pos == torch.randint(0, L, (n,), generator=g)[:, None]
    m = torch.ones(n, L, dtype=torch.bool)
    for k, pat in enumerate((m, front, back, run, holes, single, torch.zeros(n, L, dtype=torch.bool))):
        m = torch.where((kind == k)[:, None], pat, m)
    return m.float(), kind


# ------------------------------------------------------------------------------------------ attention-core sweep
# Shared by tests/test_attention_sweep_host.py (CPU: stand-in kernel, tolerances, mutation check) and
# tests/test_gpu_attention_sweep.py (the HIP kernels), so the host proof covers exactly the cases the GPU runs.
# Every tensor of a case is seen as [n, heads, L, d].
import math
import zlib
from collections import namedtuple

AttnCase = namedtuple("AttnCase", "dtype heads d L n align route regime p_out")
LOG2E = 1.4426950408889634

# Project bounds: tests/test_gpu_properties.py (bf16 outputs 2e-2, bf16 gradients 3e-2), fp32 1e-4.
ATTN_PROJECT_TOL = {"bf16": {"y": 2e-2, "dq": 3e-2, "dk": 3e-2, "dv": 3e-2}, "f32": {"y": 1e-4, "dq": 1e-4, "dk": 1e-4, "dv": 1e-4}}
# min(project bound, 3 x the stand-in's worst slice-relative error over attn_cases()): computed and pinned by
# tests/test_attention_sweep_host.py (its docstring holds the stand-in's own figures).
ATTN_TOL = {"bf16": {"y": 2e-2, "dq": 3e-2, "dk": 3e-2, "dv": 3e-2}, "f32": {"y": 1.4e-5, "dq": 9.4e-6, "dk": 1.1e-5, "dv": 8.8e-6}}
# Absolute allowance, in units of max|dy| max|V| max(|Q|, |K|), where a gradient is analytically zero (dQ / dK with at most one
# valid key, dK / dV rows of masked keys): 3 x the stand-in's worst |error| there; same test.
ATTN_ABS_ZERO = {"bf16": 5.0e-8, "f32": 5.5e-8}

# kernel route -> (forward label prefix, backward label prefix) of the library's profiler
ATTN_ROUTE_LABELS = {
    "title30": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"), "full": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"),
    "nonfull": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"), "pt4": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"),
    "c64": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"), "g64": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"),
    "gen_bf16": ("attn_mfma_fwd[bf16,", "attn_mfma_bwd[bf16,"), "gen_f32": ("attn_mfma_fwd[f32,", "attn_mfma_bwd[f32,"),
    "valu_bf16": ("attn_fwd[bf16,", "attn_bwd[bf16,"), "valu_f32": ("attn_fwd[f32,", "attn_bwd[f32,"),
}


def attn_route(dtype, heads, d, L, aligned):
    """The kernel family nr_launch_attn picks (csrc/nr_attn.hip, nr_launch_attn_mfma and b16::launch in csrc/nr_attn_mfma.hip),
    restated from the dispatch; None = the library refuses the shape.
      title30 / full / nonfull / pt4: bf16 panel kernels, L <= 32 (constants 30/20/20; FULL generic; predicated PT = 3; PT = 4)
      c64 / g64: bf16 64-row kernels (constants 50/20/20; generic);  gen_*: one wave per (sequence, head), any d <= 32
      valu_*: the LDS/VALU kernels of csrc/nr_attn.hip."""
    if not (1 <= L <= 64 and heads >= 1 and d >= 1):
        return None
    if d <= 32:
        fast = dtype == "bf16" and d % 4 == 0 and aligned
        if fast and L > 32:
            return "c64" if (L, d, heads) == (50, 20, 20) else "g64"
        if fast:
            p3 = L * d <= 768
            full = heads % 4 == 0 and L * d >= 64 and 3 * 32 * 4 * d <= 2 * 4 * 1024
            assert not (full and not p3)            # FULL + PT = 4 cannot be reached: d <= 21 and d % 4 == 0 give L * d <= 640
            if full:
                return "title30" if (L, d, heads) == (30, 20, 20) else "full"
            return "nonfull" if p3 else "pt4"
        if L <= 32:
            return "gen_" + dtype
    return "valu_" + dtype if d in (4, 8, 16, 20, 32) else None


def attn_case_id(c):
    return f"{c.dtype}-{c.align}-h{c.heads}d{c.d}-L{c.L}-n{c.n}-{c.regime}-p{c.p_out}"


def attn_cases():
    """The sweep's case list: (heads, d_head) x L reaching every route of the dispatch, then dropout on one case per route
    family, the score regimes, a masked key carrying the row maximum, and the grid-stride walks."""
    C = []

    def add(route, dtype, hd, Ls, align="aligned", n=67, regime="ordinary", p_out=0.0):
        for heads, d in hd:
            for L in Ls:
                C.append(AttnCase(dtype, heads, d, L, n, align, route, regime, p_out))

    add("title30", "bf16", [(20, 20)], [30])
    add("nonfull", "bf16", [(20, 20)], [1, 2])                        # L * d < 64: predicated kernel although heads % 4 == 0
    add("full", "bf16", [(20, 20)], [15, 16, 17, 31, 32])
    add("full", "bf16", [(8, 16)], [12, 32])
    add("nonfull", "bf16", [(3, 8), (6, 8)], [5, 20])                 # hcount < 4 in the last head group
    add("nonfull", "bf16", [(4, 4)], [8])                             # L * d < 64
    add("pt4", "bf16", [(4, 32), (5, 32)], [25, 30, 32])
    add("c64", "bf16", [(20, 20)], [50])
    add("g64", "bf16", [(20, 20)], [33, 48, 63, 64])
    add("g64", "bf16", [(8, 16), (3, 32)], [33, 64])
    add("gen_bf16", "bf16", [(4, 6), (4, 10)], [7, 32])               # d % 4 != 0
    add("gen_bf16", "bf16", [(20, 20), (4, 8)], [30], align="misaligned")
    add("valu_bf16", "bf16", [(20, 20), (4, 8)], [50], align="misaligned")
    add("gen_f32", "f32", [(3, 4), (3, 7), (3, 12), (3, 20), (3, 32)], [1, 17, 32])
    add("valu_f32", "f32", [(9, 4), (9, 8), (9, 16), (9, 20), (9, 32)], [33, 50, 64])     # 9 heads: HG = 7, 5, 4 (3 at d = 32, L = 64) < heads
    # output dropout: one case per route family
    for route, dtype, hd, L, align in (("title30", "bf16", (20, 20), 30, "aligned"), ("full", "bf16", (8, 16), 12, "aligned"),
                                       ("nonfull", "bf16", (3, 8), 5, "aligned"), ("nonfull", "bf16", (4, 4), 8, "aligned"),
                                       ("pt4", "bf16", (5, 32), 30, "aligned"), ("c64", "bf16", (20, 20), 50, "aligned"),
                                       ("g64", "bf16", (8, 16), 33, "aligned"), ("gen_bf16", "bf16", (4, 6), 7, "aligned"),
                                       ("gen_bf16", "bf16", (4, 8), 30, "misaligned"), ("valu_bf16", "bf16", (4, 8), 50, "misaligned"),
                                       ("gen_f32", "f32", (3, 20), 17, "aligned"), ("valu_f32", "f32", (9, 20), 50, "aligned")):
        add(route, dtype, [hd], [L], align=align, p_out=0.2)
    # score regimes (the ordinary one is the base case above) and a masked key that carries the row maximum
    for regime in ("negative", "positive", "masked_max"):
        add("title30", "bf16", [(20, 20)], [30], regime=regime)
        add("g64", "bf16", [(8, 16)], [33], regime=regime)
        add("gen_f32", "f32", [(3, 20)], [17], regime=regime)
        add("valu_f32", "f32", [(9, 20)], [50], regime=regime)
    # grid-stride walks: more sequences than the block caps (4 096 panel workgroups; 1 024 / 4 096 generic backward / forward)
    add("nonfull", "bf16", [(4, 8)], [5], n=4101)
    add("gen_f32", "f32", [(4, 8)], [5], n=4101)
    add("gen_f32", "f32", [(12, 8)], [5], n=12303)
    return C


def attn_mask_modes(c):
    if c.regime == "masked_max":
        return ("mmax",)
    return ("none", "rr") + (("halves",) if c.L > 32 else ())


def _bf16r(t):
    return t.to(torch.bfloat16).float()


def attn_inputs(c):
    """CPU inputs of a case, bf16-representable fp32: q, k, v, dy [n, heads, L, d] and {mask mode: [n, L] mask or None}.
    Regimes (scores s = q.k / sqrt(d)): ordinary |s| <~ 3; negative s in [-22, -18] (the 1e-8 is a visible share of the
    denominator); positive s in [38, 45]; masked_max: key L // 2 is masked and ~30 above every valid key."""
    g = torch.Generator().manual_seed(zlib.crc32(attn_case_id(c).encode()))
    n, h, L, d = c.n, c.heads, c.L, c.d
    shape = (n, h, L, d)
    u = lambda hw: (torch.rand(shape, generator=g) * 2 - 1) * hw
    if c.regime == "ordinary":
        q, k = torch.randn(shape, generator=g) * 0.7, torch.randn(shape, generator=g) * 0.7
    elif c.regime in ("negative", "positive"):
        # the first half of the head dims carries the score (q ~ +a, k ~ -/+ a, small deviations); of the rest, one half has
        # q = 0 and a free k, the other k = 0 and a free q.  With near-constant Q and K alone, dQ = dS.K and dK = dS^T.Q are
        # cancelling sums (sum_j dS_ij ~ 0) in which any bf16 kernel loses its digits; the free parts keep both well conditioned
        centre, dev = (20.0, 1.2) if c.regime == "negative" else (41.5, 2.5)
        hd = d // 2
        fk = hd + (d - hd) // 2
        a = math.sqrt(centre * math.sqrt(d) / hd)
        hw = dev * math.sqrt(d) / (hd * 2 * a)
        q, k = a + u(hw), a + u(hw)
        if c.regime == "negative":
            k = -k
        q[..., hd:fk] = 0
        k[..., hd:fk] = torch.randn(n, h, L, fk - hd, generator=g) * 2
        q[..., fk:] = torch.randn(n, h, L, d - fk, generator=g) * 2
        k[..., fk:] = 0
    else:
        q, k = 1 + u(0.3), torch.randn(shape, generator=g) * 0.5
        k[:, :, L // 2, :] = 30.0 / math.sqrt(d)
    v, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    out = dict(q=_bf16r(q), k=_bf16r(k), v=_bf16r(v), dy=_bf16r(dy), masks={})
    for mode in attn_mask_modes(c):
        if mode == "none":
            m = None
        elif mode == "rr":
            m = masks(n, L, g)[0]
        elif mode == "halves":                              # 32 < L <= 64: valid keys only >= 32 (even sequences) / only < 32 (odd)
            pos, even = torch.arange(L)[None, :], (torch.arange(n) % 2 == 0)[:, None]
            m = (torch.rand(n, L, generator=g) < 0.7) & torch.where(even, pos >= 32, pos < 32)
            m[:, L - 1] |= even[:, 0]
            m[:, 0] |= ~even[:, 0]
            m = m.float()
        else:                                               # masked_max
            m = torch.rand(n, L, generator=g) < 0.7
            m[:, (L // 2 + 1) % L] = True
            m[:, L // 2] = False
            m = m.float()
        out["masks"][mode] = m
    return out


def attn_ref64(q, k, v, mask, dy, keep=None, p=0.0):
    """The fp64 reference: O.sdpa (+ O.apply_dropout with the given keep mask) and its autograd gradient.
    Returns dict y, dq, dk, dv, fp64 [n, heads, L, d]."""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    hm = None if mask is None else mask.double()[:, None, :].expand(-1, q.shape[1], -1)
    y = O.apply_dropout(O.sdpa(q, k, v, hm), None if keep is None else keep.double(), p)
    y.backward(dy.double())
    return dict(y=y.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def attn_math(q, k, v, mask, dy, keep=None, p=0.0, dt=torch.float64, bf16=False, eps_unscaled=False, dk_skip_last_query=False):
    """Forward and analytic backward in the stable form the kernels evaluate (row maximum over ALL keys factored out,
    1e-8 * exp(-m) in the denominator), in precision `dt`.
      dt = fp64: the reference's formula (and, with a flag set, a mutant of it);
      dt = fp32: the CPU stand-in kernel; exp as exp2(x * log2 e) like v_exp_f32 behind __expf.  With bf16=True the values
        the kernels feed to a bf16 MFMA are rounded to bf16: the normalised weights P (P.V and P^T.dO), dO after the
        output dropout, dS including the 1/sqrt(d) (dS.K and dS^T.Q) -- csrc/nr_attn_mfma.hip: mm_xt / mm_xt_T /
        acc_to_img_t convert their accumulator operand, stage_head / panel_put store the dropped-out dy as bf16 -- and
        the outputs."""
    rb = (lambda t: t.to(torch.bfloat16).to(dt)) if bf16 else (lambda t: t)
    q, k, v, dy = (t.to(dt) for t in (q, k, v, dy))
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(-1, keepdim=True)
    ex = (lambda t: torch.exp2(t * LOG2E)) if dt == torch.float32 else torch.exp
    e = ex(s - m)
    if mask is not None:
        e = e * mask.to(dt)[:, None, None, :]
    inv = 1.0 / (e.sum(-1, keepdim=True) + (1e-8 if eps_unscaled else 1e-8 * ex(-m)))
    P = e * inv
    Pb = rb(P)
    y, G = Pb @ v, dy
    if keep is not None:
        drop = keep.to(dt) * (1.0 / (1.0 - p))
        y, G = y * drop, rb(dy * drop)
    dP = G @ v.transpose(-1, -2)
    rd = (e * dP).sum(-1, keepdim=True) * inv
    dSb = rb(P * (dP - rd) * scale)
    dq = dSb @ k
    dk = dSb[..., :-1, :].transpose(-1, -2) @ q[..., :-1, :] if dk_skip_last_query else dSb.transpose(-1, -2) @ q
    dv = Pb.transpose(-1, -2) @ G
    return dict(y=rb(y), dq=rb(dq), dk=rb(dk), dv=rb(dv))


def attn_standin(c, q, k, v, mask, dy, keep=None, p=0.0):
    return attn_math(q, k, v, mask, dy, keep, p, dt=torch.float32, bf16=c.dtype == "bf16")


ATTN_MUTANTS = ("last_key_ignored", "mask_rotated", "keep_shifted", "v_heads_swapped", "eps_unscaled", "dk_last_query_missing")


def attn_mutant(name, q, k, v, mask, dy, keep=None, p=0.0):
    """A subtly wrong fp64 attention (what a kernel bug of that kind would compute); None where the mutation does not apply."""
    n, h, L, d = q.shape
    kw = {}
    if name == "last_key_ignored":
        mask = (torch.ones(n, L) if mask is None else mask.clone())
        mask[:, -1] = 0
    elif name == "mask_rotated":                           # one sequence's mask rotated by one position
        if mask is None:
            return None
        s = min(1, n - 1)
        mask = mask.clone()
        mask[s] = torch.roll(mask[s], 1)
    elif name == "keep_shifted":                           # the keep mask shifted by one element of y[n, L, N]
        if keep is None:
            return None
        keep = torch.roll(keep.permute(0, 2, 1, 3).reshape(-1), 1).view(n, L, h, d).permute(0, 2, 1, 3)
    elif name == "v_heads_swapped":                        # V of two neighbouring heads swapped in one sequence
        if h < 2:
            return None
        v = v.clone()
        v[n - 1, [0, 1]] = v[n - 1, [1, 0]]
    elif name == "eps_unscaled":
        kw["eps_unscaled"] = True
    elif name == "dk_last_query_missing":
        kw["dk_skip_last_query"] = True
    else:
        raise ValueError(name)
    return attn_math(q, k, v, mask, dy, keep, p, **kw)


def attn_zero_places(mask, n, L):
    """Where a gradient is analytically zero, as bool [n, 1, L, 1] per quantity: dQ and dK of sequences with at most one valid
    key (L = 1, a single click, all masked: the softmax row is constant up to the 1e-8), dK and dV rows of masked keys."""
    valid = torch.ones(n, L, dtype=torch.bool) if mask is None else mask > 0
    few = (valid.sum(1) <= 1)[:, None].expand(n, L)
    sh = lambda t: t[:, None, :, None]
    return dict(y=None, dq=sh(few), dk=sh(few | ~valid), dv=sh(~valid))


def attn_grad_unit(q, k, v, dy):
    """max|dy| max|V| max(|Q|, |K|): the unit of ATTN_ABS_ZERO."""
    return float(dy.abs().max()) * float(v.abs().max()) * max(float(q.abs().max()), float(k.abs().max()))


def slice_rel_err(got, ref, zero=None, allow=0.0):
    """Worst over the (sequence, head) slices of [n, heads, L, d] tensors of
         max|got - ref| / max(max|ref| of the slice, 1e-2 * max|ref| of the tensor),
    so that a wrong head or sequence cannot hide behind a large neighbour.  Elements where `zero` (broadcastable bool) is set
    get the absolute allowance `allow` first.  inf for non-finite values, or a non-zero error where the reference is all zero."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    diff = (got - ref).abs()
    if zero is not None and allow > 0:
        diff = (diff - allow * zero.double()).clamp_min(0)
    num = diff.amax((2, 3))
    den = torch.maximum(ref.abs().amax((2, 3)), 1e-2 * ref.abs().max())
    err = torch.where(num > 0, num / den, torch.zeros_like(num))
    return float(err.max()) if err.numel() else 0.0


def attn_errors(c, got, ref, mask, unit, abs_zero):
    """{quantity: slice-relative error} of a kernel's (or stand-in's / mutant's) y, dq, dk, dv against the reference."""
    n, L = ref["y"].shape[0], ref["y"].shape[2]
    zp = attn_zero_places(mask, n, L)
    return {name: slice_rel_err(got[name], ref[name], zp[name], abs_zero * unit) for name in ("y", "dq", "dk", "dv")}
