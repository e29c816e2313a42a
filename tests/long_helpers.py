"""Shared by tests/test_long_history_host.py (CPU: stand-in kernel, tolerances, mutants) and tests/test_gpu_long_history.py
(the HIP kernels): the case list of the attention core at 64 < L <= 128, its masks, its extra mutants and the pinned tolerances.
Built on helpers.py (case tuple, inputs, fp64 reference, stand-in, comparator); nothing there is changed."""
import torch

import helpers as H

LONG_LS = (65, 95, 96, 97, 100, 127, 128)        # 65: one row in the third block; 96 / 97: 3 -> 4 blocks; 128: a full tile
LONG_HD = ((20, 20), (4, 8), (3, 32), (8, 16))   # reference shape; small; fewer heads than waves + widest head; generic

# route -> (forward label prefix, backward label prefix)
LONG_ROUTE_LABELS = {
    "long_bf16": ("attn_long_fwd[bf16,", "attn_long_bwd[bf16,"),
    "valu_bf16": ("attn_fwd[bf16,", "attn_bwd[bf16,"),
    "valu_f32": ("attn_fwd[f32,", "attn_bwd[f32,"),
}
ALL_ATTN_LABELS = {l for pair in list(LONG_ROUTE_LABELS.values()) + list(H.ATTN_ROUTE_LABELS.values()) for l in pair}


def long_route(dtype, heads, d, L, aligned):
    """The kernel family nr_launch_attn picks at 64 < L <= 128 (csrc/nr_attn.hip), restated; None = refused."""
    if not (64 < L <= 128 and heads >= 1 and d >= 1):
        return None
    if dtype == "bf16" and d % 4 == 0 and d <= 32 and aligned:
        return "long_bf16"
    return "valu_" + dtype if d in (4, 8, 16, 20, 32) else None


def long_cases():
    C = []

    def add(route, dtype, hd, Ls, align="aligned", n=67, regime="ordinary", p_out=0.0):
        for heads, d in hd:
            for L in Ls:
                C.append(H.AttnCase(dtype, heads, d, L, n, align, route, regime, p_out))

    add("long_bf16", "bf16", LONG_HD, LONG_LS)
    add("valu_bf16", "bf16", [(20, 20), (4, 8)], [65, 100, 128], align="misaligned")
    add("valu_f32", "f32", [(3, 4), (3, 20), (3, 32)], [65, 100, 128])
    add("long_bf16", "bf16", [(20, 20)], [100], p_out=0.2)
    add("valu_f32", "f32", [(3, 20)], [100], p_out=0.2)
    for regime in ("negative", "positive", "masked_max"):
        add("long_bf16", "bf16", [(20, 20)], [100], regime=regime)
        add("valu_f32", "f32", [(3, 20)], [100], regime=regime)
    return C


def block_mask(n, L, b, g):
    """Valid keys only in row block b (keys [32 b, 32 b + 32) below L), ~70 % of them and at least the block's first."""
    pos = torch.arange(L)[None, :]
    m = (torch.rand(n, L, generator=g) < 0.7) & (pos >= 32 * b) & (pos < 32 * b + 32)
    m[:, 32 * b] = True
    return m.float()


def has_block_masks(c):
    """The cases that also run 'valid keys only in row block b': one 3-block and one 4-block shape per route family."""
    return c.regime == "ordinary" and c.p_out == 0.0 and ((c.heads, c.d) in ((20, 20), (3, 20)) and c.L in (96, 100))


def long_inputs(c):
    """helpers.attn_inputs of the case, with the mask modes of this sweep: none, the seven patterns round-robin, and (on the
    cases of has_block_masks) valid keys only in row block b for every block of the shape."""
    inp = H.attn_inputs(c)
    keep = ("mmax",) if c.regime == "masked_max" else ("none", "rr")
    inp["masks"] = {k: inp["masks"][k] for k in keep}
    if has_block_masks(c):
        g = torch.Generator().manual_seed(1000 + c.L)
        for b in range((c.L + 31) // 32):
            inp["masks"][f"blk{b}"] = block_mask(c.n, c.L, b, g)
    return inp


# ---- mutants of the fp64 formula that only exist with more than two row blocks
LONG_MUTANTS = ("last_block_ignored", "pv_blocks_2_3_swapped", "dk_queries_from_96_missing")


def long_mutant(name, q, k, v, mask, dy, keep=None, p=0.0):
    """None where the mutation does not apply (fewer than four row blocks for the last two)."""
    n, h, L, d = q.shape
    RB = (L + 31) // 32
    if name == "last_block_ignored":                      # the last 32-row key block never read
        mask = torch.ones(n, L) if mask is None else mask.clone()
        mask[:, 32 * (RB - 1):] = 0
        return H.attn_math(q, k, v, mask, dy, keep, p)
    if L <= 96:
        return None
    out = H.attn_math(q, k, v, mask, dy, keep, p)
    if name == "pv_blocks_2_3_swapped":                   # P.V takes V of key block 3 for the weights of block 2 and back
        w = L - 96                                         # rows both blocks have
        vs = v.clone()
        vs[:, :, 64:64 + w], vs[:, :, 96:96 + w] = v[:, :, 96:96 + w], v[:, :, 64:64 + w]
        out["y"] = H.attn_math(q, k, vs, mask, dy, keep, p)["y"]
        return out
    if name == "dk_queries_from_96_missing":              # dK = dS^T Q summed over the first three query blocks only
        short = H.attn_math(q[:, :, :96], k, v, mask, dy[:, :, :96], None if keep is None else keep[:, :, :96], p)
        # (rows of the softmax are independent: dropping queries drops their terms of the sum over queries, nothing else)
        out["dk"] = short["dk"]
        return out
    raise ValueError(name)


# min(project bound, 3 x the stand-in's worst slice-relative error over long_cases()): computed and pinned by
# tests/test_long_history_host.py, whose docstring holds the stand-in's own figures.
LONG_TOL = {"bf16": {"y": 2e-2, "dq": 2.1e-2, "dk": 2.2e-2, "dv": 2.05e-2}, "f32": {"y": 1.0e-5, "dq": 6.3e-6, "dk": 8.4e-6, "dv": 7.9e-6}}
# absolute allowance where a gradient is analytically zero, as helpers.ATTN_ABS_ZERO; same test
LONG_ABS_ZERO = {"bf16": 8.0e-8, "f32": 7.0e-8}
