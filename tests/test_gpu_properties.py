"""GPU: size-independent properties at BASELINE.json's full per-GPU sizes (B=512 -> 28 160 titles, 844 800 token
rows), where the CPU oracle would take minutes, plus the reference's documented edge cases.

  * GEMM building blocks: linearity in A, agreement of the bf16 MFMA path with an fp64 torch product on sampled
    rows/columns, weight-gradient GEMM == sum over row blocks (split invariance) and db == column sums.
  * attention: all-ones key mask == no mask; all-zero mask -> exactly 0 output; permuting the tokens
    of a title permutes its outputs (no positional term).
  * pooling: permutation invariance over tokens; all-zero mask -> exactly 0.
  * embedding: gather -> scatter-add round trip counts ids, padding id 0 receives nothing.
"""
import pytest
import torch

from newsrecommendation_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
M_FULL = 512 * 55 * 30


def _bf(x):
    return x.to(torch.bfloat16)


def test_gemm_nt_full_size_sampled_against_fp64_and_linearity():
    g = torch.Generator(device=DEV).manual_seed(0)
    M, N, K = M_FULL, 1200, 304
    a = _bf(torch.randn(M, K, device=DEV, generator=g) * 0.5)
    wfull = torch.zeros(N, 320, device=DEV, dtype=torch.bfloat16)
    wfull[:, :K] = _bf(torch.randn(N, K, device=DEV, generator=g) * 0.1)
    w = wfull[:, :K]
    c = ops.gemm_nt(a, w)
    rows = torch.randint(0, M, (2048,), device=DEV, generator=g)
    ref = a[rows].double() @ w.double().t()
    err = (c[rows].double() - ref).abs().max().item()
    assert err <= 0.03, err                                   # bf16 output rounding of values up to ~5
    # last rows / last columns (tile tails) exactly as well
    assert (c[-5:].double() - a[-5:].double() @ w.double().t()).abs().max().item() <= 0.03
    # linearity: (2a) W^T == 2 (a W^T) exactly (power-of-two scaling commutes with every rounding)
    c2 = ops.gemm_nt(_bf(a.float() * 2), w)
    assert torch.equal(c2.float(), c.float() * 2)


@pytest.mark.parametrize("N,K", [(200, 400), (1200, 304), (400, 960)])     # dW1, dW_qkv (256-row n-tile), conv dW (3 k-tiles)
def test_gemm_tn_full_size_split_invariance_and_bias_grad(N, K):
    g = torch.Generator(device=DEV).manual_seed(1)
    M = M_FULL
    dc = _bf(torch.randn(M, N, device=DEV, generator=g) * 0.05)
    a = _bf(torch.randn(M, K, device=DEV, generator=g) * 0.5)
    dw, db = ops.gemm_tn(dc, a)
    half = M // 2
    dw1, db1 = ops.gemm_tn(dc[:half], a[:half])
    dw2, db2 = ops.gemm_tn(dc[half:], a[half:])
    scale = dw.abs().max().item()
    assert (dw - (dw1 + dw2)).abs().max().item() <= 2e-5 * scale + 1e-3      # fp32 accumulation order only
    assert (db - (db1 + db2)).abs().max().item() <= 1e-3 * db.abs().max().item() + 1e-3
    ref_db = dc.double().sum(0)
    assert (db.double() - ref_db).abs().max().item() <= 1e-3 * ref_db.abs().max().item() + 1e-2
    cols = torch.cat([torch.arange(0, K, 37, device=DEV), torch.tensor([K - 1], device=DEV)])
    ref = dc.double().t() @ a[:, cols].double()
    assert (dw[:, cols].double() - ref).abs().max().item() <= 1e-3 * ref.abs().max().item() + 1e-2


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_attention_mask_and_permutation_properties(dt):
    code = ops.dtype_code(dt)
    td = ops.torch_dtype(code)
    g = torch.Generator(device=DEV).manual_seed(2)
    n, L, D, heads, dh = (2048 if dt == "bf16" else 256), 30, 304 if dt == "bf16" else 300, 20, 20
    N = heads * dh
    x = (torch.randn(n, L, D, device=DEV, generator=g) * 0.4).to(td)
    ws = [torch.randn(N, D, device=DEV, generator=g) * 0.05 for _ in range(3)]
    bs = [torch.randn(N, device=DEV, generator=g) * 0.05 for _ in range(3)]
    args = (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])
    y0 = ops.mhsa(x, *args, heads=heads, code=code)
    ones = torch.ones(n, L, device=DEV)
    y1 = ops.mhsa(x, *args, heads=heads, code=code, mask=ones)
    assert torch.equal(y0, y1)                                              # all-ones mask == no mask
    zeros = torch.zeros(n, L, device=DEV)
    yz = ops.mhsa(x, *args, heads=heads, code=code, mask=zeros)
    assert float(yz.float().abs().max()) == 0.0                             # fully masked -> exactly 0, not NaN
    perm = torch.randperm(L, device=DEV, generator=g)
    yp = ops.mhsa(x[:, perm].contiguous(), *args, heads=heads, code=code)
    tol = 2e-5 if dt == "fp32" else 2e-2
    assert (yp.float() - y0[:, perm].float()).abs().max().item() <= tol     # token permutation equivariance
    # additive pooling: permutation invariance and the all-zero mask
    q = 200
    w1, b1 = torch.randn(q, N, device=DEV, generator=g) * 0.05, torch.randn(q, device=DEV, generator=g) * 0.05
    w2, b2 = torch.randn(1, q, device=DEV, generator=g) * 0.1, torch.randn(1, device=DEV, generator=g) * 0.1
    p0 = ops.additive_pool(y0, w1, b1, w2, b2, code)
    pp = ops.additive_pool(y0[:, perm].contiguous(), w1, b1, w2, b2, code)
    assert (p0 - pp).abs().max().item() <= (1e-5 if dt == "fp32" else 5e-3)
    assert float(ops.additive_pool(y0, w1, b1, w2, b2, code, mask=zeros).abs().max()) == 0.0


def test_full_batch_forward_bf16_tracks_fp32_and_is_deterministic():
    """B=512 NRMS forward (eval): bf16 path vs the exact-fp32 path of the same library, twice for bit-reproducibility."""
    import bench
    from newsrecommendation_amd.model import NRMS
    res = {}
    for dt in ("fp32", "bf16"):
        args = bench.make_args(dt)
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(1)
        table = torch.randn(3000, 300, generator=g) * 0.4
        table[0] = 0
        m = NRMS.Model(args, table.numpy()).to(DEV).eval()
        hist, mask, cand, label = bench.synth_batches(args, 512, 3000, 1, 5, DEV)[0]
        with torch.no_grad():
            l1, s1 = m(hist, mask, cand, label)
            l2, s2 = m(hist, mask, cand, label)
        assert torch.equal(s1, s2) and torch.equal(l1, l2)                 # forward is deterministic
        res[dt] = (float(l1), s1.float().cpu())
    assert abs(res["fp32"][0] - res["bf16"][0]) <= 2e-2
    assert (res["fp32"][1] - res["bf16"][1]).abs().max().item() <= 6e-2
    assert torch.isfinite(res["bf16"][1]).all()


def test_embedding_gather_scatter_roundtrip_and_padding_row():
    g = torch.Generator(device=DEV).manual_seed(3)
    V, D, n = 30000, 300, 844800 // 4
    table = torch.randn(V, D, device=DEV, generator=g)
    ids = torch.randint(0, V, (n,), device=DEV, generator=g, dtype=torch.int32)
    out = ops.embed_gather(table, ids)
    assert torch.equal(out, table[ids.long()])                              # row gather is a bit-exact copy
    from newsrecommendation_amd import _lib
    ones = torch.ones(n, 4, device=DEV)
    acc = torch.zeros(V, 4, device=DEV)
    _lib.check(_lib.lib().nr_embed_gather_bwd(ones.data_ptr(), 4, ids.data_ptr(), n, 1, 4, acc.data_ptr(), 4,
                                              torch.cuda.current_stream().cuda_stream), "nr_embed_gather_bwd")
    counts = torch.bincount(ids.long(), minlength=V).float()
    counts[0] = 0                                                           # padding_idx row receives no gradient
    assert torch.equal(acc[:, 0], counts) and torch.equal(acc[:, 3], counts)


def test_empty_inputs_are_noops():
    """n = 0 sequences: the C ABI returns OK without launching (ragged shards can produce empty tails)."""
    code = ops.dtype_code("fp32")
    x = torch.zeros(0, 5, 8, device=DEV)
    w = torch.randn(8, 8, device=DEV)
    b = torch.randn(8, device=DEV)
    y = ops.mhsa(x, w, b, w, b, w, b, heads=2, code=code)
    assert y.shape == (0, 5, 8)
    out = ops.additive_pool(y, torch.randn(4, 8, device=DEV), torch.randn(4, device=DEV), torch.randn(1, 4, device=DEV),
                            torch.randn(1, device=DEV), code)
    assert out.shape == (0, 8)


# one bf16 NRMS training step at title / history scale: loss and the sum / absolute sum of every parameter gradient
_NRMS_GRAD_SCRIPT = r"""
import json, sys, torch
from types import SimpleNamespace
from newsrecommendation_amd.model import NRMS
torch.manual_seed(0)
args = SimpleNamespace(num_words_title=30, user_log_length=50, npratio=4, word_embedding_dim=300, news_dim=400,
                       num_attention_heads=20, news_query_vector_dim=200, user_query_vector_dim=200, drop_rate=0.2,
                       user_log_mask=False, freeze_embedding=False, compute_dtype="bf16")
g = torch.Generator().manual_seed(3)
import os
V, B = 5000, int(os.environ.get("NR_TEST_B", "64"))   # B * 55 titles of 30 tokens
table = (torch.randn(V, 300, generator=g) * 0.4).numpy(); table[0] = 0
m = NRMS.Model(args, table).cuda().train()
hist = torch.randint(0, V, (B, 50, 30), generator=g, dtype=torch.int32).cuda()
cand = torch.randint(0, V, (B, 5, 30), generator=g, dtype=torch.int32).cuda()
mask = (torch.rand(B, 50, generator=g) < 0.8).float().cuda()
label = torch.randint(0, 5, (B,), generator=g).cuda()
torch.manual_seed(11)
loss, score = m(hist, mask, cand, label)
loss.backward()
torch.cuda.synchronize()
out = {"loss": float(loss)}
for n, p in m.named_parameters():
    if p.grad is not None:
        out[n] = [float(p.grad.double().sum()), float(p.grad.double().abs().sum())]
print("RESULT " + json.dumps(out))
"""


def test_attention_backward_is_independent_of_what_the_workgroup_computed_before():
    """The bf16 attention kernels keep per-head 32x32 LDS images whose padding (columns d..31, rows L..31) must act as
    zeros, and the backward parks its outputs in LDS on top of dead images.  If stale output values leaked into a later
    item's products, huge upstream gradients (1e3) would wreck the scores of the following head groups.  Dense source,
    title shapes, bf16, against the oracle's MHSA in fp32 on the CPU."""
    from oracle import nr_oracle as O
    from newsrecommendation_amd import _lib
    g = torch.Generator().manual_seed(5)
    n, L, dm, h, d = 96, 30, 64, 20, 20
    N = h * d
    x = torch.randn(n, L, dm, generator=g) * 0.5
    ws = [torch.randn(N, dm, generator=g) * 0.1 for _ in range(3)]
    bs = [torch.randn(N, generator=g) * 0.1 for _ in range(3)]
    dy = torch.randn(n, L, N, generator=g) * 1e3
    xr = x.to(torch.bfloat16).float()                      # both sides start from the same bf16 activations
    pr = [t.clone().requires_grad_(True) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
    xo = xr.clone().requires_grad_(True)
    yo = O.mhsa(xo, *pr, h)
    yo.backward(dy)
    pg = [t.clone().to(DEV).requires_grad_(True) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
    xg = xr.to(DEV).to(torch.bfloat16).requires_grad_(True)
    yg = ops.mhsa(xg, *pg, h, _lib.NR_BF16)
    yg.backward(dy.to(DEV).to(yg.dtype))
    assert (yg.float().cpu() - yo.detach()).abs().max().item() <= 2e-2 * yo.detach().abs().max().item() + 1e-3
    for a, b, name in zip(pg, pr, ["wq", "bq", "wk", "bk", "wv", "bv"]):
        if name == "bk":       # analytically 0 (a constant key shift leaves the softmax unchanged): only rounding noise
            continue
        ref = b.grad
        err = (a.grad.cpu() - ref).abs().max().item()
        assert err <= 3e-2 * ref.abs().max().item() + 1e-2, (name, err, ref.abs().max().item())
    gx = xg.grad.float().cpu()
    assert (gx - xo.grad).abs().max().item() <= 3e-2 * xo.grad.abs().max().item() + 1e-2


def test_live_slab_weight_gradients_equal_the_full_contraction():
    """At full scale (>= 200 000 token rows) the two weight-gradient GEMMs of the news encoder contract only the 32-row
    slabs that touch a sequence with a non-zero upstream gradient (NR_NO_SLABS=1 switches that off).  Masked history
    slots have an exactly zero gradient, so both runs must agree up to the order of the fp32 atomics."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(no_slabs):
        env = dict(os.environ, PYTHONPATH=root, NR_TEST_B="160")     # 160 * 55 * 30 = 264 000 rows
        env.pop("NR_NO_SLABS", None)
        if no_slabs:
            env["NR_NO_SLABS"] = "1"
        r = subprocess.run([sys.executable, "-c", _NRMS_GRAD_SCRIPT], env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        return json.loads(line[7:])

    a, b = run(True), run(False)
    assert a["loss"] == b["loss"]
    for k in a:
        if k == "loss":
            continue
        (s0, a0), (s1, a1) = a[k], b[k]
        if k.startswith("news_encoder.multi_head_self_attn") and k.endswith("bias"):
            # NR_NO_SLABS also switches the compact row storage off: db_qkv then comes from the weight-gradient GEMM's column sums
            # over bf16-rounded rows instead of the attention backward's row / column sums (tests/test_gpu_scale_parity.py);
            # d W_K.bias is analytically 0 -- rounding noise in the one, ~1e-11 in the other
            if not k.endswith("W_K.bias"):
                assert abs(a0 - a1) <= 5e-3 * a0 + 1e-6, (k, a0, a1)
            continue
        assert abs(a0 - a1) <= 1e-4 * a0 + 1e-6, (k, a0, a1)
        assert abs(s0 - s1) <= 1e-4 * a0 + 1e-6, (k, s0, s1)
