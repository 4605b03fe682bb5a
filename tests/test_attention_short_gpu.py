"""Short-sequence attention (n <= 256 tokens): every branch of theia_attention_fwd / _bwd against an f64 evaluation of the same
(dtype-rounded) inputs, all (image, head) pairs at once on the GPU.

Branches (attention.hip / attention_mfma.hip):
  bf16 n <= 192          MFMA forward, every key tile masked (TAIL = false)
  bf16 193 <= n <= 208   MFMA forward, only the last key tile masked (TAIL = true)
  bf16 n <= 208          fused persistent MFMA backward (grid min(b*h, CU budget), a workgroup walks heads blockIdx.x + k*gridDim.x);
                         THEIA_ATTN_BWD=split: the two-kernel MFMA backward
  bf16 209 <= n <= 256   VALU kernels
  f32  n <= 256          VALU kernels, rows split attn_nsplit(b*h, n) ways (8 up to b*h ~ 100, 1 at b*h >= 768)
  THEIA_ATTN_KERNEL=tiled  the key-tiled kernels at every n (below 197 tokens: one partial 64-row block)

Gates per tensor (those of test_attention_tiled_gpu.py):
  f32   norm-relative error < 1e-5 (5e-5 with strongly negative scores); lse within 1e-5 * max(1, |lse|);
  bf16  cosine > 0.99999 and norm-relative error < 5e-3; lse within 2e-3 * max(1, |lse|);
  every output finite.  Where the exact result vanishes or cancels -- dQ and dK at n = 1 (P = 1, O = V, so dS = 0), dQ with strongly
  negative scores (sum_j dS_ij = 0 against a component every key shares) -- the error is measured against the size of the terms the
  sum adds up (|dS| |K|, |dS|^T |Q|) with the same tolerances.
The backward is checked as the operation it is, a function of (QKV, O, dO, lse): the f64 delta = rowsum(dO o O) is formed from the O
the forward returned (the forward's O is checked against the exact one above).  Against the exact O instead, the MI355X measured bf16
dQ 1.05e-2 at n = 2 and dK 5.6e-3 with negative scores at n = 17 (norm-relative): the 2^-9 rounding of the stored bf16 O moves delta,
and dS = P (dP - delta) / 8 cancels at these shapes.  A CPU emulation of the kernels' roundings gives the same (1.0e-2, 5.3e-3), and
1.4e-3 / 1.6e-3 with an unrounded O -- the cost of a bf16 O, not of the kernels.
Inputs: make_inputs of the tiled module (uniform entries, one spiked key per head; `negative`: every score about -190, so the
log-sum-exp is about -190 and exp(-lse) of an unmasked padded key overflows f32).

Measured on the MI355X: see the attention rows of DESIGN.md section 3 (the tests print their numbers with -s)."""
import os
import subprocess
import sys

import pytest
import torch

from test_attention_tiled_gpu import make_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
DTS = [("f32", torch.float32), ("bf16", torch.bfloat16)]
NS = [1, 2, 16, 17, 50, 64, 65, 101, 145, 192, 193, 196, 197, 204, 208, 209, 226, 240, 255, 256]
NEG_NS = [17, 192, 197, 208, 240, 256]
HEADS = [(1, 1), (11, 12), (25, 12), (64, 12)]  # f32: 7-8, 6, 3 and 1 row splits; bf16 b*h = 768: more heads than CUs
HEAD_NS = [50, 197, 240]

SWEEP = [pytest.param(n, dt, id=f"n{n}-{dn}") for dn, dt in DTS for n in NS]
NEG = [pytest.param(n, dt, id=f"n{n}-{dn}") for dn, dt in DTS for n in NEG_NS]


def reference(qkv, do, b, n, hh, o_bwd=None):
    """f64 of the given (rounded) inputs, every (image, head) at once, on their device: o / dq / dk / dv [b, n, h, 64], lse [b, h, n],
    and the term scales dq_terms = |dS| |K|, dk_terms = |dS|^T |Q| [b, n, h, 64].
    o_bwd: the forward output the backward is given ([b*n, D] or [b, n, h, 64]); delta = rowsum(dO o O) is formed from it, as the
    backward kernels do (default: the exact o)."""
    x = qkv.double().view(b, n, 3, hh, 64).permute(2, 0, 3, 1, 4)  # [3, b, h, n, 64]
    q, k, v = x[0], x[1], x[2]
    g = do.double().view(b, n, hh, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / 8.0
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    del s
    o = p @ v
    dp = g @ v.transpose(-1, -2)
    gdo = g * (o if o_bwd is None else o_bwd.double().reshape(b, n, hh, 64).transpose(1, 2))
    ds = p * (dp - gdo.sum(-1, keepdim=True)) / 8.0
    if n == 1:  # dS = P (dP - delta) / 8 vanishes exactly (P = 1, O = V, delta = dP): its size is that of the difference's terms
        dsz = p * (g.abs() @ v.abs().transpose(-1, -2) + gdo.abs().sum(-1, keepdim=True)) / 8.0
    else:
        dsz = ds.abs()
    del dp, gdo
    t = lambda a: a.transpose(1, 2)  # [b, h, n, 64] -> [b, n, h, 64]
    return {"o": t(o), "lse": lse, "dq": t(ds @ k), "dk": t(ds.transpose(-1, -2) @ q), "dv": t(p.transpose(-1, -2) @ g),
            "dq_terms": t(dsz @ k.abs()), "dk_terms": t(dsz.transpose(-1, -2) @ q.abs())}


def kernels(qkv, do, b, n, hh):
    """the library's forward + backward: o / dq / dk / dv [b, n, h, 64], lse [b, h, n], and dqkv as launched"""
    from theia_amd import ops
    o, lse = ops.attention_fwd(qkv, b, n, hh)
    dqkv = ops.attention_bwd(qkv, o, do, lse, b, n, hh)
    torch.cuda.synchronize()
    x = dqkv.view(b, n, 3, hh, 64)
    return {"o": o.view(b, n, hh, 64), "lse": lse.view(b, hh, n), "dq": x[:, :, 0], "dk": x[:, :, 1], "dv": x[:, :, 2], "dqkv": dqkv}


def check(out, ref, n, dt, negative=False):
    """asserts the gates of the module docstring; returns {tensor: (cosine or None, error)}"""
    f32 = dt == torch.float32
    tol = (5e-5 if negative else 1e-5) if f32 else 5e-3
    res = {}
    for name in ("o", "dq", "dk", "dv"):
        a, r = out[name].double().reshape(-1), ref[name].reshape(-1)
        assert torch.isfinite(a).all(), (name, int((~torch.isfinite(a)).sum()), "non-finite outputs")
        if (n == 1 and name in ("dq", "dk")) or (negative and name == "dq"):
            e = float((a - r).norm() / ref[name + "_terms"].norm())
            assert e < tol, (name, "error / term scale", e)
            res[name] = (None, e)
            continue
        nre = float((a - r).norm() / r.norm())
        cos = float((a @ r) / (a.norm() * r.norm()))
        assert nre < tol and (f32 or cos > 0.99999), (name, cos, nre)
        res[name] = (cos, nre)
    lse = out["lse"].double()
    assert torch.isfinite(lse).all(), "lse not finite"
    e = float(((lse - ref["lse"]).abs() / ref["lse"].abs().clamp(min=1.0)).max())
    assert e < (1e-5 if f32 else 2e-3), ("lse", e)
    res["lse"] = (None, e)
    return res


def run_case(b, n, hh, dt, seed, negative=False, tag=""):
    qkv, do = make_inputs(b, n, hh, dt, seed, negative)
    out = kernels(qkv, do, b, n, hh)
    res = check(out, reference(qkv, do, b, n, hh, out["o"]), n, dt, negative)
    env = " ".join(f"{k}={os.environ[k]}" for k in ("THEIA_ATTN_BWD", "THEIA_ATTN_KERNEL") if k in os.environ)
    print(f"[short{tag} {env} {str(dt)[6:]} n={n} b={b} h={hh}] "
          + " ".join(f"{k}: " + (f"cos {c:.7f} " if c is not None else "") + f"err {e:.2e}" for k, (c, e) in res.items()))
    return out


@pytest.mark.parametrize("n,dt", SWEEP)
def test_short_attention_matches_f64(n, dt):
    """every n the dispatch treats differently, (b, h) = (2, 3): masked-tile MFMA forward (n <= 192), tail-masked (193 - 208), the
    nocls- / reg- token counts 196 / 204, interpolated inputs (101, 145, 226), the dispatch edges 208 / 209 / 256, n = 1 and 2"""
    run_case(2, n, 3, dt, seed=2000 + n)


@pytest.mark.parametrize("n,dt", NEG)
def test_short_attention_strongly_negative_scores(n, dt):
    """lse about -190: keys beyond n (padded to 16-key tiles in the MFMA kernels, to 64-row blocks in the tiled ones) must get an
    exactly zero probability and dS -- exp(-lse) of such a key is +inf in f32, and inf x 0 in dQ = dS K is NaN.  n = 208 and 256
    have no padded key in the MFMA resp. VALU kernels."""
    run_case(2, n, 3, dt, seed=300 + n, negative=True, tag=" negative")


@pytest.mark.parametrize("dn,dt", DTS, ids=[d[0] for d in DTS])
@pytest.mark.parametrize("n", HEAD_NS)
@pytest.mark.parametrize("bh", HEADS, ids=lambda x: f"b{x[0]}h{x[1]}")
def test_short_attention_head_counts(bh, n, dn, dt):
    """the row split of the VALU kernels (7-8, 6, 3, 1 ways) and the persistent backward with more heads (768) than workgroups"""
    b, hh = bh
    run_case(b, n, hh, dt, seed=4000 + n + 13 * b)


def test_short_attention_bench_shape():
    """b = 128, h = 12, n = 197, bf16: the shape the benchmark step runs (1536 heads over the persistent backward's grid)"""
    run_case(128, 197, 12, torch.bfloat16, seed=5)


@pytest.mark.parametrize("n", [50, 197, 208])
def test_persistent_backward_under_a_small_cu_budget(n):
    """bf16, 96 heads on 1, 7, 13 or 16 workgroups (the CU budget caps the fused backward's grid): a workgroup walks many heads,
    prefetching the next one's pieces, its idle waves rotate with the head, and the last iterations of a workgroup run past the
    last head.  A head is computed by one workgroup in a fixed order, so every budget must give the full-device result bit for bit
    (and that result must meet the f64 gates)."""
    from theia_amd import ops
    b, hh, dt = 8, 12, torch.bfloat16
    qkv, do = make_inputs(b, n, hh, dt, seed=600 + n)
    prev = ops.get_compute_cus()
    try:
        ops.set_compute_cus(0)
        full = kernels(qkv, do, b, n, hh)
        ref = reference(qkv, do, b, n, hh, full["o"])
        check(full, ref, n, dt)
        for c in (1, 7, 13, 16):
            ops.set_compute_cus(c)
            assert ops.get_compute_cus() == c
            out = kernels(qkv, do, b, n, hh)
            res = check(out, ref, n, dt)
            assert torch.equal(out["o"].view(torch.int16), full["o"].view(torch.int16))
            differ = int((out["dqkv"].view(torch.int16) != full["dqkv"].view(torch.int16)).sum())
            assert differ == 0, (c, differ, "dQKV entries differ from the full-device run")
            print(f"[short cus={c} n={n}] " + " ".join(f"{k}: err {e:.2e}" for k, (_, e) in res.items()))
    finally:
        ops.set_compute_cus(prev)


def _child(env_key, env_val, ids):
    """the given tests of this module in a child pytest with env_key=env_val (the switches are read once per process)"""
    env = dict(os.environ, **{env_key: env_val})
    assert ids and not any("fresh_process" in i for i in ids)  # only the named cases (never this test itself again)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-s", *[f"{HERE}::{i}" for i in ids]], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"{len(ids)} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    print("\n".join(l[l.index("[short"):] for l in r.stdout.splitlines() if "[short" in l))  # (behind pytest's progress dots)


def _ids(test, params, keep=lambda n, dt: True):
    return [f"{test}[{p.id}]" for p in params if keep(*p.values)]


def test_split_mfma_backward_in_a_fresh_process():
    """THEIA_ATTN_BWD=split: the two-kernel MFMA backward on every bf16 n <= 208 of the n sweep and of the negative-score cases"""
    mfma = lambda n, dt: dt == torch.bfloat16 and n <= 208
    _child("THEIA_ATTN_BWD", "split", _ids("test_short_attention_matches_f64", SWEEP, mfma)
           + _ids("test_short_attention_strongly_negative_scores", NEG, mfma))


def test_tiled_kernels_below_257_tokens_in_a_fresh_process():
    """THEIA_ATTN_KERNEL=tiled: the key-tiled kernels on every case of the n sweep and of the negative-score cases"""
    _child("THEIA_ATTN_KERNEL", "tiled", _ids("test_short_attention_matches_f64", SWEEP)
           + _ids("test_short_attention_strongly_negative_scores", NEG))
