"""Key-tiled attention kernels (attention_tiled.hip): sequences above 256 tokens, bf16 (matrix cores) and f32 (VALU), against an
f64 evaluation of the same (dtype-rounded) inputs, head by head on the GPU.

Gates per tensor (o, dQ, dK, dV separately):
  f32   norm-relative error < 1e-5 (lse: absolute 1e-5 * max(1, |lse|));
  bf16  cosine > 0.99999 and norm-relative error < 5e-3 -- the bound test_attention_bwd_per_tensor_bound_at_batch_8 holds the
        n = 197 kernels to (lse: absolute 2e-3 * max(1, |lse|); it is computed from f32 scores of the bf16 inputs).
Inputs: uniform entries with one spiked key per head (a near-one-hot row of P); n = 257 also with every score strongly negative
(lse around -190: a padded key's exp against that lse would overflow if it were not masked).

Measured on the MI355X (n = 257 ... 4104, both (b, h)): f32 norm-relative errors 2e-7 - 1e-6; bf16 cosines >= 0.999995 (dQ), norm-
relative errors 1.7e-3 (o), 2.8-3.2e-3 (dQ), 2.5-2.7e-3 (dK), 2.1-2.4e-3 (dV)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [257, 301, 577, 1025, 4104]
BH = [(2, 3), (1, 12)]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def make_inputs(b, n, hh, dt, seed, negative=False):
    """qkv [b*n, 3D] and dO [b*n, D] on the GPU in dtype `dt` (generated on the CPU: the same values in every process)."""
    g = torch.Generator().manual_seed(seed)
    D = hh * 64
    qkv = (torch.rand(b, n, 3, hh, 64, generator=g, dtype=torch.float64) * 2 - 1) * 1.7
    if negative:  # q along +u, k along -u (|u| = 1): every score q.k / 8 about -39 * 39 / 8 = -190
        u = torch.ones(64, dtype=torch.float64) / 8.0
        qkv[:, :, 0] += 39.0 * u
        qkv[:, :, 1] -= 39.0 * u
    else:  # one spiked key per (image, head): key j* = 3 q_i*, so row i* of P is near one-hot
        for bi in range(b):
            for hi in range(hh):
                i_s = int(torch.randint(0, n, (1,), generator=g))
                j_s = int(torch.randint(0, n, (1,), generator=g))
                qkv[bi, j_s, 1, hi] = 3.0 * qkv[bi, i_s, 0, hi]
    do = torch.rand(b, n, D, generator=g, dtype=torch.float64) * 2 - 1
    dev = _dev()
    return qkv.reshape(b * n, 3 * D).to(dev, dt), do.reshape(b * n, D).to(dev, dt)


def reference(qkv, do, b, n, hh):
    """f64: o [b*n, D], lse [b*h*n], dqkv [b*n, 3D] -- one (image, head) at a time"""
    D = hh * 64
    x = qkv.double().view(b, n, 3, hh, 64)
    g = do.double().view(b, n, hh, 64)
    o = torch.empty(b, n, hh, 64, dtype=torch.float64, device=qkv.device)
    lse = torch.empty(b, hh, n, dtype=torch.float64, device=qkv.device)
    dx = torch.empty(b, n, 3, hh, 64, dtype=torch.float64, device=qkv.device)
    dq_terms = torch.empty(b, n, hh, 64, dtype=torch.float64, device=qkv.device)
    for bi in range(b):
        for hi in range(hh):
            q, k, v = x[bi, :, 0, hi], x[bi, :, 1, hi], x[bi, :, 2, hi]
            s = (q @ k.T) / 8.0
            l = torch.logsumexp(s, dim=1)
            p = torch.exp(s - l[:, None])
            oo = p @ v
            gg = g[bi, :, hi]
            dp = gg @ v.T
            ds = p * (dp - (gg * oo).sum(1, keepdim=True)) / 8.0
            o[bi, :, hi], lse[bi, hi] = oo, l
            dx[bi, :, 0, hi], dx[bi, :, 1, hi], dx[bi, :, 2, hi] = ds @ k, ds.T @ q, p.T @ gg
            dq_terms[bi, :, hi] = ds.abs() @ k.abs()
            del s, p, dp, ds
    reference.dq_terms = dq_terms  # size of the terms dQ sums (for the ill-conditioned case)
    return o.view(b * n, D), lse.view(-1), dx.view(b * n, 3 * D)


def parts(dqkv, b, n, hh):
    x = dqkv.view(b, n, 3, hh, 64)
    return {"dq": x[:, :, 0], "dk": x[:, :, 1], "dv": x[:, :, 2]}


def compare(name, a, r, dt, f32_tol=1e-5):
    """(cosine, norm-relative error) of a against r; asserts the dtype's gates"""
    a = a.double().reshape(-1)
    r = r.double().reshape(-1)
    assert torch.isfinite(a).all(), name
    nre = float((a - r).norm() / r.norm())
    cos = float((a @ r) / (a.norm() * r.norm()))
    if dt == torch.float32:
        assert nre < f32_tol, (name, nre)
    else:
        assert cos > 0.99999 and nre < 5e-3, (name, cos, nre)
    return cos, nre


def check_lse(lse, lref, dt):
    assert torch.isfinite(lse).all()
    tol = 1e-5 if dt == torch.float32 else 2e-3
    err = float(((lse.double() - lref).abs() / lref.abs().clamp(min=1.0)).max())
    assert err < tol, err


def run_case(b, n, hh, dt, seed, negative=False):
    from theia_amd import ops
    qkv, do = make_inputs(b, n, hh, dt, seed, negative)
    o, lse = ops.attention_fwd(qkv, b, n, hh)
    dqkv = ops.attention_bwd(qkv, o, do, lse, b, n, hh)
    torch.cuda.synchronize()
    ro, rl, rd = reference(qkv, do, b, n, hh)
    # scores of magnitude ~190 carry an f32 rounding of ~190 * 6e-8 = 1e-5 (absolute), a 1e-5 relative change of P: f32 gate 5e-5 there
    tol = 5e-5 if negative else 1e-5
    res = {"o": compare("o", o, ro, dt, tol)}
    check_lse(lse, rl, dt)
    for k, v in parts(dqkv, b, n, hh).items():
        if negative and k == "dq":
            # every key carries the same large component (-39 u): in dQ_i = sum_j dS_ij k_j it cancels because sum_j dS_ij = 0, exactly
            # only in exact arithmetic, so dQ is ~40x smaller than its terms and any rounding of dS shows at that ratio.  Gated
            # against the size of the terms instead (the forward-error scale of the sum).
            a, r = v.double().reshape(-1), parts(rd, b, n, hh)[k].double().reshape(-1)
            assert torch.isfinite(a).all()
            e = float((a - r).norm() / reference.dq_terms.norm())
            assert e < (tol if dt == torch.float32 else 5e-3), e
            res[k] = (float((a @ r) / (a.norm() * r.norm())), e)
            continue
        res[k] = compare(k, v, parts(rd, b, n, hh)[k], dt, tol)
    return res


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("bh", BH, ids=lambda x: f"b{x[0]}h{x[1]}")
@pytest.mark.parametrize("n", NS)
def test_tiled_attention_matches_f64(n, bh, dt):
    """fwd + bwd at n = 257 ... 4104 (4104: a 1024x1024 input with register tokens); measured values in the module docstring"""
    b, hh = bh
    res = run_case(b, n, hh, dt, seed=1000 + n + 7 * hh)
    print(f"[tiled {dt} n={n} b={b} h={hh}] " + " ".join(f"{k}: cos {c:.7f} nre {e:.2e}" for k, (c, e) in res.items()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_tiled_attention_strongly_negative_scores(dt):
    """every score about -190 at n = 257 (the last 16-key tile holds one real key and 15 padded ones): every output finite, o / lse /
    dK / dV within the usual gates (f32: 5e-5, see run_case), dQ (ill-conditioned here) against the size of its terms"""
    res = run_case(2, 257, 3, dt, seed=77, negative=True)
    print(f"[tiled negative {dt}] " + " ".join(f"{k}: cos {c:.7f} nre {e:.2e}" for k, (c, e) in res.items()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_tiled_attention_backward_is_bit_reproducible(dt):
    from theia_amd import ops
    b, n, hh = 2, 1025, 3
    qkv, do = make_inputs(b, n, hh, dt, 5)
    o, lse = ops.attention_fwd(qkv, b, n, hh)
    o2, lse2 = ops.attention_fwd(qkv, b, n, hh)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    d1 = ops.attention_bwd(qkv, o, do, lse, b, n, hh)
    d2 = ops.attention_bwd(qkv, o, do, lse, b, n, hh)
    assert torch.equal(d1.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                       d2.view(torch.int16 if dt == torch.bfloat16 else torch.int32))


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from theia_amd import ops, _native as N
import importlib.util
spec = importlib.util.spec_from_file_location("tiled_t", sys.argv[2])
t = importlib.util.module_from_spec(spec); spec.loader.exec_module(t)
# the switch is in force: an output overlapping the input is refused at n = 197 (only the tiled launcher checks that; nothing is
# launched -- and if the switch were not read, the default kernel would run in place inside one valid buffer)
lib = N.lib()
buf = torch.zeros(197 * 3 * 64 * 3, dtype=torch.float32, device="cuda:0")
assert lib.theia_attention_fwd(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 197, 3, N.F32, N.stream_ptr()) == -1
assert b"overlap" in lib.theia_last_error()
out = {}
for n in (197, 240):
    for dt in (torch.float32, torch.bfloat16):
        qkv, do = t.make_inputs(2, n, 6, dt, 31 + n)
        o, lse = ops.attention_fwd(qkv, 2, n, 6)
        d = ops.attention_bwd(qkv, o, do, lse, 2, n, 6)
        out[(n, str(dt))] = (o.cpu(), lse.cpu(), d.cpu())
torch.save(out, sys.argv[3])
print("child ok")
"""


def test_tiled_kernels_agree_with_the_default_kernels_in_a_fresh_process(tmp_path):
    """THEIA_ATTN_KERNEL=tiled (read once per process) forces the tiled kernels at every n: at n = 197 (bf16: the MFMA kernels by
    default) and n = 240 (the VALU kernels) they agree with the default dispatch of this process -- f32 to 1e-5, bf16 within the
    per-tensor gates -- and both with the f64 evaluation."""
    from theia_amd import ops
    env = dict(os.environ, THEIA_ATTN_KERNEL="tiled")
    outp = str(tmp_path / "tiled.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.abspath(__file__), outp], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    tiled = torch.load(outp)
    for n in (197, 240):
        for dt in (torch.float32, torch.bfloat16):
            qkv, do = make_inputs(2, n, 6, dt, 31 + n)
            o, lse = ops.attention_fwd(qkv, 2, n, 6)
            d = ops.attention_bwd(qkv, o, do, lse, 2, n, 6)
            to, tl, td = (x.to(o.device) for x in tiled[(n, str(dt))])
            ro, rl, rd = reference(qkv, do, 2, n, 6)
            compare("o", to, o, dt)
            compare("o", to, ro, dt)
            check_lse(tl, rl, dt)
            for k in ("dq", "dk", "dv"):
                compare(k, parts(td, 2, n, 6)[k], parts(d, 2, n, 6)[k], dt)
                compare(k, parts(td, 2, n, 6)[k], parts(rd, 2, n, 6)[k], dt)
