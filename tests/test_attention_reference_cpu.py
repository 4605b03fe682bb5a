"""The batched f64 attention reference of test_attention_short_gpu.py, on the CPU, against torch.autograd of softmax(Q K^T / 8) V:
the oracle the short-sequence kernel tests gate against is itself checked without a GPU."""
import pytest
import torch

from test_attention_short_gpu import reference


@pytest.mark.parametrize("n", [1, 17, 50])
def test_batched_reference_matches_autograd(n):
    b, hh = 2, 3
    D = hh * 64
    g = torch.Generator().manual_seed(70 + n)
    qkv = (torch.rand(b * n, 3 * D, generator=g, dtype=torch.float64) * 2 - 1) * 1.7
    do = torch.rand(b * n, D, generator=g, dtype=torch.float64) * 2 - 1
    ref = reference(qkv, do, b, n, hh)

    x = qkv.clone().requires_grad_(True)
    q, k, v = (t.reshape(b, n, hh, 64).transpose(1, 2) for t in x.split(D, dim=-1))
    s = (q @ k.transpose(-1, -2)) / 8.0
    o = torch.softmax(s, dim=-1) @ v
    (o * do.view(b, n, hh, 64).transpose(1, 2)).sum().backward()
    dx = x.grad.view(b, n, 3, hh, 64)

    def close(a, r, scale):
        assert a.shape == r.shape
        assert float((a - r).abs().max()) <= 1e-12 * float(scale.abs().max()), float((a - r).abs().max())

    close(ref["o"], o.detach().transpose(1, 2), o.detach())
    close(ref["lse"], torch.logsumexp(s.detach(), dim=-1), s.detach())
    for i, name in enumerate(("dq", "dk", "dv")):
        # dQ / dK vanish at n = 1: measured against their term scales there (what the GPU tests gate them with)
        scale = ref[name + "_terms"] if name + "_terms" in ref else dx[:, :, i]
        close(ref[name], dx[:, :, i], scale)
    # the term scales bound what they scale
    assert (ref["dq"].abs() <= ref["dq_terms"] * (1 + 1e-12)).all() and (ref["dk"].abs() <= ref["dk_terms"] * (1 + 1e-12)).all()
    assert float(ref["dq_terms"].min()) > 0 and float(ref["dk_terms"].min()) > 0
