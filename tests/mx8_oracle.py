"""The fp32 oracle with the MX fp8 round trip of precision="mxfp8" (tests/mx8_ref.py) applied to the operands of the five covered
GEMM sites of every ViT layer -- q/k/v, fc1 and fc2 forward (activation and weight), fc2 and fc1 data-gradient (incoming gradient and
W^T) -- and exact f32 everywhere else.  It separates what the format costs from what the kernels and the engine cost: the engine's
gradients are compared against both this and the plain oracle."""
import contextlib
import math

import torch

from mx8_ref import dequantize, quantize
from oracle import theia_oracle as O  # checker only


def _rt(x2d: torch.Tensor) -> torch.Tensor:
    q, s = quantize(x2d)
    return dequantize(q, s).to(x2d.dtype)


class _MXLinear(torch.autograd.Function):
    """y = rt(x) @ rt(W)^T; dx = rt(dy) @ rt(W^T)^T when dgrad (fc1 / fc2), else dy @ W (q/k/v); dW = dy^T x exactly"""

    @staticmethod
    def forward(ctx, x, W, dgrad):
        ctx.save_for_backward(x, W)
        ctx.dgrad = dgrad
        return (_rt(x.reshape(-1, x.shape[-1])) @ _rt(W).t()).reshape(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x, W = ctx.saved_tensors
        g2, x2 = gy.reshape(-1, gy.shape[-1]), x.reshape(-1, x.shape[-1])
        gx = _rt(g2) @ _rt(W.t().contiguous()).t() if ctx.dgrad else g2 @ W
        return gx.reshape(x.shape), g2.t() @ x2, None


def _vit_forward_mx(params, pix, backbone, interpolate_pos_encoding=False):
    """theia_oracle.vit_forward (224 input) with the MX sites"""
    assert not interpolate_pos_encoding
    D, nh, _F = O._arch(backbone)
    _base, has_cls, nreg = O.backbone_variant(backbone)
    dh, b = D // nh, pix.shape[0]
    e = "backbone.model.embeddings."
    Wp = params[e + "patch_embeddings.projection.weight"].reshape(D, -1)
    emb = O.patch_matrix(pix) @ Wp.t() + params[e + "patch_embeddings.projection.bias"]
    pos = params[e + "position_embeddings"][0]
    toks = [emb + pos[1:]]
    if has_cls:
        toks.insert(0, (params[e + "cls_token"][0] + pos[:1]).expand(b, 1, D))
    if nreg:
        toks.append((params[e + "reg_token"][0] + params[e + "reg_pos_embed"][0]).expand(b, nreg, D))
    h = torch.cat(toks, dim=1)
    n = h.shape[1]
    for i in range(O.NUM_LAYERS):
        p = f"backbone.model.layers.{i}."
        a = O._layernorm_rows(h, params[p + "layernorm_before.weight"], params[p + "layernorm_before.bias"], O.LN_EPS_VIT)
        Wqkv = torch.cat([params[p + f"attention.{t}.weight"] for t in ("q_proj", "k_proj", "v_proj")], 0)
        bqkv = torch.cat([params[p + f"attention.{t}.bias"] for t in ("q_proj", "k_proj", "v_proj")], 0)
        q, k, v = (_MXLinear.apply(a, Wqkv, False) + bqkv).split(D, dim=-1)
        q, k, v = (t.view(b, n, nh, dh).transpose(1, 2) for t in (q, k, v))
        o = (torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh)), dim=-1) @ v).transpose(1, 2).reshape(b, n, D)
        h = h + (o @ params[p + "attention.o_proj.weight"].t() + params[p + "attention.o_proj.bias"])
        m = O._layernorm_rows(h, params[p + "layernorm_after.weight"], params[p + "layernorm_after.bias"], O.LN_EPS_VIT)
        m = O._gelu_erf(_MXLinear.apply(m, params[p + "mlp.fc1.weight"], True) + params[p + "mlp.fc1.bias"])
        h = h + (_MXLinear.apply(m, params[p + "mlp.fc2.weight"], True) + params[p + "mlp.fc2.bias"])
    return O._layernorm_rows(h, params["backbone.model.layernorm.weight"], params["backbone.model.layernorm.bias"], O.LN_EPS_VIT)


@contextlib.contextmanager
def _mx_sites():
    orig = O.vit_forward
    O.vit_forward = _vit_forward_mx
    try:
        yield
    finally:
        O.vit_forward = orig


def train_step_grads_mx(params, images, targets, backbone, teachers, loss_kind="cos_l1"):
    """O.train_step_grads with the MX round trips at the covered sites"""
    with _mx_sites():
        return O.train_step_grads(params, images, targets, backbone, teachers, loss_kind)


def worst_cosine(grads, grads_ref, min_numel=4096):
    """(worst per-tensor cosine, its name) over the tensors with >= min_numel elements, k_proj excluded (as test_model_gpu.py does)"""
    worst, who = 1.0, ""
    for k, r in grads_ref.items():
        if "k_proj" in k or r.numel() < min_numel:
            continue
        a, b = grads[k].detach().float().cpu().reshape(-1).double(), r.detach().float().cpu().reshape(-1).double()
        c = float((a @ b) / (a.norm() * b.norm() + 1e-30))
        if c < worst:
            worst, who = c, k
    return worst, who
