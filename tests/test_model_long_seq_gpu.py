"""The student on inputs above 256 tokens: forward_feature(img, do_resize=False, interpolate_pos_encoding=True) at 256x256,
240x320 and 512x512 (257 / 301 / 1025 tokens for DeiT, one fewer for nocls-, seven more for reg-) runs through the key-tiled
attention kernels, against the CPU oracle's forward_feature and its autograd gradients on the same parameters and images.

fp32: the tolerances of the 160x192 golden test (G17): features 1e-4 relative to their max, abs-sum 1e-5; gradients of the
position table, a mid-depth weight and the patch projection: norm 1e-3 relative (and their difference within 1e-2 of the norm).
bf16 / fp8 at 512x512: finite features; gradient cosines against the oracle above the model tests' per-tensor gates (0.99 / 0.9)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import theia_oracle as O  # noqa: E402  (checker only)

SIZES = [(256, 256), (240, 320), (512, 512)]
BACKBONES = [("deit", "facebook/deit-tiny-patch16-224"), ("nocls", "nocls-facebook/deit-tiny-patch16-224"),
             ("reg", "reg-facebook/deit-tiny-patch16-224")]
GRADS = (("pos", "backbone.model.embeddings.position_embeddings"), ("fc1", "backbone.model.layers.3.mlp.fc1.weight"),
         ("patch", "backbone.model.embeddings.patch_embeddings.projection.weight"))


def build(backbone, teachers, precision, seed=0):
    from theia_amd.models.rvfm import RobotVisionFM
    from theia_amd.foundation_models.common import get_model_feature_size
    m = RobotVisionFM(backbone=backbone, translator="lconv", translator_kwargs={"hidden_size_factor": 1.0},
                      target_feature_sizes={t: (get_model_feature_size(t[:-4], keep_spatial=True)[:1] if t.endswith("_cls")
                                                else get_model_feature_size(t, keep_spatial=True)) for t in teachers},
                      precision=precision)
    params = O.synth_params(backbone, teachers, seed)
    m.load_state_dict(params, strict=True)
    return m.to("cuda:0"), params


def images(b, hh, ww, seed):
    return torch.from_numpy((O._hash_uniform(b * hh * ww * 3, seed) * 0.5 + 0.5).reshape(b, hh, ww, 3) * 255.999).to(torch.uint8)


def oracle(params, img, bb):
    """the oracle's features and the gradients of (z * w).sum() (w: fixed hash weights) with respect to every parameter"""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    z = O.forward_feature(leaf, img, bb, interpolate_pos_encoding=True)
    w = torch.from_numpy(O._hash_uniform(z.numel(), 77).reshape(tuple(z.shape)).copy())
    (z * w).sum().backward()
    return z.detach(), w, {k: v.grad for k, v in leaf.items() if v.grad is not None}


def run(model, img, w):
    model.zero_grad(set_to_none=True)
    z = model.forward_feature(img, do_resize=False, interpolate_pos_encoding=True)
    (z.float() * w.to(z.device)).sum().backward()
    torch.cuda.synchronize()
    return z.detach().float().cpu(), dict(model.named_parameters())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("tag,bb", BACKBONES, ids=[t for t, _ in BACKBONES])
def test_fp32_long_sequences_match_the_oracle(tag, bb, size):
    hh, ww = size
    model, params = build(bb, O.TEACHER_SETS["dinov2"], "fp32")
    img = images(2, hh, ww, 700 + hh + ww)
    zr, w, gr = oracle(params, img, bb)
    z, sdp = run(model, img, w)
    assert tuple(z.shape) == tuple(zr.shape)
    zz, rr = z.double().numpy().reshape(-1), zr.double().numpy().reshape(-1)
    assert np.abs(zz - rr).max() / np.abs(rr).max() < 1e-4
    assert abs(np.abs(zz).sum() - np.abs(rr).sum()) / np.abs(rr).sum() < 1e-5
    for short, k in GRADS:
        a, b = sdp[k].grad.detach().double().cpu().reshape(-1), gr[k].double().reshape(-1)
        assert abs(float(a.norm() / b.norm()) - 1.0) < 1e-3, (tag, short)
        assert float((a - b).norm() / b.norm()) < 1e-2, (tag, short)


@pytest.mark.parametrize("precision,gate", [("bf16", 0.99), ("fp8", 0.9)])
@pytest.mark.parametrize("tag,bb", BACKBONES, ids=[t for t, _ in BACKBONES])
def test_low_precision_long_sequences_track_the_oracle(tag, bb, precision, gate):
    """512x512 (1025 tokens for DeiT): bf16 / fp8 modes, second pass (fp8: every quantisation site calibrated by the first)"""
    model, params = build(bb, O.TEACHER_SETS["dinov2"], precision)
    img = images(2, 512, 512, 1900)
    zr, w, gr = oracle(params, img, bb)
    for _ in range(2):
        z, sdp = run(model, img, w)
    assert tuple(z.shape) == tuple(zr.shape) and torch.isfinite(z).all()
    cz = float(torch.nn.functional.cosine_similarity(z.double().reshape(1, -1), zr.double().reshape(1, -1)))
    cos = {}
    for short, k in GRADS:
        a, b = sdp[k].grad.detach().double().cpu().reshape(-1), gr[k].double().reshape(-1)
        assert torch.isfinite(a).all(), short
        cos[short] = float((a @ b) / (a.norm() * b.norm()))
    print(f"[{precision} {tag} 512x512] feature cosine {cz:.5f}; gradient cosines " + " ".join(f"{k} {v:.5f}" for k, v in cos.items()))
    assert all(c > gate for c in cos.values()), cos
