"""Shared helpers of the MLP-translator tests: deterministic weights for the translator's parameters and an f64 restatement of the
reference's MLP translator (models/feature_translators.py:12-122, models/adapter_heads.py:61-127) in the reference's own order --
LayerNorm and Linear on every token, then per head: drop CLS, nearest interpolation to the target grid, Linear (-> ReLU -> Linear)*.

Imported by the tests and by tools/gen_golden_mlp.py; it uses the oracle only through its public helpers."""
from __future__ import annotations

import math
import os
import sys
from typing import Dict, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import theia_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g18_tiny_mlp_translator.npz")
BACKBONE = "facebook/deit-tiny-patch16-224"
TEACHERS = ["facebook/dinov2-large", "facebook/sam-vit-huge", "LiheYoung/depth-anything-large-hf", "llava-hf/llava-1.5-7b-hf"]
HIDDEN, N_LAYER, B = 1024, 3, 2
LN_EPS = 1e-5


def sizes(teachers: Sequence[str]) -> Dict[str, Tuple[int, int, int]]:
    return {t: O.MODEL_FEATURE_SIZES[t] for t in teachers}


def translator_shapes(backbone: str, teachers: Sequence[str], hidden: int = HIDDEN, n_layer: int = N_LAYER) -> Dict[str, Tuple[int, ...]]:
    """state_dict names and shapes of the MLP translator, in registration order"""
    C = O._arch(backbone)[0]
    out: Dict[str, Tuple[int, ...]] = {
        "translator.backbone_adapter.0.weight": (C,), "translator.backbone_adapter.0.bias": (C,),
        "translator.backbone_adapter.1.weight": (hidden, C), "translator.backbone_adapter.1.bias": (hidden,),
    }
    for t in teachers:
        Ct = O.MODEL_FEATURE_SIZES[t][0]
        widths = [hidden] + [2 * hidden] * (n_layer - 1) + [Ct]
        for i in range(n_layer):
            p = f"translator.translator_heads.{O.head_key(t)}.adapter.{2 * i}."
            out[p + "weight"] = (widths[i + 1], widths[i])
            out[p + "bias"] = (widths[i + 1],)
    return out


def synth_translator_params(backbone: str, teachers: Sequence[str], hidden: int = HIDDEN, n_layer: int = N_LAYER,
                            seed: int = 0) -> Dict[str, torch.Tensor]:
    """matrices U(+-sqrt(3/fan_in)), biases 0.02 U(+-1), LayerNorm weight 1 +- 0.1 and bias 0.05 U(+-1), from O._hash_uniform"""
    out: Dict[str, torch.Tensor] = {}
    for idx, (name, shape) in enumerate(translator_shapes(backbone, teachers, hidden, n_layer).items()):
        n = int(np.prod(shape))
        u = O._hash_uniform(n, 7000003 + seed * 100003 + idx)
        if name.startswith("translator.backbone_adapter.0."):
            v = 1.0 + 0.1 * u if name.endswith("weight") else 0.05 * u
        elif name.endswith("bias"):
            v = 0.02 * u
        else:
            v = math.sqrt(3.0 / shape[1]) * u
        out[name] = torch.from_numpy(np.ascontiguousarray(v.reshape(shape).astype(np.float32)))
    return out


def synth_params(backbone: str, teachers: Sequence[str], hidden: int = HIDDEN, n_layer: int = N_LAYER, seed: int = 0) -> Dict[str, torch.Tensor]:
    """the whole model: the oracle's backbone weights + the translator's"""
    p = O.synth_params(backbone, [], seed)
    p.update(synth_translator_params(backbone, teachers, hidden, n_layer, seed))
    return p


def translator_forward(params: Dict[str, torch.Tensor], z: torch.Tensor, teachers: Sequence[str], n_layer: int,
                       backbone_no_cls: bool = False) -> Dict[str, torch.Tensor]:
    """z: [b, (1)+196, C] (register tokens already stripped); in the dtype of params / z (f64 for the checks)"""
    a = "translator.backbone_adapter."
    x = F.layer_norm(z, (z.shape[-1],), params[a + "0.weight"], params[a + "0.bias"], LN_EPS)
    x = F.linear(x, params[a + "1.weight"], params[a + "1.bias"])
    out = {}
    for t in teachers:
        _Ct, Ht, Wt = O.MODEL_FEATURE_SIZES[t]
        h = x if backbone_no_cls else x[:, 1:]
        if Ht != O.GRID:  # adapter_heads.py:96-102: Rearrange -> Interpolation(nearest) -> Rearrange
            b, _n, c = h.shape
            m = h.transpose(1, 2).reshape(b, c, O.GRID, O.GRID)
            m = F.interpolate(m, size=(Ht, Wt), mode="nearest")
            h = m.reshape(b, c, Ht * Wt).transpose(1, 2)
        p = f"translator.translator_heads.{O.head_key(t)}.adapter."
        for i in range(n_layer):
            if i:
                h = torch.relu(h)
            h = F.linear(h, params[p + f"{2 * i}.weight"], params[p + f"{2 * i}.bias"])
        out[t] = h
    return out


def forward(params: Dict[str, torch.Tensor], images, backbone: str, teachers: Sequence[str], n_layer: int) -> Dict[str, torch.Tensor]:
    """models/rvfm.py:115-136 with the MLP translator: O.vit_forward, register tokens stripped, then the restatement"""
    ref = next(iter(params.values()))
    z = O.vit_forward(params, O.preprocess(images).to(ref.device, ref.dtype), backbone)
    _base, has_cls, nreg = O.backbone_variant(backbone)
    if nreg:
        z = z[:, :-nreg]
    return translator_forward(params, z, teachers, n_layer, backbone_no_cls=not has_cls)


def train_step_grads(params: Dict[str, torch.Tensor], images, targets: Dict[str, torch.Tensor], backbone: str,
                     teachers: Sequence[str], n_layer: int, loss_kind: str = "cos_l1"):
    """(losses, main loss, gradients by name, predictions) of one step in the dtype of `params`"""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    pred = forward(leaf, images, backbone, teachers, n_layer)
    losses = O.get_loss(pred, {t: targets[t].to(pred[t].dtype) for t in teachers})
    main = O.main_loss(losses, loss_kind)
    main.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    return losses, main.detach(), grads, {k: v.detach() for k, v in pred.items()}


def sample_idx(n: int, k: int, seed: int) -> np.ndarray:
    u = O._hash_uniform(k, 31337 + seed)
    return np.minimum(((u.astype(np.float64) + 1.0) * 0.5 * n).astype(np.int64), n - 1)
