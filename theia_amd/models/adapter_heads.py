"""Per-teacher adapter heads: parameter containers with the reference's names
(reference ``LightConvAdapterHead`` models/adapter_heads.py:232-359, ``MLPAdapterHead`` :61-127, ``LinearAdapterHead`` :28-58).

Key layout kept for checkpoint compatibility: ``pad.1`` (ConvTranspose2d 14->16), ``adapter.{0,3,6}`` (LayerNorm
[C,H,W]), ``adapter.{1,4}`` (Conv2d for 16x16 targets / ConvTranspose2d for 64x64 targets), ``adapter.8`` (Linear).
Compute is in the HIP engine; ``kind`` tells it which branch of the reference constructor this head is."""
from __future__ import annotations

import math
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .backbones import ConvParams, LayerNormParams, LinearParams, _Holder


class _Slot(_Holder):
    """parameter-less positions of the reference's nn.Sequential (Rearrange / ReLU)."""


class LinearAdapterHead(nn.Module):
    """CLS-token distillation head: one Linear on token 0 (reference ``LinearAdapterHead`` adapter_heads.py:28-58;
    ``adapter.0`` = nn.Linear(C, Ct)).  Parameter container; compute is in the HIP engine (``kind == "cls"``)."""

    def __init__(self, source_size, target_size):
        super().__init__()
        self.source_size, self.target_size = tuple(source_size), tuple(target_size)
        self.kind = "cls"
        self.adapter = nn.ModuleDict({"0": LinearParams(int(source_size[0]), int(target_size[0]))})
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self) -> None:
        lin = self.adapter["0"]
        bound = 1.0 / math.sqrt(lin.weight.shape[1])
        nn.init.uniform_(lin.weight, -bound, bound)
        nn.init.uniform_(lin.bias, -bound, bound)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("LinearAdapterHead holds parameters only; use the translator's forward")


def nearest_index(n_in: int, n_out: int) -> List[int]:
    """source index of every output index along one axis, exactly as the reference's 2-D F.interpolate(mode="nearest") picks it
    (adapter_heads.py:96-102; taken from F.interpolate itself on an f32 index map, so it follows PyTorch's float32 scale arithmetic --
    the 1-D form on f64 input would compute its scale in f64 and can differ)"""
    idx = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return [int(v) for v in F.interpolate(idx, size=(n_out, 1), mode="nearest").view(-1).tolist()]


class MLPAdapterHead(nn.Module):
    """MLP head: nearest interpolation of the source grid to the target grid, then ``num_layer`` Linears with ReLUs between them
    (reference adapter_heads.py:61-127; ``adapter.0/2/4/...`` are the Linears, the odd positions the ReLUs, hidden width
    2 * source channels).  Parameter container; compute is in the HIP engine (``kind == "mlp"``), which runs the Linears on the
    source rows and expands their result: nearest interpolation copies rows and the MLP acts on each row alone, so the two commute.
    ``nearest_index`` = (row, column) source index of every target row / column (the map is separable)."""

    def __init__(self, source_size, target_size, num_layer: int):
        super().__init__()
        assert num_layer >= 1, f"`num_layer` in {self._get_name()} should >= 1. Got {num_layer}"
        self.source_size, self.target_size = tuple(source_size), tuple(target_size)
        self.kind = "mlp"
        self.num_layer = int(num_layer)
        Cs, Ct = int(source_size[0]), int(target_size[0])
        hidden = 2 * Cs
        widths = [Cs] + [hidden] * (num_layer - 1) + [Ct]
        self.widths = widths
        mods = {}
        for i in range(num_layer):
            mods[str(2 * i)] = LinearParams(widths[i], widths[i + 1])
            if i + 1 < num_layer:
                mods[str(2 * i + 1)] = _Slot()  # nn.ReLU
        self.adapter = nn.ModuleDict(mods)
        self.nearest_index = (nearest_index(int(source_size[1]), int(target_size[1])),
                              nearest_index(int(source_size[2]), int(target_size[2])))
        self.reset_parameters()

    def linears(self) -> List[LinearParams]:
        return [self.adapter[str(2 * i)] for i in range(self.num_layer)]

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """PyTorch default initialiser of nn.Linear"""
        for lin in self.linears():
            bound = 1.0 / math.sqrt(lin.weight.shape[1])
            nn.init.uniform_(lin.weight, -bound, bound)
            nn.init.uniform_(lin.bias, -bound, bound)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("MLPAdapterHead holds parameters only; use the translator's forward")


class LightConvAdapterHead(nn.Module):
    def __init__(self, source_size, target_size, hidden_size_factor: float = 1.0):
        super().__init__()
        if source_size[1] != source_size[2] or target_size[1] != target_size[2]:
            raise NotImplementedError("Currently does not support non-square feature maps like source size"
                                      "{source_size} and target size {target_size}.")
        if tuple(source_size[1:]) != (14, 14):
            raise NotImplementedError("the MI355X hot path covers the 14x14 DeiT-patch16-224 source map")
        C = int(source_size[0])
        hidden = int(C * hidden_size_factor)
        if hidden != C:
            raise NotImplementedError("hidden_size_factor != 1.0 is not part of the hot path (configs/model/translator/lconv.yaml)")
        Ct, Ht = int(target_size[0]), int(target_size[1])
        self.source_size = (C, 16, 16)  # after padding, as in the reference (adapter_heads.py:290)
        self.target_size = tuple(target_size)
        self.hidden_size_factor = hidden_size_factor
        self.pad = nn.ModuleDict({"0": _Slot(), "1": ConvParams((C, C, 3, 3), C)})  # ConvTranspose2d(C, C, 3, stride 1)
        if Ht == 64:      # adapter_heads.py:304-315
            self.kind, sizes = "up64", (16, 31, 64)
        elif Ht == 16:    # adapter_heads.py:316-327
            self.kind, sizes = "same16", (16, 16, 16)
        else:
            raise NotImplementedError(f"{tuple(source_size)} to {tuple(target_size)} is not supported.")
        self.sizes = sizes
        self.adapter = nn.ModuleDict({
            "0": LayerNormParams((C, sizes[0], sizes[0])),
            "1": ConvParams((C, C, 3, 3), C),
            "2": _Slot(),
            "3": LayerNormParams((C, sizes[1], sizes[1])),
            "4": ConvParams((C, C, 3, 3), C),
            "5": _Slot(),
            "6": LayerNormParams((C, sizes[2], sizes[2])),
            "7": _Slot(),
            "8": LinearParams(C, Ct),
        })
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """PyTorch default initialisers of Conv2d / ConvTranspose2d / Linear (kaiming-uniform a=sqrt(5))."""
        def conv_like(w, b):
            fan_in = w.shape[1] * w.shape[2] * w.shape[3]  # torch uses dim 1 for both conv and conv-transpose
            bound = 1.0 / math.sqrt(fan_in)
            nn.init.uniform_(w, -bound, bound)
            nn.init.uniform_(b, -bound, bound)
        conv_like(self.pad["1"].weight, self.pad["1"].bias)
        conv_like(self.adapter["1"].weight, self.adapter["1"].bias)
        conv_like(self.adapter["4"].weight, self.adapter["4"].bias)
        lin = self.adapter["8"]
        bound = 1.0 / math.sqrt(lin.weight.shape[1])
        nn.init.uniform_(lin.weight, -bound, bound)
        nn.init.uniform_(lin.bias, -bound, bound)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("LightConvAdapterHead holds parameters only; use the translator's forward")
