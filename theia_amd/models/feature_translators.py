"""``lconv`` and ``mlp`` feature translators (reference models/feature_translators.py:12-122,159-205,293-313).

backbone_adapter = Identity and translator_stem = Identity for ``lconv`` (feature_translators.py:56,183), so that
translator is just the per-teacher heads; ``mlp`` keeps the base class's backbone_adapter = LayerNorm(C) -> Linear(C, hidden)
(:49-55) in front of one MLPAdapterHead per teacher (:114-122).  Head module names are the teacher names with '.' -> '_' (:46)."""
from __future__ import annotations

import math
from typing import Any, Optional

import torch
import torch.nn as nn

from .adapter_heads import LightConvAdapterHead, LinearAdapterHead, MLPAdapterHead
from .backbones import LayerNormParams, LinearParams


class LightConvFeatureTranslator(nn.Module):
    kind = "lconv"

    def __init__(self, backbone_feature_size, target_feature_sizes: dict, translator_hidden_size: int = 1024,
                 hidden_size_factor: float = 1.0) -> None:
        super().__init__()
        self.backbone_feature_size = backbone_feature_size
        self.target_feature_sizes = target_feature_sizes
        self.translator_hidden_size = translator_hidden_size
        self.hidden_size_factor = hidden_size_factor
        self.target_model_names = list(target_feature_sizes.keys())
        self.legit_target_model_name_map = {t: t.replace(".", "_") for t in self.target_model_names}
        heads = {}
        for t, size in target_feature_sizes.items():
            if "_cls" in t:  # feature_translators.py:193-197: "<teacher>_cls" targets get a Linear head on the CLS token
                heads[self.legit_target_model_name_map[t]] = LinearAdapterHead(backbone_feature_size, size)
            else:
                heads[self.legit_target_model_name_map[t]] = LightConvAdapterHead(backbone_feature_size, size, hidden_size_factor)
        self.translator_heads = nn.ModuleDict(heads)
        self._engine = None  # set by RobotVisionFM

    def forward(self, x: torch.Tensor, target_model_names: Optional[list] = None, backbone_no_cls: bool = False) -> dict:
        if self._engine is None:
            raise RuntimeError("the translator is driven by RobotVisionFM's engine")
        # backbone_no_cls (nocls- students: heads take all 196 tokens instead of x[:, 1:], adapter_heads.py:355-356) is a property
        # of the engine's token layout: it reads the patch rows in place for every student
        assert bool(backbone_no_cls) == (self._engine.tok0 == 0), "backbone_no_cls does not match the student's token layout"
        names = target_model_names if target_model_names is not None else self.target_model_names
        return self._engine.translator(x, list(names))


class MLPFeatureTranslator(nn.Module):
    """backbone_adapter (LayerNorm eps 1e-5, Linear C -> translator_hidden_size) + one MLPAdapterHead per teacher with source size
    (translator_hidden_size, 14, 14).  Parameter container; the engine runs it (engine.StudentEngine._mlp_fwd / _mlp_bwd)."""
    kind = "mlp"

    def __init__(self, backbone_feature_size, target_feature_sizes: dict, translator_hidden_size: int = 1024,
                 translator_n_layer: int = 3) -> None:
        super().__init__()
        self.backbone_feature_size = backbone_feature_size
        self.target_feature_sizes = target_feature_sizes
        self.translator_hidden_size = translator_hidden_size
        self.translator_n_layer = translator_n_layer
        self.target_model_names = list(target_feature_sizes.keys())
        self.legit_target_model_name_map = {t: t.replace(".", "_") for t in self.target_model_names}
        C = int(backbone_feature_size[0])
        self.backbone_adapter = nn.ModuleDict({"0": LayerNormParams((C,)), "1": LinearParams(C, int(translator_hidden_size))})
        source_size = (int(translator_hidden_size), *backbone_feature_size[1:])
        heads = {}
        for t, size in target_feature_sizes.items():
            if "_cls" in t or len(size) < 3:
                # the reference builds every head as MLPAdapterHead, whose constructor reads target_size[1] (adapter_heads.py:95):
                # a "_cls" target's size is (C,), so the reference's MLP translator cannot be built with one either
                raise NotImplementedError(f"target '{t}': the MLP translator has no CLS-token head (the reference's MLPAdapterHead "
                                          f"indexes target_size[1] of the 1-tuple {tuple(size)})")
            heads[self.legit_target_model_name_map[t]] = MLPAdapterHead(source_size, size, translator_n_layer)
        self.translator_heads = nn.ModuleDict(heads)
        self.reset_parameters()
        self._engine = None  # set by RobotVisionFM

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """PyTorch defaults: LayerNorm (1, 0), nn.Linear kaiming-uniform a=sqrt(5) -> U(+-1/sqrt(fan_in)) for weight and bias"""
        nn.init.ones_(self.backbone_adapter["0"].weight)
        nn.init.zeros_(self.backbone_adapter["0"].bias)
        lin = self.backbone_adapter["1"]
        bound = 1.0 / math.sqrt(lin.weight.shape[1])
        nn.init.uniform_(lin.weight, -bound, bound)
        nn.init.uniform_(lin.bias, -bound, bound)

    def forward(self, x: torch.Tensor, target_model_names: Optional[list] = None, backbone_no_cls: bool = False) -> dict:
        if self._engine is None:
            raise RuntimeError("the translator is driven by RobotVisionFM's engine")
        assert bool(backbone_no_cls) == (self._engine.tok0 == 0), "backbone_no_cls does not match the student's token layout"
        names = target_model_names if target_model_names is not None else self.target_model_names
        return self._engine.translator(x, list(names))


def build_feature_translator(translator_type: str, **kwargs: Any) -> nn.Module:
    if translator_type == "lconv":
        return LightConvFeatureTranslator(**kwargs)
    if translator_type == "mlp":
        return MLPFeatureTranslator(**kwargs)
    if translator_type in ("conv", "transformer", "trans"):
        raise NotImplementedError(f"translator '{translator_type}' is out of the hot-path scope (only 'lconv', the reference default)")
    raise NotImplementedError(f"Requested {translator_type} is not implemented yet.")
