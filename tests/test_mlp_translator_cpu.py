"""MLP translator (translator="mlp"): the parts that need no GPU -- the nearest index map, the C ABI's argument checks, the parameter
layout against the reference's fixture, the gradient buckets, the constructor's refusals, the hub round trip, and the f64
restatement against the reference's own numbers."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_translator_ref as R  # noqa: E402
from oracle import theia_oracle as O  # noqa: E402


def kernel_index(n_in: int, n_out: int) -> np.ndarray:
    """the formula csrc/upsample_rows.hip evaluates, in float32 like the kernel"""
    i = np.arange(n_out)
    if n_out == n_in:
        return i
    if n_out == 2 * n_in:
        return i >> 1
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(i.astype(np.float32) * scale).astype(np.int64), n_in - 1)


@pytest.mark.parametrize("hs", [14])
def test_nearest_index_matches_f_interpolate(hs):
    from theia_amd.models.adapter_heads import nearest_index
    for ht in range(1, 129):
        for wt in (ht, 14, 64):
            # a 2-D index map through F.interpolate: the map is separable, source (row, column) = (hi[y], wi[x])
            idx = torch.arange(hs * hs, dtype=torch.float32).view(1, 1, hs, hs)  # (f32 maps, as the model's activations; f64 input computes its scale in f64)
            got = F.interpolate(idx, size=(ht, wt), mode="nearest").view(ht, wt).long().numpy()
            hi, wi = kernel_index(hs, ht), kernel_index(hs, wt)
            assert (got == hi[:, None] * hs + wi[None, :]).all(), (ht, wt)
        hi = kernel_index(hs, ht)
        assert list(hi) == nearest_index(hs, ht)
        # monotone, so every source index's preimage is one contiguous interval (possibly empty)
        assert (np.diff(hi) >= 0).all() and hi[0] >= 0 and hi[-1] <= hs - 1


def test_new_symbols_are_exported():
    from theia_amd import _native as N
    lib = N.lib()
    for name in ("theia_nearest_rows_fwd", "theia_nearest_rows_bwd"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.theia_abi_version() == 12


@pytest.mark.parametrize("fn", ["theia_nearest_rows_fwd", "theia_nearest_rows_bwd"])
def test_bad_arguments_are_refused(fn):
    """every call here is refused by the host-side checks before anything is launched (the pointers are never dereferenced)"""
    from theia_amd import _native as N
    f = getattr(N.lib(), fn)
    a, b = 1 << 20, 1 << 30  # far apart: no overlap
    ok = dict(b=2, hs=14, ws=14, ht=16, wt=16, C=32)

    def call(src=a, dst=b, dtype=N.BF16, **kw):
        s = dict(ok, **kw)
        return f(src, dst, s["b"], s["hs"], s["ws"], s["ht"], s["wt"], s["C"], dtype, None)

    assert call(src=None) == -1 and call(dst=None) == -1
    for k in ok:
        assert call(**{k: 0}) == -1, k
        assert call(**{k: -3}) == -1, k
    assert call(dtype=N.FP8) == -1 and call(dtype=7) == -1
    # output overlapping the input, from either side
    assert call(src=a, dst=a) == -1
    assert call(src=a, dst=a + 64) == -1
    assert call(src=a + 64, dst=a) == -1
    assert b"overlap" in N.lib().theia_last_error()


def _model(backbone=R.BACKBONE, teachers=R.TEACHERS, **kw):
    from theia_amd.models.rvfm import RobotVisionFM
    return RobotVisionFM(backbone=backbone, translator="mlp", translator_kwargs=kw or None,
                         target_feature_sizes=R.sizes(teachers), precision="fp32")


def test_state_dict_matches_the_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "g18_tiny_mlp_translator.npz"))
    m = _model(translator_hidden_size=int(g["meta_hidden"]), translator_n_layer=int(g["meta_n_layer"]))
    sd = m.state_dict()
    ref = {str(k): tuple(int(x) for x in s if x) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k], k


@pytest.mark.parametrize("n_layer", [1, 2, 3])
def test_state_dict_layout_per_layer_count(n_layer):
    m = _model(translator_n_layer=n_layer, translator_hidden_size=512)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("translator.")}
    assert sd == R.translator_shapes(R.BACKBONE, R.TEACHERS, 512, n_layer)
    for t in R.TEACHERS:
        hm = m.translator.translator_heads[O.head_key(t)]
        assert hm.kind == "mlp" and len(hm.linears()) == n_layer
        assert hm.nearest_index == (list(kernel_index(14, hm.target_size[1])), list(kernel_index(14, hm.target_size[2])))


def test_every_parameter_sits_in_exactly_one_bucket():
    m = _model()
    seen = [id(p) for b in m.engine.buckets for p in b.params]
    assert len(seen) == len(set(seen))
    assert set(seen) == {id(p) for p in m.parameters()}
    names = [b.name for b in m.engine.buckets]
    nh = len(R.TEACHERS)
    assert names[:nh] == [f"head:{t}" for t in R.TEACHERS] and names[nh] == "translator:adapter"
    assert all(n.startswith("vit:") for n in names[nh + 1:])


def test_constructor_refusals():
    from theia_amd.models.feature_translators import build_feature_translator
    from theia_amd.models.rvfm import RobotVisionFM
    with pytest.raises(TypeError):  # the reference's mlp.yaml key: its constructor has no such argument
        _model(hidden_size=1024)
    with pytest.raises(NotImplementedError, match="CLS"):
        RobotVisionFM(backbone=R.BACKBONE, translator="mlp", precision="fp32",
                      target_feature_sizes={"facebook/dinov2-large": (1024, 16, 16), "facebook/dinov2-large_cls": (1024,)})
    for kind in ("conv", "transformer", "trans"):
        with pytest.raises(NotImplementedError):
            build_feature_translator(kind, backbone_feature_size=(192, 14, 14), target_feature_sizes=R.sizes(R.TEACHERS[:1]))


def test_default_initialisers_are_pytorch_defaults():
    torch.manual_seed(0)
    m = _model(translator_hidden_size=256, translator_n_layer=2)
    a = m.translator.backbone_adapter
    assert torch.equal(a["0"].weight, torch.ones(192)) and torch.equal(a["0"].bias, torch.zeros(192))
    for lin in [a["1"]] + m.translator.translator_heads[O.head_key(R.TEACHERS[0])].linears():
        bound = 1.0 / lin.weight.shape[1] ** 0.5
        assert lin.weight.abs().max() <= bound and lin.bias.abs().max() <= bound and lin.weight.std() > bound / 3


def test_hub_round_trip_keeps_translator_type_and_kwargs(tmp_path):
    from theia_amd.hub import TheiaModel
    m = TheiaModel(backbone=R.BACKBONE, translator="mlp", translator_kwargs={"translator_hidden_size": 512, "translator_n_layer": 2},
                   target_feature_sizes=R.sizes(R.TEACHERS[:2]), precision="fp32")
    m.save_pretrained(str(tmp_path))
    r = TheiaModel.from_pretrained(str(tmp_path))
    assert r.config["translator"] == "mlp"
    assert r.config["translator_kwargs"] == {"translator_hidden_size": 512, "translator_n_layer": 2}
    assert r.translator.kind == "mlp" and r.translator.translator_n_layer == 2 and r.translator.translator_hidden_size == 512
    a, b = m.state_dict(), r.state_dict()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    # an lconv model still saves as lconv
    l = TheiaModel(backbone=R.BACKBONE, translator="lconv", translator_kwargs={"hidden_size_factor": 1.0},
                   target_feature_sizes=R.sizes(R.TEACHERS[:1]), precision="fp32")
    l.save_pretrained(str(tmp_path / "l"))
    rl = TheiaModel.from_pretrained(str(tmp_path / "l"))
    assert rl.config["translator"] == "lconv" and rl.translator.kind == "lconv"


def test_config_tree_has_the_reference_mlp_translator():
    from theia_amd.utils import config as cfglib
    cfg = cfglib.compose(["model/translator=mlp"])
    assert cfg.model.translator.type == "mlp"
    assert dict(cfg.model.translator.kwargs) == {"translator_n_layer": 3, "hidden_size": 1024}


def test_restatement_reproduces_the_reference_fixture(golden_dir):
    """the f64 restatement (interpolate first, as the reference) against the reference's own f32 numbers"""
    g = np.load(os.path.join(golden_dir, "g18_tiny_mlp_translator.npz"))
    teachers = [str(t) for t in g["meta_teachers"]]
    params = {k: v.double() for k, v in R.synth_params(str(g["meta_backbone"]), teachers, int(g["meta_hidden"]), int(g["meta_n_layer"])).items()}
    B = int(g["meta_B"])
    images = O.synth_images(B, seed=0)
    targets = O.synth_targets(B, teachers, seed=1)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    losses, main, grads, pred = R.train_step_grads(params, images, targets, str(g["meta_backbone"]), teachers, int(g["meta_n_layer"]))
    for ti, t in enumerate(teachers):
        p = pred[t].numpy().reshape(-1)
        assert tuple(pred[t].shape) == tuple(g[f"pred{ti}_shape"])
        np.testing.assert_allclose(p[g[f"pred{ti}_idx"]], g[f"pred{ti}_val"], rtol=1e-4, atol=1e-5 * np.abs(g[f"pred{ti}_val"]).max())
        assert abs(np.abs(p).sum() - float(g[f"pred{ti}_abssum"])) <= 1e-4 * float(g[f"pred{ti}_abssum"])
    for k in ("mse_loss", "cos_loss", "l1_loss"):
        assert abs(float(losses[k]) - float(g[k])) <= 1e-4 * abs(float(g[k])), k
    assert abs(float(main) - float(g["main_cos_l1"])) <= 1e-4 * abs(float(g["main_cos_l1"]))
    for name, ref in zip(g["grad_names"], g["gradnorm_cos_l1"]):
        if "k_proj.bias" in str(name):  # exactly zero in exact arithmetic (softmax is shift invariant): rounding noise in the fixture
            continue
        got = float(grads[str(name)].norm())
        assert abs(got - ref) <= 1e-3 * ref + 1e-12, (str(name), got, ref)
