"""Generate tests/golden/g18_tiny_mlp_translator.npz from the REFERENCE's own RobotVisionFM(translator="mlp").

Needs the reference source tree (oracle.gen_golden.import_reference); run where it exists, never on the GPU machines:

    python tools/gen_golden_mlp.py

The reference model gets the deterministic weights of tests/mlp_translator_ref.py (backbone from the oracle's synth_params), runs
forward / get_loss / backward at b = 2 on the oracle's synthetic images and targets, and the fixture keeps data only: the state_dict
keys and shapes, sampled predictions with their absolute sums, the losses and every parameter's gradient norm."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import gen_golden as G  # noqa: E402
from oracle import theia_oracle as O  # noqa: E402
import mlp_translator_ref as R  # noqa: E402


def main() -> None:
    RobotVisionFM, gmfs, _hfo = G.import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model = RobotVisionFM(backbone=R.BACKBONE, pretrained=False, translator="mlp",
                          translator_kwargs={"translator_hidden_size": R.HIDDEN, "translator_n_layer": R.N_LAYER},
                          target_feature_sizes={t: gmfs(t, keep_spatial=True) for t in R.TEACHERS})
    params = R.synth_params(R.BACKBONE, R.TEACHERS)
    sd = model.state_dict()
    keys = [k for k in sd if "pooler" not in k]
    assert sorted(keys) == sorted(params), (set(keys) ^ set(params))
    model.load_state_dict({k: v.clone() for k, v in params.items()}, strict=False)
    images = O.synth_images(R.B, seed=0)
    targets = O.synth_targets(R.B, R.TEACHERS, seed=1)
    fx = {"meta_backbone": np.array(R.BACKBONE), "meta_teachers": np.array(R.TEACHERS), "meta_B": np.array(R.B),
          "meta_hidden": np.array(R.HIDDEN), "meta_n_layer": np.array(R.N_LAYER),
          "sd_keys": np.array(keys), "sd_shapes": np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys])}
    model.train()
    pred = model(images)
    losses = model.get_loss(pred, targets)
    main_loss = 0.9 * losses["cos_loss"] + 0.1 * losses["l1_loss"]
    for ti, t in enumerate(R.TEACHERS):
        p = pred[t].detach().numpy().reshape(-1)
        pi = R.sample_idx(p.size, 128, 100 + ti)
        fx[f"pred{ti}_shape"] = np.array(pred[t].shape)
        fx[f"pred{ti}_idx"] = pi
        fx[f"pred{ti}_val"] = p[pi]
        fx[f"pred{ti}_abssum"] = np.array(np.abs(p.astype(np.float64)).sum())
    for k in ("mse_loss", "cos_loss", "l1_loss"):
        fx[k] = np.array(float(losses[k].detach()))
    fx["cos_pm"] = np.array([losses["cos_losses_per_model"][t] for t in R.TEACHERS])
    fx["l1_pm"] = np.array([losses["l1_losses_per_model"][t] for t in R.TEACHERS])
    fx["main_cos_l1"] = np.array(float(main_loss))
    main_loss.backward()
    named = dict(model.named_parameters())
    names = list(params)
    fx["grad_names"] = np.array(names)
    fx["gradnorm_cos_l1"] = np.array([float(named[k].grad.double().norm()) if named[k].grad is not None else 0.0 for k in names])
    out = R.GOLDEN
    np.savez_compressed(out, **fx)
    print(f"[gen_golden_mlp] wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
