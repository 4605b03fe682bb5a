#!/usr/bin/env python
"""Eager train-step time of the two translators on the same GPU, alternating arms.

    python tools/translator_bench.py [--backbone facebook/deit-base-patch16-224] [--batch 128] [--teachers cddsv]
                                     [--translator mlp lconv] [--rounds 5] [--steps 10] [--precision bf16]

One model per arm (synthetic weights, synthetic uint8 images and teacher features resident on the GPU); a step is zero_grad, forward,
losses, backward and the fused AdamW update (train_rvfm.py:116-131).  Every round runs --steps timed steps of each arm in turn after
warm-up steps, so drifts in clock or temperature hit both arms alike; prints the median ms/step per arm and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import theia_oracle as O  # noqa: E402
from theia_amd.foundation_models.common import get_model_feature_size  # noqa: E402
from theia_amd.models.rvfm import RobotVisionFM  # noqa: E402
from theia_amd.optimizers import FusedAdamW  # noqa: E402
from theia_amd.train_graph import default_main_loss  # noqa: E402

KWARGS = {"lconv": {"hidden_size_factor": 1.0}, "mlp": {"translator_hidden_size": 1024, "translator_n_layer": 3}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="facebook/deit-base-patch16-224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--teachers", default="cddsv")
    ap.add_argument("--translator", nargs="+", default=["mlp", "lconv"], choices=["mlp", "lconv"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp8"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    teachers = O.TEACHER_SETS[a.teachers]
    images = torch.randint(0, 256, (a.batch, 224, 224, 3), dtype=torch.uint8, device=dev)
    targets = {t: v.to(dev) for t, v in O.synth_targets(a.batch, teachers, 1).items()}
    arms = {}
    for kind in a.translator:
        m = RobotVisionFM(backbone=a.backbone, translator=kind, translator_kwargs=KWARGS[kind],
                          target_feature_sizes={t: get_model_feature_size(t, keep_spatial=True) for t in teachers},
                          precision=a.precision).to(dev)
        arms[kind] = (m, FusedAdamW(m, lr=1e-4, weight_decay=0.01))

    def step(kind):
        m, opt = arms[kind]
        opt.zero_grad(set_to_none=True)
        default_main_loss(m.get_loss(m(images), targets, as_float=False)).backward()
        opt.step()

    for kind in arms:
        for _ in range(a.warmup):
            step(kind)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for kind in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(kind)
            torch.cuda.synchronize()
            times[kind].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res = {k: round(statistics.median(v), 2) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:6s} {a.backbone.split('/')[-1]} + {a.teachers} b={a.batch} {a.precision}: {res[k]:.2f} ms/step "
              f"(rounds {', '.join(f'{x:.2f}' for x in v)})")
    print(json.dumps({"backbone": a.backbone, "teachers": a.teachers, "batch": a.batch, "precision": a.precision, "ms_per_step": res}))


if __name__ == "__main__":
    main()
