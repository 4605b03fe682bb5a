#!/usr/bin/env python
"""precision="mxfp8" against bf16 (and fp8) on one GPU.

    python tools/mx8_bench.py [--gemm-only | --steps-only] [--reps 100] [--rounds 3] [--steps 10]

1. Isolated GEMMs, the five MX sites of DeiT-base at b = 128 (M = 25216): theia_gemm_nt_mx8 with and without the activation's quantise
   pass, against theia_gemm_nt on bf16 operands with the same epilogue.  HIP events around each launch, median of --reps after
   warm-up; the arms alternate launch by launch.
2. Train-step time (zero_grad, forward, losses, backward, fused AdamW) of DeiT-base + cddsv at b = 128 and DeiT-small + cddsv at b = 256
   in bf16 / fp8 / mxfp8, eager and captured (CapturedTrainStep; fp8: eager only, it is not capturable): --rounds rounds of --steps timed steps per arm, arms in turn.
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import theia_oracle as O  # noqa: E402
from theia_amd import _native as N, ops  # noqa: E402

M = 25216
SITES = [  # (name, N, K, epilogue)
    ("qkv fwd", 2304, 768, "bias"),
    ("fc1 fwd", 3072, 768, "gelu"),
    ("fc2 fwd", 768, 3072, "resid"),
    ("fc2 dgrad", 3072, 768, "dgelu"),
    ("fc1 dgrad", 768, 3072, "none"),
]


def _time(fns, reps, warm=10):
    """median microseconds of each callable, launches interleaved"""
    for f in fns:
        for _ in range(warm):
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ts[i].append((e0, e1))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 for a, b in t) for t in ts]


def gemms(reps):
    dev = torch.device("cuda:0")
    rows = []
    for name, Nn, K, epi in SITES:
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        w = (torch.randn(Nn, K, device=dev) * 0.05).to(torch.bfloat16)
        wq, ws = ops.quantize_mx8(w)
        xq, xs = ops.quantize_mx8(x)
        bias = torch.randn(Nn, device=dev)
        aux = torch.randn(M, Nn, device=dev).to(torch.bfloat16)
        out = torch.empty(M, Nn, dtype=torch.bfloat16, device=dev)
        kw = {"none": {}, "bias": dict(bias=bias), "gelu": dict(bias=bias, act=N.ACT_GELU, aux_out=aux),
              "resid": dict(bias=bias, resid=aux), "dgelu": dict(act=N.ACT_MUL_DGELU, aux_in=aux)}[epi]
        f_bf16 = lambda: ops.linear(x, w, out=out, **kw)  # noqa: E731
        f_mx = lambda: ops.linear_mx8(xq, xs, wq, ws, out=out, **kw)  # noqa: E731
        f_mxq = lambda: ops.linear_mx8(*ops.quantize_mx8(x, xq, xs), wq, ws, out=out, **kw)  # noqa: E731
        f_q = lambda: ops.quantize_mx8(x, xq, xs)  # noqa: E731
        t_bf16, t_mx, t_mxq, t_q = _time([f_bf16, f_mx, f_mxq, f_q], reps)
        fl = 2.0 * M * Nn * K
        rows.append(dict(site=name, shape=[M, Nn, K], epilogue=epi, bf16_us=round(t_bf16, 1), mx_us=round(t_mx, 1),
                         mx_with_quant_us=round(t_mxq, 1), quant_us=round(t_q, 1), bf16_pf=round(fl / t_bf16 / 1e9, 3),
                         mx_pf=round(fl / t_mx / 1e9, 3), speedup=round(t_bf16 / t_mx, 3), speedup_with_quant=round(t_bf16 / t_mxq, 3)))
        r = rows[-1]
        print(f"{name:10s} {M}x{Nn}x{K} {epi:6s} bf16 {r['bf16_us']:7.1f} us ({r['bf16_pf']:.2f} PF)  mx {r['mx_us']:7.1f} us "
              f"({r['mx_pf']:.2f} PF)  mx+quant {r['mx_with_quant_us']:7.1f} us  quant {r['quant_us']:6.1f} us  "
              f"x{r['speedup']:.2f} / x{r['speedup_with_quant']:.2f}", flush=True)
    return rows


def steps(rounds, nsteps, warmup):
    from theia_amd.foundation_models.common import get_model_feature_size
    from theia_amd.models.rvfm import RobotVisionFM
    from theia_amd.optimizers import FusedAdamW
    from theia_amd.train_graph import CapturedTrainStep, default_main_loss
    dev = torch.device("cuda:0")
    results = []
    for bb, B in (("facebook/deit-base-patch16-224", 128), ("facebook/deit-small-patch16-224", 256)):
        teachers = O.TEACHER_SETS["cddsv"]
        images = O.synth_images(B, 0).to(dev)
        targets = {t: v.to(dev) for t, v in O.synth_targets(B, teachers, 1).items()}
        arms = {}
        for prec in ("bf16", "fp8", "mxfp8"):
            for mode in ("eager", "captured") if prec != "fp8" else ("eager",):  # (CapturedTrainStep refuses the fp8 mode)
                m = RobotVisionFM(backbone=bb, translator="lconv", translator_kwargs={"hidden_size_factor": 1.0},
                                  target_feature_sizes={t: get_model_feature_size(t, keep_spatial=True) for t in teachers}, precision=prec)
                m.load_state_dict(O.synth_params(bb, teachers, 0))
                m = m.to(dev)
                opt = FusedAdamW(m, lr=1e-4)
                if mode == "captured":
                    cs = CapturedTrainStep(m, opt, warmup=2)
                    fn = (lambda cs=cs: cs(images, targets))
                else:
                    def fn(m=m, opt=opt):
                        opt.zero_grad(set_to_none=True)
                        default_main_loss(m.get_loss(m(images), targets, as_float=False)).backward()
                        opt.step()
                for _ in range(warmup):
                    fn()
                arms[(prec, mode)] = (fn, [])
        torch.cuda.synchronize()
        for _ in range(rounds):
            for key, (fn, ts) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(nsteps):
                    fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / nsteps)
        for (prec, mode), (_, ts) in arms.items():
            ms = statistics.median(ts)
            results.append(dict(backbone=bb, batch=B, precision=prec, mode=mode, ms_per_step=round(ms, 2)))
            print(f"{bb.split('/')[-1]:28s} b={B:3d} {prec:6s} {mode:8s} {ms:7.2f} ms/step  (rounds: {[round(t, 2) for t in ts]})", flush=True)
        del arms
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gemm-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {}
    if not a.steps_only:
        out["gemm"] = gemms(a.reps)
    if not a.gemm_only:
        out["steps"] = steps(a.rounds, a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
