"""Training entry point for the MI355X hot path -- drop-in for the reference's ``scripts/train/train_rvfm.py``.

    torchrun --nproc_per_node=8 --nnodes 1 --rdzv_backend c10d --rdzv_endpoint 127.0.0.1:11111 \
        -m theia_amd.scripts.train.train_rvfm training/target_models=cddsv dataset=synthetic \
        model.backbone.backbone=facebook/deit-base-patch16-224 training.batch_size=128 precision=bf16

Same structure as the reference (train_rvfm.py: ``main`` :332-345 -> ``ddp_main`` :221-329 -> ``train`` :38-208), same
config tree / override syntax (Hydra is used when importable, otherwise ``theia_amd.utils.config.compose``), same
step order: batch -> forward -> get_loss -> main loss select -> zero_grad -> backward (gradient all-reduce over RCCL
overlapped with it) -> optional clip -> optimizer.step -> lr_scheduler.step -> log -> optional translator freeze ->
checkpoint (model-only state_dict on rank 0).

Deliberate differences (documented in DESIGN.md): one process per GPU with ``TheiaDataParallel`` instead of torch DDP;
loss scalars stay on the device and are read back every ``logging.log_interval`` steps instead of ~3T+7 blocking
``.item()`` per step; ``random_target_models > 0`` is rejected (in the reference it samples 2 teachers and would
dead-lock DDP with find_unused_parameters=False, train_rvfm.py:102-103); the webdataset reader is out of scope
 -- ``dataset=synthetic`` feeds synthetic batches of the right shapes.
"""
from __future__ import annotations

import math
import os
import os.path as osp
import sys
import time
from typing import Any, Iterator

import torch
import torch.distributed as dist
import torch.nn as nn

from theia_amd.foundation_models.common import MODEL_FEATURE_SIZES, get_model_feature_size
from theia_amd.models.rvfm import RobotVisionFM
from theia_amd.optimizers import FusedAdamW, param_groups_weight_decay
from theia_amd.parallel import TheiaDataParallel
from theia_amd.utils import config as cfglib
from theia_amd.utils.seed import seed_everything


class SyntheticFrames:
    """Infinite iterator of synthetic batches in the reference's batch format
    ({"image": uint8 [b,224,224,3], teacher: {"embedding": [b, HW, C]}}), generated on the device."""

    def __init__(self, batch_size: int, target_model_names, device, seed: int, fixed: bool = False, on_disk_format: bool = False):
        self.b, self.names, self.device = batch_size, list(target_model_names), device
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self.fixed, self._cached = fixed, None  # fixed: replay one batch (over-fitting sanity runs)
        # on_disk_format: synthesise the features as the extractor stores them (bf16 [C, H, W] per sample, host memory, with
        # per-channel statistics) and run them through the real ingest path (pinned staging -> H2D -> theia_feature_ingest_bf16)
        self.ingest = None
        if on_disk_format:
            from theia_amd.dataset import FeatureIngest
            cpu_gen = torch.Generator().manual_seed(seed + 1)
            means = {t: torch.randn(get_model_feature_size(t, keep_spatial=True)[0], generator=cpu_gen) * 0.1 for t in self.names}
            stds = {t: torch.rand(get_model_feature_size(t, keep_spatial=True)[0], generator=cpu_gen) + 0.5 for t in self.names}
            self.ingest = FeatureIngest(device, means, stds)
            self.cpu_gen = cpu_gen

    def __iter__(self) -> Iterator[dict]:
        return self

    def __next__(self) -> dict:
        if self.fixed and self._cached is not None:
            return self._cached
        batch: dict[str, Any] = {"image": torch.randint(0, 256, (self.b, 224, 224, 3), dtype=torch.uint8, device=self.device,
                                                        generator=self.gen)}
        spatial = [t for t in self.names if not t.endswith("_cls")]
        if self.ingest is not None:
            raw = {t: torch.randn((self.b,) + tuple(get_model_feature_size(t, keep_spatial=True)), generator=self.cpu_gen).to(torch.bfloat16)
                   for t in spatial}
            for t, emb in self.ingest(raw).items():
                batch[t] = {"embedding": emb}
        else:
            for t in spatial:
                C, H, W = get_model_feature_size(t, keep_spatial=True)
                batch[t] = {"embedding": torch.randn(self.b, H * W, C, device=self.device, generator=self.gen)}
        for t in self.names:  # "<teacher>_cls": the teacher's CLS token rides in the teacher's sample dict (data_utils.py:156-160)
            if t.endswith("_cls"):
                Ct = get_model_feature_size(t[:-4], keep_spatial=True)[0]
                batch.setdefault(t[:-4], {})["cls"] = torch.randn(self.b, Ct, device=self.device, generator=self.gen)
        self._cached = batch if self.fixed else None
        return batch


def _targets_of(batch: dict, names) -> dict:
    """train_rvfm.py:107-114: "<teacher>_cls" targets are the teacher's CLS token, everything else its spatial embedding."""
    return {t: (batch[t[:-4]]["cls"] if t.endswith("_cls") else batch[t]["embedding"]).float() for t in names}


def select_main_loss(losses: dict, main_loss: str | None):
    """train_rvfm.py:119-122"""
    if main_loss == "mse" or main_loss is None:
        return losses["mse_loss"]
    if main_loss == "cos_l1":
        return 0.9 * losses["cos_loss"] + 0.1 * losses["l1_loss"]
    raise ValueError(f"unknown training.main_loss '{main_loss}'")


def train(rvfm: nn.Module, target_model_names, optimizer, lr_scheduler, train_iter, eval_iter, cfg, device: int = 0,
          train_epoch_steps: int = 0, eval_epoch_steps: int = 0, total_train_steps: int = 0, warmup_steps: int = 0) -> dict:
    rank = dist.get_rank() if dist.is_initialized() else 0
    log_interval = int(cfg.logging.get("log_interval", 10))
    steps = 0
    history = {"train_main_loss": [], "eval_main_loss": []}
    # training.capture_step=true (no reference equivalent): the loop body below -- forward, get_loss, backward, clipping, optimizer.step --
    # runs as ONE hipGraph replay per step, or, under torchrun with world size > 1, as two replays around the eager gradient-bucket
    # exchange (theia_amd/train_graph.py); it pays where the eager loop is host-bound, i.e. at the reference's default per-GPU batch
    # of 16 (configs/training/frame_level.yaml:8)
    captured = None
    if cfg.training.get("capture_step", False):
        if not isinstance(optimizer, FusedAdamW):
            raise NotImplementedError("training.capture_step needs the fused optimizer")
        from theia_amd.train_graph import CapturedTrainStep
        multi = dist.is_initialized() and dist.get_world_size() > 1
        captured = CapturedTrainStep(rvfm if multi else rvfm.module, optimizer, main_loss=lambda l: select_main_loss(l, cfg.training.main_loss),
                                     warmup=2)
    for ep in range(cfg.training.epochs):
        rvfm.train()
        t0 = time.time()
        for _ in range(train_epoch_steps):
            batch = next(train_iter)
            images_batch = batch["image"]
            if cfg.training.random_target_models > 0:
                raise NotImplementedError("random_target_models > 0 is not supported (breaks data-parallel reduction in the reference too)")
            target_features_batch = _targets_of(batch, target_model_names)
            max_norm = None
            if cfg.training.grad_clip:
                max_norm = cfg.training.grad_clip_norm_warmup if steps < warmup_steps else cfg.training.grad_clip_norm
            if captured is not None:
                captured.set_grad_clip(max_norm)
                main_loss = captured(images_batch, target_features_batch)["main_loss"]
            else:
                pred = rvfm(images_batch)
                losses = rvfm.module.get_loss(pred, target_features_batch, as_float=False)
                main_loss = select_main_loss(losses, cfg.training.main_loss)
                optimizer.zero_grad()
                main_loss.backward()
                if max_norm is not None:
                    if isinstance(optimizer, FusedAdamW):  # global norm + clip factor on the device, applied inside the AdamW kernel
                        optimizer.clip_grad_norm_(max_norm)
                    else:
                        nn.utils.clip_grad_norm_(rvfm.parameters(), max_norm)
                optimizer.step()
            if lr_scheduler is not None:
                lr_scheduler.step()
            steps += 1
            if rank == 0 and steps % log_interval == 0:
                ml = float(main_loss.detach())
                history["train_main_loss"].append((steps, ml))
                print(f"[train] ep {ep} step {steps}/{total_train_steps} main_loss {ml:.5f} "
                      f"({(time.time() - t0) / max(1, steps % train_epoch_steps or train_epoch_steps) * 1e3:.1f} ms/step)", flush=True)
            if cfg.training.freeze_translator and steps == int(cfg.training.freeze_translator_start_steps_ratio * total_train_steps):
                rvfm.module.freeze_translator()
                if captured is not None:
                    captured.invalidate()
            if steps % cfg.logging.save_ckpt_interval == 0 and rank == 0:
                save_checkpoint(rvfm.module, cfg, steps)
        if dist.is_initialized():
            dist.barrier()
        rvfm.eval()
        with torch.no_grad():
            acc, n = 0.0, 0
            for _ in range(eval_epoch_steps):
                batch = next(eval_iter)
                target_features_batch = _targets_of(batch, target_model_names)
                pred = rvfm(batch["image"])
                losses = rvfm.module.get_loss(pred, target_features_batch, as_float=False)
                acc += float(select_main_loss(losses, cfg.training.main_loss))
                n += 1
            if rank == 0 and n:
                history["eval_main_loss"].append((steps, acc / n))
                print(f"[eval] ep {ep} main_loss {acc / n:.5f}", flush=True)
        if rank == 0:
            save_checkpoint(rvfm.module, cfg, steps)
        if dist.is_initialized():
            dist.barrier()
    return history


def save_checkpoint(model: nn.Module, cfg, steps: int) -> str:
    """Model-only state_dict, reference file naming (train_rvfm.py:153-156)."""
    os.makedirs(cfg.logging.model_path, exist_ok=True)
    path = osp.join(cfg.logging.model_path, f"{cfg.logging.run_identifier_prefix}_step{steps:08d}.pth")
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, path)
    return path


def ddp_setup() -> None:
    if "RANK" in os.environ and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from theia_amd.parallel import configure_rccl_env
        configure_rccl_env()
        dist.init_process_group("nccl")  # RCCL on ROCm


def ddp_cleanup() -> None:
    if dist.is_initialized():
        dist.destroy_process_group()


def ddp_main(cfg) -> dict:
    ddp_setup()
    rank = dist.get_rank() if dist.is_initialized() else 0
    world_size = dist.get_world_size() if dist.is_initialized() else 1
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    names = cfg.training.target_models.target_model_names
    target_model_names = list(names) if len(names) > 0 else list(MODEL_FEATURE_SIZES.keys())
    target_model_names = [t for t in target_model_names if "llava" not in t]
    target_feature_sizes = {t: get_model_feature_size(t, keep_spatial=True) for t in target_model_names}
    if cfg.training.get("distill_cls", False):  # train_rvfm.py:238-246: CLS-token heads for the ViT / DINOv2 / CLIP teachers
        for t in list(target_model_names):
            if "google/vit" in t or "facebook/dino" in t or "openai/clip" in t:
                target_feature_sizes[t + "_cls"] = get_model_feature_size(t, keep_spatial=True)[:1]
                target_model_names.append(t + "_cls")

    translator_kwargs = dict(cfg.model.translator.kwargs)
    if cfg.model.translator.type == "mlp" and "hidden_size" in translator_kwargs:
        # the reference's configs/model/translator/mlp.yaml names the width `hidden_size`, which MLPFeatureTranslator
        # (models/feature_translators.py:91-103) does not take: its own config fails with a TypeError.  Renamed here only.
        translator_kwargs["translator_hidden_size"] = translator_kwargs.pop("hidden_size")
    rvfm = RobotVisionFM(translator=cfg.model.translator.type, translator_kwargs=translator_kwargs,
                         target_feature_sizes=target_feature_sizes,
                         target_loss_weights=cfg.training.target_models.target_model_weights,
                         precision=cfg.get("precision", None), **cfg.model.backbone)
    rvfm.to(device)
    rvfm_ddp = TheiaDataParallel(rvfm)

    if "synthetic" not in cfg.dataset.dataset_mix:
        raise NotImplementedError("the webdataset shard reader is outside the accelerated hot path; run with dataset=synthetic "
                                  "or feed batches in the reference format to train()")
    train_epoch_steps = int(cfg.dataset.get("train_steps_per_epoch", 20))
    eval_epoch_steps = int(cfg.dataset.get("eval_steps_per_epoch", 2))
    fixed = bool(cfg.dataset.get("fixed_batch", False))
    on_disk = bool(cfg.dataset.get("feature_norm", False))  # dataset.feature_norm=true: features arrive as stored + statistics
    train_iter = SyntheticFrames(cfg.training.batch_size, target_model_names, device, cfg.seed + rank * 100, fixed, on_disk)
    eval_iter = SyntheticFrames(cfg.training.batch_size, target_model_names, device, cfg.seed + (rank * 100 if fixed else 7777), fixed, on_disk)
    total_train_steps = train_epoch_steps * cfg.training.epochs

    lr = cfg.training.base_lr * ((cfg.training.batch_size * world_size) / (cfg.training.base_batch_size * cfg.training.base_world_size))
    if cfg.training.optimizer.get("_target_", "") in ("torch.optim.AdamW", "theia_amd.optimizers.FusedAdamW"):
        # same update rule as torch.optim.AdamW, fused over the engine's flat buckets (2 HIP launches per bucket); it is a
        # torch.optim.Optimizer, so the configured LR scheduler (constant or cosine warm restarts, both behind a linear
        # warm-up: lr_schedulers.py:8-77) drives it exactly as in the reference
        optimizer = FusedAdamW(rvfm_ddp, lr=lr, betas=tuple(cfg.training.optimizer.get("betas", (0.9, 0.999))),
                               weight_decay=cfg.training.weight_decay)
    else:
        groups = param_groups_weight_decay(rvfm_ddp, cfg.training.weight_decay)
        optimizer = cfglib.instantiate(cfg.training.optimizer, groups, lr=lr)
    warm_up_steps = int(cfg.training.warm_up_steps_ratio * total_train_steps)
    sched_kwargs = dict(optimizer=optimizer, warm_up_steps=warm_up_steps)
    if "get_cos_lrs" in cfg.training.lr_scheduler.get("_target_", ""):
        sched_kwargs["cos_lrs_T_0"] = int(total_train_steps * (1 - cfg.training.warm_up_steps_ratio))
    lr_scheduler = cfglib.instantiate(cfg.training.lr_scheduler, **sched_kwargs)
    if rank == 0:
        print(cfglib.to_yaml(cfg), flush=True)
    history = train(rvfm_ddp, target_model_names, optimizer, lr_scheduler, train_iter, eval_iter, cfg=cfg, device=local_rank,
                    train_epoch_steps=train_epoch_steps, eval_epoch_steps=eval_epoch_steps, total_train_steps=total_train_steps,
                    warmup_steps=int(cfg.training.warm_up_steps_ratio * total_train_steps))
    ddp_cleanup()
    return history


def main(argv=None) -> dict:
    argv = list(sys.argv[1:] if argv is None else argv)
    config_path = None
    if "--config-path" in argv:
        i = argv.index("--config-path")
        config_path = argv[i + 1]
        del argv[i:i + 2]
    cfg = cfglib.compose(argv, config_path=config_path)
    backbone_fn = f"_{cfg.model.backbone.backbone.replace('/', '-')}"
    notes_fn = f"_{cfg.logging.notes}" if cfg.logging.notes else ""
    translator_fn = f"_{cfg.model.translator.type}"
    pretrained_fn = "_pretrained" if cfg.model.backbone.pretrained else ""
    dp_fn = f"_dp{cfg.dataset.dataset_ratio:.3f}"
    cfg.logging.run_identifier_prefix = f"rvfm{dp_fn}{backbone_fn}{translator_fn}{pretrained_fn}{notes_fn}"
    seed_everything(cfg.seed)
    return ddp_main(cfg)


if __name__ == "__main__":
    main()
