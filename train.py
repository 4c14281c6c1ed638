#!/usr/bin/env python3
"""Training script (drop-in for the reference's train.py: same flags, same checkpoint dict).

    python train.py --data_root data/coco/ --batch_size 64 --epochs 210 --lr 5e-4 [--resume ckpt.pth] [--config hrformer_small]
    torchrun --nproc-per-node 8 train.py ...          # data parallel, one process per GPU (RCCL)

Differences from the reference loop (train.py:131-228): no per-step `loss.item()` host sync (losses are read back only at the
log interval), bf16 instead of fp16+GradScaler, fused AdamW over a flat parameter buffer, optional hipGraph replay
(`--graph`), GradScaler's "drop the step when a gradient is inf/NaN" and gradient-norm clipping as an opt-in device-side guard
(`--skip_nonfinite`, `--clip_grad_norm X`), colour jitter on the device (`--color_jitter B C S`, or DATA.COLOR_JITTER of a legacy
yaml), blur, sensor noise and rectangle erasing of the crops on the device (`--blur`, `--noise`, `--occlusion`, or DATA.BLUR / NOISE /
OCCLUSION of a legacy yaml; labels stay), and an exponential moving average of the weights kept by the optimiser kernel (`--ema DECAY`): validation inside the loop then
scores the averaged weights, and checkpoints carry them as "ema_state_dict" (validate.py / inference.py `--ema` load them), and online
hard keypoint mining (`--ohkm TOPK [--ohkm_weight W]`, or LOSS.USE_OHKM / TOPK of a legacy yaml): per sample only the TOPK worst-fitted
joints count in the heatmap loss, selected on the device inside the step; every validation interval logs which joints were selected, and
per-tensor diagnostics reduced on the device (`--tensor_stats K`: at every log interval the K tensors with the largest gradient norm and
with the smallest / largest update-to-weight ratio; `--trace_nonfinite`: which tensors held inf / NaN when a step's gradients did).  With POSE_SYNTHETIC=1 the loader yields device-resident synthetic batches (no COCO on disk needed; they are not jittered).
"""
import argparse
import contextlib
import copy
import logging
import os
import sys
import time
from datetime import datetime, timedelta

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from infantposeestimation_gaussianbias_amd import engine  # noqa: E402
from infantposeestimation_gaussianbias_amd.configs import get_config  # noqa: E402
from infantposeestimation_gaussianbias_amd.datasets import build_dataloader  # noqa: E402
from infantposeestimation_gaussianbias_amd.models import build_model  # noqa: E402
from infantposeestimation_gaussianbias_amd.utils import AverageMeter  # noqa: E402


def set_seed(seed: int):
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def save_checkpoint(model, trainer, epoch, metrics, output_dir, is_best=False):
    """Same dict as the reference (train.py:351-357); optimizer state is exported in torch.optim.AdamW's format.  With the weight EMA on,
    and only then, two more keys: the averaged weights as a model state dict, and the decay."""
    os.makedirs(output_dir, exist_ok=True)
    ckpt = {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": trainer.opt.state_dict(),
            "scheduler_state_dict": trainer.sched.state_dict(), "metrics": metrics}
    if trainer.opt.ema is not None:
        ckpt["ema_state_dict"], ckpt["ema_decay"] = trainer.opt.ema_state_dict(), trainer.opt.ema_decay
    torch.save(ckpt, os.path.join(output_dir, "latest.pth"))
    if is_best:
        torch.save(ckpt, os.path.join(output_dir, "best.pth"))
    if epoch % 10 == 0:
        torch.save(ckpt, os.path.join(output_dir, f"epoch_{epoch}.pth"))


def tensor_stats_report(opt, k, grad_scale=1.0):
    """Three log lines from the flat buffers as the last step left them (which ran with snapshot=True): the k tensors with the largest
    gradient norm, and the k with the smallest and the largest update-to-weight ratio.  Three statistics calls, three device reads."""
    grad = opt.tensor_stats("grad", scale=grad_scale)
    ratio = engine.update_to_weight_ratio(opt.tensor_stats("update"), opt.tensor_stats("param"))
    by_norm = sorted((n for n, v in grad.items() if v["numel"]), key=lambda n: -grad[n]["norm"])[:k]
    by_ratio = sorted((n for n, r in ratio.items() if r == r and grad[n]["numel"]), key=lambda n: ratio[n])
    return ["largest grad norm: " + ", ".join(f"{n} {grad[n]['norm']:.3g}" for n in by_norm),
            "smallest update/weight: " + ", ".join(f"{n} {ratio[n]:.3g}" for n in by_ratio[:k]),
            "largest update/weight: " + ", ".join(f"{n} {ratio[n]:.3g}" for n in by_ratio[::-1][:k])]


def nonfinite_report(opt, seen):
    """(line or None, events so far): one line when steps with non-finite gradients happened since `seen` events."""
    tr = opt.nonfinite_trace()
    if tr is None or tr["events"] <= seen:
        return None, seen
    return (f"non-finite gradients in {tr['events'] - seen} step(s) since the last report; latest: {len(tr['tensors'])} tensors, nearest "
            f"the loss: {tr['last']} ({tr['tensors'][tr['last']]} elements)"), tr["events"]


def train_one_epoch(trainer, loader, epoch, cfg, logger, rank, tensor_stats=0, trace_state=None):
    loss_meter, batch_time = AverageMeter("Loss", ":.4f"), AverageMeter("Time", ":.3f")
    n = len(loader)
    log_interval = max(1, n // 10)
    end = time.time()
    for i, batch in enumerate(loader):
        dev = next(trainer.model.parameters()).device
        batch = {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
        logged = i % log_interval == 0 or i == n - 1
        out = trainer.step(batch, snapshot=bool(tensor_stats) and logged and rank == 0)      # the copy is taken on log steps only
        if logged:          # the only host syncs of the epoch
            loss_meter.update(float(out["loss"].detach()), batch["img"].size(0))
            batch_time.update((time.time() - end) / (log_interval if i else 1))
            end = time.time()
            if rank == 0:
                msg = (f"Epoch [{epoch}][{i}/{n}] Loss: {loss_meter.val:.4f} ({loss_meter.avg:.4f}) "
                       f"LR: {trainer.opt.lr:.6f} Time: {batch_time.val:.3f}s")
                if "losses" in out:
                    msg += " | " + ", ".join(f"{k}: {float(v.detach()):.4f}" for k, v in out["losses"].items() if k != "total_loss")
                if trainer.opt.guarded:
                    gs = trainer.opt.guard_stats()
                    msg += f" | grad_norm: {gs['grad_norm']:.4g} clip_coef: {gs['clip_coef']:.4g} skipped_steps: {gs['skipped_steps']}"
                logger.info(msg)
                if tensor_stats:
                    for line in tensor_stats_report(trainer.opt, tensor_stats, trainer.comm.grad_scale):
                        logger.info(f"Epoch [{epoch}][{i}/{n}] {line}")
                if trace_state is not None:
                    line, trace_state["events"] = nonfinite_report(trainer.opt, trace_state["events"])
                    if line:
                        logger.info(f"Epoch [{epoch}][{i}/{n}] {line}")
    return loss_meter.avg


def selection_report(model, names):
    """'joint share%' of the mining loss's selections since the last report, hardest first (and the counts start again); None while mining
    is off or nothing was selected."""
    counts = model.selection_counts(reset=True)
    if counts is None or counts.sum() == 0:
        return None
    share = counts / counts.sum()
    names = list(names) if len(names) == len(counts) else [f"kpt_{i}" for i in range(len(counts))]
    return ", ".join(f"{names[i]} {100 * share[i]:.1f}%" for i in np.argsort(-share, kind="stable"))


def parse_fill(text):
    """--occlusion_fill: 'random', 'mean' or 'R,G,B'."""
    if text in ("random", "mean"):
        return text
    try:
        return tuple(int(v) for v in text.split(","))
    except ValueError:
        return text          # check_augment refuses it and names the flag


def apply_augment_flags(cfg, args):
    """--blur / --noise / --occlusion (+ --occlusion_area, --occlusion_fill) onto cfg.train.blur / sensor_noise / occlusion, over what a
    yaml set.  A flag gives the probability and the upper end of the range; the lower end is the default's, or the upper end where that is
    smaller.  PROB 0 turns the stage off.  ValueError (naming the flag) for a value `check_augment` refuses."""
    from infantposeestimation_gaussianbias_amd.configs.config import AUGMENT_DEFAULTS, check_augment
    for flag, kind, attr in (("blur", "blur", "blur"), ("noise", "noise", "sensor_noise")):
        v = getattr(args, flag)
        if v is not None:
            lo = min(AUGMENT_DEFAULTS[kind]["sigma"][0], v[1])
            setattr(cfg.train, attr, check_augment(kind, {"prob": v[0], "sigma": (lo, v[1])}, f"--{flag}"))
    if args.occlusion is not None:
        n = args.occlusion[1]
        cfg.train.occlusion = check_augment("occlusion", {**(cfg.train.occlusion or {}), "prob": args.occlusion[0],
                                                          "max_rects": int(n) if float(n).is_integer() else n}, "--occlusion")
    for flag, key, value in (("occlusion_area", "area", args.occlusion_area),
                             ("occlusion_fill", "fill", parse_fill(args.occlusion_fill) if args.occlusion_fill is not None else None)):
        if value is not None:
            if cfg.train.occlusion is None:
                raise ValueError(f"--{flag} needs --occlusion PROB MAX_RECTS (or a DATA.OCCLUSION block) with PROB > 0")
            cfg.train.occlusion = check_augment("occlusion", {**cfg.train.occlusion, key: tuple(value) if key == "area" else value},
                                                f"--{flag}")


def main(args):
    cfg = get_config(args.config) if args.config else get_config()
    if args.data_root:
        cfg.data.data_root = args.data_root
    if args.batch_size:
        cfg.train.batch_size = args.batch_size
    if args.epochs:
        cfg.train.max_epochs = args.epochs
    if args.lr:
        cfg.train.lr = args.lr
    if args.color_jitter is not None:
        cfg.train.color_jitter = tuple(args.color_jitter)
    if args.color_jitter_prob is not None:
        cfg.train.color_jitter_prob = args.color_jitter_prob
    apply_augment_flags(cfg, args)
    if args.ema is not None:
        cfg.train.ema_decay = args.ema
    if args.ohkm is not None:
        cfg.model.ohkm_topk = args.ohkm
    if args.ohkm_weight is not None:
        cfg.model.ohkm_weight = args.ohkm_weight
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    logger = logging.getLogger("train")
    set_seed(cfg.seed + rank)
    out_dir = os.path.join(cfg.train.checkpoint_dir, f"{cfg.exp_name}_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    loader = build_dataloader(cfg, is_train=True)
    model = build_model(cfg).to(torch.device("cuda", local))
    trainer = engine.Trainer(model, cfg, iters_per_epoch=len(loader), use_graph=args.graph, graph_streams=args.graph,
                             clip_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite, ema_decay=cfg.train.ema_decay or 0.0,
                             trace_nonfinite=args.trace_nonfinite)
    trace_state = {"events": 0} if args.trace_nonfinite else None
    start_epoch, best_ap = 0, 0.0
    if args.resume and os.path.isfile(args.resume):
        ckpt = torch.load(args.resume, map_location="cpu", weights_only=True)
        model.load_state_dict(ckpt["model_state_dict"])
        trainer.opt.load_state_dict(ckpt["optimizer_state_dict"])
        trainer.sched.load_state_dict(ckpt["scheduler_state_dict"])
        if trainer.opt.ema is not None:
            # load_state_dict above rewrote the masters through the parameter views: the average taken at construction is stale
            if "ema_state_dict" in ckpt:
                trainer.opt.load_ema_state_dict(ckpt["ema_state_dict"])
            else:
                trainer.opt.reset_ema()
                logger.info("Checkpoint has no ema_state_dict: the weight EMA restarts from the loaded weights")
        start_epoch, best_ap = ckpt["epoch"] + 1, ckpt.get("metrics", {}).get("AP", 0.0)
        logger.info(f"Resumed from epoch {start_epoch}")
    val_loader = None
    for epoch in range(start_epoch, cfg.train.max_epochs):
        loss = train_one_epoch(trainer, loader, epoch, cfg, logger, rank, tensor_stats=args.tensor_stats, trace_state=trace_state)
        if rank == 0 and cfg.model.ohkm_topk and ((epoch + 1) % cfg.train.val_interval == 0 or epoch == cfg.train.max_epochs - 1):
            report = selection_report(model, cfg.data.keypoint_names)      # which joints are the hard ones
            if report:
                logger.info(f"Epoch [{epoch}] hard keypoint selections (top {cfg.model.ohkm_topk}): {report}")
        if rank == 0 and ((epoch + 1) % cfg.train.val_interval == 0 or epoch == cfg.train.max_epochs - 1):
            # validation inside the training loop (train.py:231-325, 437-452 of the reference): AP decides `best.pth`
            from validate import validate
            if val_loader is None:
                val_cfg = copy.copy(cfg)
                val_cfg.test_scales = None           # this monitor stays single-scale and un-flipped; validate.py runs the multi-scale test
                val_loader = build_dataloader(val_cfg, is_train=False)
            # the heatmap decode follows the config (cfg.decode / cfg.modulate_kernel); a config that names none keeps the quarter-pixel shift
            # with the weight EMA on, the averaged weights are the ones scored (and so the ones that pick best.pth)
            with trainer.ema_weights() if trainer.opt.ema is not None else contextlib.nullcontext():
                metrics, _ = validate(model, val_loader, torch.device("cuda", local), cfg, logger, flip_test=False)
            model.train()
            is_best = metrics["AP"] > best_ap
            best_ap = max(best_ap, metrics["AP"])
            save_checkpoint(model, trainer, epoch, dict({k: float(v) for k, v in metrics.items()}, train_loss=float(loss)), out_dir, is_best=is_best)
        if world > 1 and ((epoch + 1) % cfg.train.val_interval == 0 or epoch == cfg.train.max_epochs - 1):
            # The other ranks wait for rank 0's validation on the HOST (a key in the rendezvous store), not inside a collective: a
            # dist.barrier() or the next epoch's first all-reduce would sit enqueued for the whole validation and trip the RCCL
            # watchdog timeout.  Unverified on hardware until a >= 2-GPU run exists (SCALE has been skipped so far).
            store = dist.distributed_c10d._get_default_store()
            key = f"pose/validated/{epoch}"
            if rank == 0:
                store.set(key, "1")
            else:
                store.wait([key], timedelta(hours=12))
    if world > 1:
        dist.destroy_process_group()


def build_parser():
    p = argparse.ArgumentParser(description="Train Pose Estimation Model")
    p.add_argument("--data_root", type=str, default=None)
    p.add_argument("--batch_size", type=int, default=None)
    p.add_argument("--epochs", type=int, default=None)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--config", type=str, default=None, help="preset name or legacy yaml (extension over the reference)")
    p.add_argument("--graph", action="store_true", help="replay the step as a captured hipGraph")
    p.add_argument("--color_jitter", type=float, nargs=3, default=None, metavar=("B", "C", "S"),
                   help="brightness / contrast / saturation ranges of the colour jitter applied to training crops on the device")
    p.add_argument("--color_jitter_prob", type=float, default=None, help="share of the samples that are jittered (default 0.5)")
    p.add_argument("--blur", type=float, nargs=2, default=None, metavar=("PROB", "SIGMA_MAX"),
                   help="Gaussian blur of a share PROB of the training crops on the device, sigma up to SIGMA_MAX <= 2.5 pixels")
    p.add_argument("--noise", type=float, nargs=2, default=None, metavar=("PROB", "SIGMA_MAX"),
                   help="additive sensor noise on a share PROB of the training crops, standard deviation up to SIGMA_MAX <= 73 grey levels")
    p.add_argument("--occlusion", type=float, nargs=2, default=None, metavar=("PROB", "MAX_RECTS"),
                   help="erase 1 to MAX_RECTS <= 4 random rectangles in a share PROB of the training crops (labels stay)")
    p.add_argument("--occlusion_area", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="area of one erased rectangle as a fraction of the crop (default 0.02 0.2)")
    p.add_argument("--occlusion_fill", type=str, default=None, metavar="random|mean|R,G,B",
                   help="what the erased rectangles hold: random bytes (default), the ImageNet mean, or one colour")
    p.add_argument("--clip_grad_norm", type=float, default=0.0, metavar="X",
                   help="clip the global gradient norm to X on the device (torch.nn.utils.clip_grad_norm_; 0 = off); implies --skip_nonfinite")
    p.add_argument("--skip_nonfinite", action="store_true",
                   help="drop the whole optimiser step when a gradient is inf or NaN (what GradScaler.step does in the reference)")
    p.add_argument("--ema", type=float, default=None, metavar="DECAY",
                   help="keep an exponential moving average of the weights in the optimiser kernel (e.g. 0.9998; warm-up "
                        "min(DECAY, (1+t)/(10+t))); validation and best.pth use the averaged weights (default: off)")
    p.add_argument("--ohkm", type=int, default=None, metavar="TOPK",
                   help="online hard keypoint mining: per sample only the TOPK joints with the largest heatmap error count (the fusion "
                        "loss gains the term ohkm_loss; the heatmap head's loss becomes the mined one; default: off)")
    p.add_argument("--ohkm_weight", type=float, default=None, metavar="W", help="weight of ohkm_loss in the fusion loss (default 1.0)")
    p.add_argument("--tensor_stats", type=int, default=0, metavar="K",
                   help="at every log interval log the K tensors with the largest gradient norm and the K with the smallest / largest "
                        "update-to-weight ratio, reduced per tensor on the device (0 = off)")
    p.add_argument("--trace_nonfinite", action="store_true",
                   help="record on the device which tensors held inf / NaN gradients; logged at the log interval when it happened")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
