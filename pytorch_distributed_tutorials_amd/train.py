"""Trainer: the reference ``resnet/main.py`` behaviour on the MI355X framework.

    torchrun --nproc_per_node=8 -m pytorch_distributed_tutorials_amd.train [flags]
    python -m pytorch_distributed_tutorials_amd.launch --nproc_per_node=8 [flags]

Flags and defaults follow the reference (``resnet/main.py:42-59``),
with its defects fixed: ``--local_rank`` and ``--local-rank`` and the
``LOCAL_RANK`` env var are all accepted (D5), ``--learning_rate`` is a float (D4),
the default checkpoint name exists (D2), the sampler is re-seeded every epoch
(D6), evaluation uses no augmentation (D7), the device is bound before the
process group comes up (D9), resume also restores optimizer state and epoch
through a sidecar file (D10), and the process group is torn down at exit (D12).

Behaviour kept: per-process batch 256, SGD(momentum 0.9, wd 1e-5),
CrossEntropyLoss(mean), DistributedSampler sharding, rank-0 evaluation +
checkpoint every 10 epochs *before* training that epoch, test batch 128, the
stdout lines of ``resnet/main.py:107,113-115``.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .data import (AugConfig, CenterCropResize, DeviceLoader, DistributedSampler, MixConfig, RandomResizedCrop,
                   build_dataset)
from .models import build_model
from .optim import LARS, SGD, ModelEma, WarmupPolyLR
from .parallel import DistributedDataParallel, destroy, init_distributed
from .parallel.comm import CommOptions
from .utils.checkpoint import load_checkpoint, save_checkpoint
from .utils import trace
from .utils.metrics import StepTimer
from .utils.seed import set_random_seeds
from .utils.watchdog import FaultInjector, Watchdog

DEFAULTS = {
    "num_epochs": 10000,
    "batch_size": 256,
    "lr": 0.01,
    "seed": 0,
    "model_dir": "saved_models",
    "model_filename": "resnet_distributed.pth",
}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--local_rank", "--local-rank", dest="local_rank", type=int, default=None,
                   help="Local rank (torch.distributed.launch); falls back to $LOCAL_RANK")
    p.add_argument("--num_epochs", type=int, default=DEFAULTS["num_epochs"], help="Number of training epochs")
    p.add_argument("--batch-size", "--batch_size", dest="batch_size", type=int,
                   default=DEFAULTS["batch_size"], help="Training batch size (per process)")
    p.add_argument("--learning_rate", "--learning-rate", dest="learning_rate", type=float,
                   default=DEFAULTS["lr"], help="Learning rate")
    p.add_argument("--seed", type=int, default=DEFAULTS["seed"], help="Random seed for training")
    p.add_argument("--model_dir", type=str, default=DEFAULTS["model_dir"],
                   help="Model directory to store saved models")
    p.add_argument("--model_filename", type=str, default=DEFAULTS["model_filename"],
                   help="Model filename to be saved")
    p.add_argument("--resume", action="store_true", help="Resume training from saved checkpoint.")
    # ---- framework extensions
    p.add_argument("--arch", default="resnet18", choices=["resnet18", "resnet34", "resnet50",
                                                          "resnet101", "resnet152"])
    p.add_argument("--num-classes", type=int, default=1000,
                   help="fc outputs (the reference keeps torchvision's 1000)")
    p.add_argument("--impl", default="auto", choices=["auto", "native", "torch"],
                   help="native = MI355X HIP kernels (GPU); torch = stock ATen ops")
    p.add_argument("--data", default="cifar10",
                   choices=["cifar10", "synthetic-cifar", "synthetic-imagenet", "learnable-cifar", "array"],
                   help="array = --data-root/{train,val}_images.npy (uint8 [N,3,H,W]) + {train,val}_labels.npy")
    p.add_argument("--data-root", default="data")
    p.add_argument("--synthetic-samples", type=int, default=None)
    p.add_argument("--backend", default=None, choices=[None, "nccl", "gloo"])
    p.add_argument("--bucket-mb", type=float, default=25.0)
    p.add_argument("--wire-dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--eval-every", type=int, default=10)
    p.add_argument("--max-steps-per-epoch", type=int, default=None)
    p.add_argument("--timeout", type=float, default=None, help="collective timeout (s)")
    p.add_argument("--log-every", type=int, default=0, help="print img/s every N steps (0 = off)")
    p.add_argument("--dtype", default="auto", choices=["auto", "bf16", "fp32", "fp8"],
                   help="compute dtype: native kernels are bf16 (fp32 master weights), or fp8 convs "
                        "(e4m3 forward / e5m2 input gradients, delayed scaling); the torch path runs "
                        "fp32 (reference) or bf16 autocast; auto = bf16 native / fp32 torch")
    p.add_argument("--steps", type=int, default=None, help="stop after this many training steps in total")
    p.add_argument("--trace", action="store_true",
                   help="emit roctx ranges (fwd/bwd/step/eval) for rocprofv3 --marker-trace")
    p.add_argument("--watchdog-timeout", type=float, default=None,
                   help="abort this rank when it makes no progress for N seconds (default: 900 when "
                        "world_size > 1, off for a single process; 0 = off)")
    p.add_argument("--deterministic", action=argparse.BooleanOptionalAction, default=True,
                   help="bitwise-reproducible kernels (reference sets cudnn.deterministic=True); "
                        "--no-deterministic enables atomic split-K weight gradients")
    p.add_argument("--graph", action="store_true",
                   help="native impl on a GPU: capture the whole training step (forward, backward with "
                        "the bucketed all-reduces, SGD) in a HIP graph once and replay it for every "
                        "full-size batch; the launch-bound ResNet-18/CIFAR step gains the most")
    # ---- large-batch recipe (the defaults are the reference's plain SGD at a constant rate)
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "lars"],
                   help="lars = layer-wise trust ratios on top of SGD with momentum (optim.LARS)")
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--weight-decay", type=float, default=1e-5)
    p.add_argument("--trust-coefficient", type=float, default=1e-3, help="LARS eta")
    p.add_argument("--lars-eps", type=float, default=1e-8)
    p.add_argument("--lars-adapt-1d", action="store_true",
                   help="LARS: also decay and adapt BatchNorm parameters and biases (exclude_1d off)")
    p.add_argument("--label-smoothing", type=float, default=0.0)
    p.add_argument("--lr-schedule", default="constant", choices=["constant", "warmup-poly"],
                   help="warmup-poly: linear warm-up over --warmup-epochs to --learning_rate, then "
                        "polynomial (power 2) decay to --lr-end at the end of --num_epochs")
    p.add_argument("--warmup-epochs", type=float, default=5.0)
    p.add_argument("--lr-end", type=float, default=0.0)
    # ---- input-side regularisers (off by default): per-sample MixUp / CutMix on the training batch
    p.add_argument("--mixup-alpha", type=float, default=0.0,
                   help="MixUp: blend each sample with its batch neighbour, weight ~ Beta(alpha, alpha); 0 = off")
    p.add_argument("--cutmix-alpha", type=float, default=0.0,
                   help="CutMix: paste a box of the batch neighbour, area from Beta(alpha, alpha); 0 = off")
    p.add_argument("--mix-prob", type=float, default=1.0, help="probability that a sample is mixed at all")
    p.add_argument("--mix-switch-prob", type=float, default=0.5,
                   help="with both alphas set: probability that a mixed sample takes CutMix rather than MixUp")
    # ---- input transforms (the defaults are the CIFAR recipe: pad-crop + flip, untransformed evaluation)
    p.add_argument("--train-transform", default="pad-crop", choices=["pad-crop", "random-resized-crop"],
                   help="random-resized-crop: a random box of --rrc-scale x the area and --rrc-ratio aspect, "
                        "resized to --train-size, then a flip (the ImageNet recipe)")
    p.add_argument("--train-size", type=int, default=None,
                   help="output side of random-resized-crop and of the center-crop evaluation "
                        "(default: the side of the stored images)")
    p.add_argument("--rrc-scale", type=float, nargs=2, default=[0.08, 1.0], metavar=("LO", "HI"),
                   help="random-resized-crop: range of the box area as a share of the image")
    p.add_argument("--rrc-ratio", type=float, nargs=2, default=[3.0 / 4.0, 4.0 / 3.0], metavar=("LO", "HI"),
                   help="random-resized-crop: range of the box aspect w / h (log-uniform)")
    p.add_argument("--eval-transform", default="none", choices=["none", "center-crop"],
                   help="center-crop: evaluate on the centred --eval-crop-pct box resized to --train-size")
    p.add_argument("--eval-crop-pct", type=float, default=0.875)
    # ---- per-sample augmentation policy (off by default): after crop + flip, before normalisation
    p.add_argument("--auto-augment", default="none", choices=["none", "trivial-wide"],
                   help="trivial-wide: TrivialAugmentWide, one of 14 operations per sample at a random magnitude "
                        "(un-normalised uint8 datasets: cifar10, array)")
    p.add_argument("--random-erase-prob", type=float, default=0.0,
                   help="RandomErasing: probability that a box of the normalised sample is zeroed; 0 = off")
    p.add_argument("--random-erase-scale", type=float, nargs=2, default=[0.02, 0.33], metavar=("LO", "HI"),
                   help="RandomErasing: range of the box area as a share of the image")
    p.add_argument("--random-erase-ratio", type=float, nargs=2, default=[0.3, 3.3], metavar=("LO", "HI"),
                   help="RandomErasing: range of the box aspect h / w (log-uniform)")
    # ---- weight EMA (off by default): evaluated and checkpointed beside the raw weights
    p.add_argument("--ema-decay", type=float, default=0.0,
                   help="exponential moving average of the weights and BatchNorm statistics with this decay "
                        "(optim.ModelEma), evaluated after the raw weights and saved as <name>.ema<ext>; 0 = off")
    p.add_argument("--ema-every", type=int, default=1, help="update the EMA every N-th step")
    p.add_argument("--ema-warmup", action="store_true",
                   help="EMA decay min(--ema-decay, (1 + k) / (10 + k)) at update k")
    return p


def input_transforms(args, image_hw):
    """(train, eval) loader transforms of the parsed flags, None where the CIFAR chain stays; raises
    ValueError on a bad size or range.  ``image_hw`` sizes the output when --train-size is not given."""
    size = (args.train_size, args.train_size) if args.train_size is not None else tuple(image_hw)
    train = evalt = None
    if args.train_size is not None and args.train_size < 1:
        raise ValueError(f"--train-size must be positive, got {args.train_size}")
    if args.train_transform == "random-resized-crop":
        train = RandomResizedCrop(size, tuple(args.rrc_scale), tuple(args.rrc_ratio)).validate()
    if args.eval_transform == "center-crop":
        evalt = CenterCropResize(size, args.eval_crop_pct).validate()
    return train, evalt


class _GraphStep:
    """One training step replayed from a HIP graph (``utils.graph.CapturedStep``).

    The first WARMUP full-size batches train eagerly (lazy initialisation, allocator pools,
    kernel attributes); the next one is copied into static input tensors, captured (capture
    executes nothing) and replayed, and so is every later full-size batch -- every batch is
    trained on exactly once.  A batch of another shape (an epoch's last, partial batch) runs
    eagerly.  The CPU bookkeeping of the step (reducer hooks, BN counters, weight-mirror
    versions) runs during capture only, which is valid because the ResNet step is static.
    """

    WARMUP = 3

    def __init__(self, ddp_model, criterion, optimizer, period: int = 1):
        self.ddp_model, self.criterion, self.optimizer = ddp_model, criterion, optimizer
        self.period = period  # 3 with fp8: the delayed-scaling slot ring (utils.graph.CapturedStep)
        self.x = self.y = None
        self.warm = 0
        self.side = None
        self.captured = None
        self.hyper = None

    def _hyperparameters(self):
        """The optimizer settings the fused SGD launch bakes into the graph as kernel arguments."""
        return [tuple((k, v) for k, v in sorted(g.items()) if k != "params" and isinstance(v, (int, float, bool)))
                for g in self.optimizer.param_groups]

    def eager(self, inputs, labels):
        self.optimizer.zero_grad()
        loss = self.criterion(self.ddp_model(inputs), labels)
        loss.backward()
        self.optimizer.step()
        return loss

    def __call__(self, inputs, labels):
        from .utils.graph import CapturedStep
        if self.x is not None and (inputs.shape != self.x.shape or labels.shape != self.y.shape):
            return self.eager(inputs, labels)
        if self.warm < self.WARMUP:
            self.warm += 1
            if self.warm == self.WARMUP:  # the full-size batch shape the graph is captured for
                self.x, self.y = inputs.clone(), labels.clone()
            # on a side stream, as torch prescribes for pre-capture warm-up: autograd nodes created
            # here (AccumulateGrad) must not tie the captured backward to the legacy default stream
            cur = torch.cuda.current_stream()
            if self.side is None:
                self.side = torch.cuda.Stream()
            self.side.wait_stream(cur)
            with torch.cuda.stream(self.side):
                loss = self.eager(inputs, labels)
            cur.wait_stream(self.side)
            return loss
        self.x.copy_(inputs)
        self.y.copy_(labels)
        hyper = self._hyperparameters()
        if self.captured is not None and (hyper != self.hyper or not self.captured.in_phase()):
            # lr / momentum / weight decay changed (a scheduler, user code): the captured SGD
            # launch would keep the old values; or (fp8) an eager partial batch / an evaluation
            # advanced the delayed-scaling slot rings past the graphs' phases -- capture again
            self.captured = None
        if self.captured is None:
            from .ops.fused import FP8_RING
            self.hyper = hyper
            self.captured = CapturedStep(lambda: self.eager(self.x, self.y), warmup=0, period=self.period,
                                         ring=FP8_RING if self.period > 1 else None)
        return self.captured()


def evaluate(model: nn.Module, device: torch.device, test_loader) -> float:
    """Top-1 accuracy (``resnet/main.py:23-37``), fused argmax/compare/count on GPU."""
    model.eval()
    correct = torch.zeros((), dtype=torch.long, device=device)
    total = 0
    with torch.no_grad():
        for images, labels in test_loader:
            images, labels = images.to(device), labels.to(device)
            outputs = model(images)
            correct += ops.top1_correct(outputs, labels)
            total += labels.size(0)
    return correct.item() / max(total, 1)


def main(argv: Optional[list] = None) -> int:
    args = build_parser().parse_args(argv)
    if args.graph and args.lr_schedule != "constant":
        # the captured step bakes lr in as a kernel argument: _GraphStep would capture again every step
        raise SystemExit(f"--graph cannot follow --lr-schedule {args.lr_schedule}: the captured step bakes "
                         "the learning rate in, so a schedule would re-capture it every step; use "
                         "--lr-schedule constant with --graph")
    try:
        mix = MixConfig(args.mixup_alpha, args.cutmix_alpha, args.mix_prob, args.mix_switch_prob).validate()
    except ValueError as e:
        raise SystemExit(f"--mixup-alpha / --cutmix-alpha / --mix-prob / --mix-switch-prob: {e}")
    mix = mix if mix.enabled else None
    if args.graph and mix is not None:
        # _GraphStep keeps one static label tensor; a mixed batch carries two labels and a weight per row
        raise SystemExit("--graph cannot be combined with --mixup-alpha / --cutmix-alpha: the captured step "
                         "holds one static label tensor, not a mixed target; run mixing without --graph")
    try:  # ranges now, before anything is set up; the sizes again once the dataset is known
        input_transforms(args, (1, 1))
    except ValueError as e:
        raise SystemExit(f"--train-size / --rrc-scale / --rrc-ratio / --eval-crop-pct: {e}")
    try:
        aug = AugConfig(args.auto_augment, args.random_erase_prob, tuple(args.random_erase_scale),
                        tuple(args.random_erase_ratio)).validate()
    except ValueError as e:
        raise SystemExit(f"--auto-augment / --random-erase-prob / --random-erase-scale / --random-erase-ratio: {e}")
    aug = aug if aug.enabled else None
    if aug is not None and args.data not in ("cifar10", "array"):
        raise SystemExit(f"--auto-augment / --random-erase-prob cannot be combined with --data {args.data}: the "
                         "policy works on 8-bit levels and must be given an un-normalised uint8 dataset (cifar10, array)")
    if not 0.0 <= args.ema_decay < 1.0:
        raise SystemExit(f"--ema-decay must be in [0, 1) (0 = off), got {args.ema_decay}")
    if args.ema_every < 1:
        raise SystemExit(f"--ema-every must be at least 1, got {args.ema_every}")
    if args.ema_decay > 0.0 and args.dtype == "fp8":
        # the delayed-scaling slot rings are process-global: an evaluation of the twin would advance them
        raise SystemExit("--ema-decay cannot be combined with --dtype fp8: the fp8 delayed-scaling state is "
                         "process-global, so the EMA twin cannot be evaluated beside the model")
    set_random_seeds(args.seed, deterministic=args.deterministic)
    env = init_distributed(args.backend, args.local_rank, args.timeout)
    local_rank = env.local_rank
    use_cuda = torch.cuda.is_available() and args.backend != "gloo"
    device = torch.device(f"cuda:{local_rank}") if use_cuda else torch.device("cpu")
    impl = args.impl
    if impl == "auto":
        impl = "native" if device.type == "cuda" else "torch"
    dtype = args.dtype
    if dtype == "auto":
        dtype = "bf16" if impl == "native" else "fp32"
    if impl == "native" and dtype not in ("bf16", "fp8"):
        raise SystemExit("--impl native computes in bf16 or fp8 (fp32 master weights); use --impl torch for fp32")
    if dtype == "fp8":
        if impl != "native" or device.type != "cuda":
            raise SystemExit("--dtype fp8 needs the native impl on a GPU")
        ops.set_fp8(True)
    if args.graph and (impl != "native" or device.type != "cuda"):
        raise SystemExit("--graph needs the native impl on a GPU")
    if impl == "native" and device.type == "cuda":
        torch.cuda.set_device(device)
        from .ops.streams import use_critical_stream
        # high-priority critical path: eager single-process fp8 steps only (ops/streams.py)
        use_critical_stream(device, collective=env.world_size > 1, graph=bool(args.graph), fp8=dtype == "fp8")
    autocast = (impl == "torch" and dtype == "bf16")
    if args.trace:
        trace.enable(True)

    # progress watchdog, armed before the DDP constructor so a peer that dies during the
    # communicator bring-up is caught too (on by default for multi-process runs)
    wd_timeout = args.watchdog_timeout
    if wd_timeout is None:
        wd_timeout = 900.0 if env.world_size > 1 else 0.0
    holder = {}
    watchdog = None
    if wd_timeout > 0:
        watchdog = Watchdog(wd_timeout, rank=env.rank,
                            on_timeout=lambda: holder["ddp"].abort() if "ddp" in holder else None)
        watchdog.heartbeat("setup")

    model = build_model(args.arch, num_classes=args.num_classes, impl=impl).to(device)
    if impl == "native":
        model.set_impl("native")  # re-assert channels_last weights after .to()
    ddp_model = DistributedDataParallel(model, device_ids=[local_rank] if use_cuda else None,
                                        output_device=local_rank if use_cuda else None,
                                        bucket_cap_mb=args.bucket_mb, wire_dtype=args.wire_dtype,
                                        comm_options=CommOptions.from_env(timeout=args.timeout))
    holder["ddp"] = ddp_model
    if mix is not None:  # the two-label target: ops.CrossEntropyLoss for both impls (CPU = reference)
        criterion = ops.CrossEntropyLoss(label_smoothing=args.label_smoothing)
    elif args.label_smoothing != 0.0:
        criterion = ops.CrossEntropyLoss(label_smoothing=args.label_smoothing) if impl == "native" \
            else nn.CrossEntropyLoss(label_smoothing=args.label_smoothing)
    else:
        criterion = ops.CrossEntropyLoss() if impl == "native" else nn.CrossEntropyLoss()
    timer = StepTimer(device, ddp_model)
    if args.log_every:
        ddp_model.enable_comm_timing(True)
    inject = FaultInjector(env.rank)
    # a captured step keeps the post-backward update (the per-bucket one's local-mode reducer made
    # graph replay ~2.7x slower, bench.py --graph)
    if args.optimizer == "lars":
        optimizer = LARS(ddp_model.parameters(), lr=args.learning_rate, momentum=args.momentum,
                         weight_decay=args.weight_decay, trust_coefficient=args.trust_coefficient,
                         eps=args.lars_eps, exclude_1d=not args.lars_adapt_1d,
                         overlap=False if args.graph else None)
    else:
        optimizer = SGD(ddp_model.parameters(), lr=args.learning_rate, momentum=args.momentum,
                        weight_decay=args.weight_decay, overlap=False if args.graph else None)

    # every rank keeps its own, identical EMA (the parameters are the same everywhere): no collectives
    ema = ModelEma(ddp_model, args.ema_decay, every=args.ema_every, warmup=args.ema_warmup) \
        if args.ema_decay > 0.0 else None

    model_filepath = os.path.join(args.model_dir, args.model_filename)
    start_epoch = 0
    if args.resume:
        ep = load_checkpoint(ddp_model, model_filepath, device, optimizer, ema=ema)
        if ep is not None:
            start_epoch = int(ep)

    n_train = args.synthetic_samples
    train_set = build_dataset(args.data, True, args.data_root, n_train,
                              num_classes=min(args.num_classes, 10 if "cifar" in args.data else 1000),
                              seed=args.seed)
    test_set = build_dataset(args.data, False, args.data_root,
                             None if n_train is None else max(n_train // 5, 1),
                             num_classes=min(args.num_classes, 10 if "cifar" in args.data else 1000),
                             seed=args.seed)
    if args.data == "array" and int(max(train_set.labels.max(), test_set.labels.max())) >= args.num_classes:
        raise SystemExit(f"--data array: labels reach {int(max(train_set.labels.max(), test_set.labels.max()))} "
                         f"but --num-classes is {args.num_classes}")
    train_tf, _ = input_transforms(args, train_set.images.shape[2:])
    _, eval_tf = input_transforms(args, test_set.images.shape[2:])
    train_sampler = DistributedSampler(len(train_set), num_replicas=env.world_size, rank=env.rank)
    train_loader = DeviceLoader(train_set, args.batch_size, sampler=train_sampler, augment=True,
                                device=device, seed=args.seed + env.rank, mix=mix, transform=train_tf, aug=aug)
    test_loader = DeviceLoader(test_set, 128, shuffle=False, augment=False, device=device, transform=eval_tf)

    graph_step = _GraphStep(ddp_model, criterion, optimizer, period=3 if dtype == "fp8" else 1) \
        if args.graph else None
    steps_per_epoch = len(train_loader)
    if args.max_steps_per_epoch is not None:
        steps_per_epoch = min(steps_per_epoch, args.max_steps_per_epoch)
    # a resumed run continues the step count (and with it the stateless schedule) where it stopped
    global_step = start_epoch * steps_per_epoch
    schedule = None
    if args.lr_schedule == "warmup-poly":
        total = max(args.num_epochs * steps_per_epoch, 1)
        schedule = WarmupPolyLR(optimizer, args.learning_rate,
                                min(int(round(args.warmup_epochs * steps_per_epoch)), total), total,
                                power=2.0, end_lr=args.lr_end)
    done = False
    for epoch in range(start_epoch, args.num_epochs):
        print("Local Rank: {}, Epoch: {}, Training ...".format(local_rank, epoch), flush=True)
        if epoch % args.eval_every == 0 and local_rank == 0:
            if watchdog is not None:
                watchdog.heartbeat("eval")
            with trace.trace_range("eval"):
                # a replayed graph cannot skip its captured buffer broadcast the way an eager
                # forward after a rank-0-only eval does, so with --graph rank 0
                # evaluates the wrapped module itself: no collective, same buffers
                accuracy = evaluate(model=ddp_model.module if graph_step is not None else ddp_model,
                                    device=device, test_loader=test_loader)
            # never persist weights a failed all-reduce left on this rank (a timed-out xGMI wait
            # NaN-poisons its bucket; a failed RCCL communicator is marked unusable): raise first
            if device.type == "cuda":
                torch.cuda.synchronize(device)
            ddp_model.check_comm()
            save_checkpoint(ddp_model, model_filepath, optimizer, epoch, ema=ema)
            print("-" * 75)
            print("Epoch: {}, Accuracy: {}".format(epoch, accuracy))
            print("-" * 75, flush=True)
            if ema is not None:
                with trace.trace_range("eval_ema"):
                    ema_accuracy = evaluate(model=ema.module, device=device, test_loader=test_loader)
                print("Epoch: {}, EMA accuracy: {}".format(epoch, ema_accuracy), flush=True)

        ddp_model.train()
        train_loader.set_epoch(epoch)
        timer.start()
        for step, (inputs, labels) in enumerate(train_loader):
            if args.max_steps_per_epoch is not None and step >= args.max_steps_per_epoch:
                break
            if args.steps is not None and global_step >= args.steps:
                done = True
                break
            if watchdog is not None:
                watchdog.heartbeat(f"epoch {epoch} step {step}")
            inject(global_step)
            inputs, labels = inputs.to(device), labels.to(device)
            if schedule is not None:
                # before the forward: the per-bucket update is armed with the rate it has there
                lr = schedule.set(global_step)
                if step == 0 and env.rank == 0:
                    print("Epoch: {}, step: {}, lr: {!r}".format(epoch, global_step, lr), flush=True)
            if graph_step is not None:
                with trace.trace_range("step"):
                    loss = graph_step(inputs, labels)
            else:
                optimizer.zero_grad()
                with trace.trace_range("forward"), torch.autocast(device.type, torch.bfloat16,
                                                                  enabled=autocast):
                    outputs = ddp_model(inputs)
                    loss = criterion(outputs, labels)
                with trace.trace_range("backward"):
                    loss.backward()
                with trace.trace_range("optimizer"):
                    optimizer.step()
            if ema is not None:  # eager also under --graph: warm-up and --ema-every stay host-side
                ema.update()
            timer.tick()
            global_step += 1
            if args.log_every and (step + 1) % args.log_every == 0:
                r = timer.report()
                if env.rank == 0 and r is not None:
                    msg = (f"  step {step + 1} loss {loss.item():.4f} {r['step_ms']:.2f} ms/step "
                           f"{args.batch_size * env.world_size * 1000.0 / r['step_ms']:.1f} img/s")
                    if "comm_ms" in r:
                        msg += f" allreduce {r['comm_ms']:.2f} ms (exposed {r['exposed_ms']:.2f} ms)"
                    print(msg, flush=True)
        if done:
            break
    if watchdog is not None:
        watchdog.stop()
    if env.world_size > 1:
        # every rank is past its last collective: end the process here (as bench.py does) rather
        # than in interpreter teardown, where the reducer's native communicators (RCCL, and the
        # xGMI buffers peers may still map) would be destroyed in an unspecified order with torch's
        torch.distributed.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        destroy()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    destroy()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
