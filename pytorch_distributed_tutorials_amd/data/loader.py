"""Device-side batch loader with the reference's CIFAR augmentation.

Replaces ``DataLoader(dataset, batch_size, sampler, num_workers=8)``
(``resnet/main.py:98,100``) + the PIL transform chain
``RandomCrop(32, padding=4) -> RandomHorizontalFlip -> ToTensor -> Normalize``
(``resnet/main.py:87-92``) with batched GPU ops on a device-resident dataset:
gather the sampler's indices, zero-pad by 4, random-crop via two ``gather``s,
random flip, normalize.  Padding happens before normalization exactly like
torchvision (pad pixels are black, i.e. ``-mean/std`` after normalization).
Evaluation uses no augmentation (reference defect D7 fixed).

On the GPU the whole chain (gather by index, /255, pad+crop, flip, normalize) is ONE fused HIP
kernel (``csrc/kernels/augment.hip``) fed with crop offsets and flips drawn exactly as the torch
path draws them, so both paths produce identical batches (tests/test_kernels_gpu.py).

With ``transform=`` the loader runs the ImageNet chain of ``data/resize.py`` instead: a box per
sample (``RandomResizedCrop`` for training, ``CenterCropResize`` for evaluation) resized to a fixed
output size, flipped and normalized -- one ``_C_img.resized_crop`` kernel on the GPU
(``csrc/img/resample.hip``), ``resized_crop`` of ``data/resize.py`` otherwise, both fed by the same
box and flip draws.

With ``aug=`` the batch goes through the per-sample augmentation policy of ``data/autoaug.py``
(TrivialAugmentWide, RandomErasing) between the crop chain and normalisation: the crop kernel runs with
normalisation off and one ``_C_img.autoaug`` op (``csrc/img/autoaug.hip``) applies the policy,
normalises and erases on the GPU, ``apply_policy`` of ``data/autoaug.py`` otherwise, both fed by the same
``draw_policy`` draws.  Order: crop + flip, policy, normalise, erase, mix.
"""
from __future__ import annotations

import math
from typing import Iterator, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from .autoaug import MAX_SIDE, AugConfig, AugDraw, apply_policy, draw_policy
from .datasets import TensorImageDataset
from .mix import MixConfig, MixDraw, MixedTarget, draw_mix, mix_batch
from .resize import CenterCropResize, RandomResizedCrop, center_box, draw_rrc, resized_crop


def _normalize(x: torch.Tensor, mean, std) -> torch.Tensor:
    m = torch.tensor(mean, device=x.device, dtype=x.dtype).view(1, -1, 1, 1)
    s = torch.tensor(std, device=x.device, dtype=x.dtype).view(1, -1, 1, 1)
    return (x - m) / s


def draw_crop_flip(b: int, pad: int, device, gen: Optional[torch.Generator]):
    """Per-sample RandomCrop offsets (0..2*pad) and RandomHorizontalFlip(p=0.5) decisions."""
    oy = torch.randint(0, 2 * pad + 1, (b,), device=device, generator=gen)
    ox = torch.randint(0, 2 * pad + 1, (b,), device=device, generator=gen)
    flip = torch.rand((b,), device=device, generator=gen) < 0.5
    return oy, ox, flip


def random_crop_flip(x: torch.Tensor, pad: int, gen: Optional[torch.Generator]) -> torch.Tensor:
    """Batched RandomCrop(size=H, padding=pad) + RandomHorizontalFlip(p=0.5)."""
    b, c, h, w = x.shape
    xp = F.pad(x, (pad, pad, pad, pad))
    oy, ox, flip = draw_crop_flip(b, pad, x.device, gen)
    ar_h = torch.arange(h, device=x.device)
    ar_w = torch.arange(w, device=x.device)
    iy = (oy[:, None] + ar_h)[:, None, :, None].expand(b, c, h, w + 2 * pad)
    xr = xp.gather(2, iy)
    cols = torch.where(flip[:, None], ox[:, None] + (w - 1 - ar_w), ox[:, None] + ar_w)
    return xr.gather(3, cols[:, None, None, :].expand(b, c, h, w))


class DeviceLoader:
    """Iterates ``(images[B,3,H,W] float32, labels[B] int64)`` batches on ``device``.

    With ``mix=MixConfig(...)`` the batch is mixed per sample (MixUp / CutMix, ``data/mix.py``) and
    comes as ``(images, MixedTarget)``: one ``augment_mix`` kernel on the fused path, the chain
    below followed by ``mix_batch`` on the torch path, both fed by the same ``draw_mix`` draws made
    after the batch's crop/flip draws.  Evaluation loaders pass no ``mix``.

    ``transform=RandomResizedCrop(...)`` replaces the pad-crop + flip chain of ``augment`` (which it
    implies) by a random box resized to the transform's size and a flip;
    ``transform=CenterCropResize(...)`` is the evaluation counterpart (no draws, ``augment`` must be
    off).  Batches then have the transform's output size, and mix boxes are drawn for that size and
    applied (``mix_batch``) to the transformed batch on both paths.  ``None`` changes nothing.

    ``aug=AugConfig(...)`` runs the per-sample policy of ``data/autoaug.py`` on the training batch: after
    crop and flip the batch is quantised to 8-bit levels, every sample goes through its own operation,
    then normalisation, the erase box and the mix (``mix_batch`` on both paths).  It needs a training
    chain (``augment=True`` or a ``RandomResizedCrop``) over an un-normalised 3-channel dataset.  Its
    draws come from a third random stream, after the batch's crop/flip draws: a run with the policy
    sees the crops, flips and mixes of the run without it.  ``None`` (or a config with everything
    off) changes nothing."""

    def __init__(self, dataset: TensorImageDataset, batch_size: int, sampler=None,
                 shuffle: bool = False, augment: bool = False, device="cpu",
                 drop_last: bool = False, seed: int = 0, fused: Optional[bool] = None,
                 mix: Optional[MixConfig] = None,
                 transform: Union[RandomResizedCrop, CenterCropResize, None] = None,
                 aug: Optional[AugConfig] = None):
        self.ds = dataset.to(device)
        # MixUp / CutMix (data/mix.py): batches come as (images, MixedTarget); None = hard labels
        self.mix = MixConfig(*mix).validate() if mix is not None else None
        self.batch_size = batch_size
        self.sampler = sampler
        self.shuffle = shuffle
        self.augment = augment
        self.device = torch.device(device)
        self.drop_last = drop_last
        self.seed = seed
        self.epoch = 0
        # fused HIP augmentation on GPU datasets (None = when the native extension is available)
        if fused is None:
            from ..ops._ext import native_available
            fused = self.device.type == "cuda" and native_available()
        if transform is not None:
            if not isinstance(transform, (RandomResizedCrop, CenterCropResize)):
                raise ValueError(f"transform must be RandomResizedCrop, CenterCropResize or None, got {transform!r}")
            if augment and isinstance(transform, CenterCropResize):
                raise ValueError("CenterCropResize is an evaluation transform: it cannot follow augment=True")
            transform.validate()
        self.transform = transform
        # size of the batches (the 16-byte stores of the fused kernels need a width that is a multiple of 4)
        self.out_hw = tuple(self.ds.images.shape[2:]) if transform is None else transform.out_hw
        self.fused = bool(fused) and self.device.type == "cuda" and self.out_hw[1] % 4 == 0
        # the per-sample policy (data/autoaug.py); None = off
        aug = AugConfig(*aug).validate() if aug is not None else None
        self.aug = aug if aug is not None and aug.enabled else None
        if self.aug is not None:
            if isinstance(transform, CenterCropResize):
                raise ValueError("aug: the augmentation policy cannot follow CenterCropResize, an evaluation transform")
            if not augment and transform is None:
                raise ValueError("aug: the augmentation policy is a training transform: it needs augment=True or a "
                                 "RandomResizedCrop (evaluation never augments)")
            if self.ds.normalized:
                raise ValueError("aug: the augmentation policy works on 8-bit levels: it needs an un-normalised "
                                 "uint8 dataset (cifar10, array), not a normalised one")
            if self.ds.images.shape[1] != 3:
                raise ValueError(f"aug: the augmentation policy needs RGB images, got C = {self.ds.images.shape[1]}")
            if max(self.out_hw) > MAX_SIDE:
                raise ValueError(f"aug: the augmentation policy takes sides up to {MAX_SIDE}, got {self.out_hw}")

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch
        if self.sampler is not None and hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def _indices(self) -> Sequence[int]:
        if self.sampler is not None:
            return list(iter(self.sampler))
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            return torch.randperm(len(self.ds), generator=g).tolist()
        return list(range(len(self.ds)))

    def __len__(self) -> int:
        n = len(self.sampler) if self.sampler is not None else len(self.ds)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        idx = torch.tensor(self._indices(), dtype=torch.long)
        gen = None
        if self.augment or isinstance(self.transform, RandomResizedCrop):
            gen = torch.Generator(device=self.device)
            gen.manual_seed(self.seed * 1000003 + self.epoch)
        mgen = None
        if self.mix is not None:
            # the loader's second random stream: the mix draws of a batch come after its crop/flip
            # draws and never advance their stream, so every batch of a mixing run sees the crops
            # and flips the same run without mixing sees
            mgen = torch.Generator(device=self.device)
            mgen.manual_seed((self.seed * 1000003 + self.epoch) ^ 0x4D6978)
        agen = None
        if self.aug is not None:
            # the third stream: the policy draws of a batch come after its crop/flip draws and advance
            # neither that stream nor the mix stream
            agen = torch.Generator(device=self.device)
            agen.manual_seed((self.seed * 1000003 + self.epoch) ^ 0x417567)
        idx = idx.to(self.device)
        n = idx.numel()
        stop = (n // self.batch_size) * self.batch_size if self.drop_last else n
        for s in range(0, stop, self.batch_size):
            bi = idx[s:s + self.batch_size]
            y = self.ds.labels.index_select(0, bi)
            if self.fused:
                x, draw = self._fused_batch(bi, gen, mgen, agen)
                yield x, self._target(y, draw)
                continue
            x = self.ds.images.index_select(0, bi)
            if self.transform is not None:
                box, flip = self._draw_transform(bi.numel(), gen)
                x = x.float()
                if not self.ds.normalized:
                    x = self._finish(resized_crop(x.div_(255.0), box, self.out_hw, flip), agen)
                else:
                    x = resized_crop(x, box, self.out_hw, flip)
            elif not self.ds.normalized:
                x = x.float().div_(255.0)
                if self.augment:
                    x = random_crop_flip(x, 4, gen)
                x = self._finish(x, agen)
            elif self.augment:
                x = random_crop_flip(x, 4, gen)
            x = x.float().contiguous()
            draw = self._draw_mix(bi.numel(), mgen)
            if draw is not None:
                x = mix_batch(x, draw.partner, draw.w, draw.box)
            yield x, self._target(y, draw)

    def _draw_aug(self, b: int, gen) -> AugDraw:
        return draw_policy(b, *self.out_hw, self.aug, device=self.device, gen=gen)

    def _finish(self, x: torch.Tensor, agen) -> torch.Tensor:
        """The torch path from the cropped ``[0, 1]`` batch on: the policy when there is one (it
        normalises and erases as well), the normalisation alone otherwise."""
        if self.aug is None:
            return _normalize(x, self.ds.mean, self.ds.std)
        return apply_policy(x, self._draw_aug(x.shape[0], agen), self.ds.mean, self.ds.std)

    def _fused_aug(self, x: torch.Tensor, agen) -> torch.Tensor:
        """The fused path's counterpart of ``_finish`` for a policy: one ``_C_img.autoaug`` op."""
        from ..ops._ext import native_img
        d = self._draw_aug(x.shape[0], agen)
        # erasing alone: every operation is Identity, so the statistics pass has nothing to do
        passes = 2 if self.aug.policy == "none" else 3
        return native_img().autoaug(x, d.op, d.param, d.matrix, d.erase, True, list(self.ds.mean),
                                    list(self.ds.std), passes)

    def _draw_mix(self, b: int, gen) -> Optional[MixDraw]:
        if self.mix is None:
            return None
        return draw_mix(b, *self.out_hw, *self.mix, device=self.device, gen=gen)

    def _draw_transform(self, b: int, gen):
        """The boxes and flips of one batch under ``transform``: RandomResizedCrop draws the boxes
        (``draw_rrc``), then the flips, from the crop generator; CenterCropResize draws nothing."""
        h, w = self.ds.images.shape[2], self.ds.images.shape[3]
        if isinstance(self.transform, CenterCropResize):
            return center_box(b, h, w, self.transform.crop_pct, self.device), None
        box = draw_rrc(b, h, w, self.transform.scale, self.transform.ratio, self.device, gen)
        return box, torch.rand((b,), device=self.device, generator=gen) < 0.5

    @staticmethod
    def _target(y: torch.Tensor, draw: Optional[MixDraw]):
        if draw is None:
            return y
        return MixedTarget(y, y.index_select(0, draw.partner), draw.lam)

    def _fused_batch(self, bi: torch.Tensor, gen, mgen=None, agen=None) -> Tuple[torch.Tensor, Optional[MixDraw]]:
        from ..ops._ext import native, native_img, native_mix
        b = bi.numel()
        # with a policy the crop kernel leaves the batch in [0, 1] and autoaug normalises
        normalize = not self.ds.normalized and self.aug is None
        if self.transform is not None:
            box, flip = self._draw_transform(b, gen)
            imgs = self.ds.images
            if imgs.dtype not in (torch.uint8, torch.float32):
                imgs = imgs.float()
            x = native_img().resized_crop(imgs.contiguous(), bi.contiguous(), box, flip, *self.out_hw,
                                          normalize, list(self.ds.mean), list(self.ds.std))
            if self.aug is not None:
                x = self._fused_aug(x, agen)
            draw = self._draw_mix(b, mgen)
            if draw is not None:
                x = mix_batch(x, draw.partner, draw.w, draw.box)
            return x, draw
        if self.augment:
            oy, ox, flip = draw_crop_flip(b, 4, self.device, gen)
            pad = 4
        else:
            oy = ox = torch.zeros(b, dtype=torch.long, device=self.device)
            flip, pad = None, 0
        imgs = self.ds.images
        if imgs.dtype not in (torch.uint8, torch.float32):
            imgs = imgs.float()
        draw = self._draw_mix(b, mgen)
        if self.aug is not None:
            x = self._fused_aug(native().augment(imgs.contiguous(), bi.contiguous(), oy, ox, flip, pad, False,
                                                 list(self.ds.mean), list(self.ds.std)), agen)
            if draw is not None:
                x = mix_batch(x, draw.partner, draw.w, draw.box)
            return x, draw
        if draw is None:
            return native().augment(imgs.contiguous(), bi.contiguous(), oy, ox, flip, pad,
                                    not self.ds.normalized, list(self.ds.mean), list(self.ds.std)), None
        x = native_mix().augment_mix(imgs.contiguous(), bi.contiguous(), oy, ox, flip, pad,
                                     not self.ds.normalized, list(self.ds.mean), list(self.ds.std),
                                     draw.partner, draw.w, draw.box)
        return x, draw
