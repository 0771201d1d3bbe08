from .autoaug import (  # noqa: F401
    AugConfig,
    AugDraw,
    apply_policy,
    apply_policy_levels,
    draw_policy,
    erase_boxes,
)
from .datasets import (  # noqa: F401
    CIFAR_MEAN,
    CIFAR_STD,
    IMAGENET_MEAN,
    IMAGENET_STD,
    TensorImageDataset,
    array_dataset,
    build_dataset,
    cifar10,
    learnable_dataset,
    synthetic_dataset,
)
from .loader import DeviceLoader, draw_crop_flip, random_crop_flip  # noqa: F401
from .mix import MixConfig, MixDraw, MixedTarget, draw_mix, mix_batch  # noqa: F401
from .resize import (  # noqa: F401
    CenterCropResize,
    RandomResizedCrop,
    center_box,
    draw_rrc,
    resample_weights,
    resized_crop,
)
from .sampler import DistributedSampler  # noqa: F401
