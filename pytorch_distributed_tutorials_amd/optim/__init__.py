from .clip import clip_grad_norm_  # noqa: F401
from .ema import ModelEma  # noqa: F401
from .lamb import LAMB  # noqa: F401
from .lars import LARS  # noqa: F401
from .schedule import WarmupCosineLR, WarmupPolyLR  # noqa: F401
from .sgd import SGD  # noqa: F401
