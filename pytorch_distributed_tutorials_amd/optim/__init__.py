from .ema import ModelEma  # noqa: F401
from .lars import LARS  # noqa: F401
from .schedule import WarmupPolyLR  # noqa: F401
from .sgd import SGD  # noqa: F401
