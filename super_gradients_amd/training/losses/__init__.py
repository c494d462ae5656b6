from .ddrnet_loss import DDRNetLoss  # noqa: F401
from .label_smoothing_cross_entropy_loss import CrossEntropyLoss  # noqa: F401
from .ohem_ce_loss import OhemCELoss  # noqa: F401
from .ppyolo_loss import PPYoloELoss  # noqa: F401
from .shelfnet_ohem_loss import ShelfNetOHEMLoss  # noqa: F401
