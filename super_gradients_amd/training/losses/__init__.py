from .bce_dice_loss import BCEDiceLoss  # noqa: F401
from .ddrnet_loss import DDRNetLoss  # noqa: F401
from .dice_loss import BinaryDiceLoss, DiceLoss, GeneralizedDiceLoss  # noqa: F401
from .iou_loss import BinaryIoULoss, GeneralizedIoULoss, IoULoss  # noqa: F401
from .label_smoothing_cross_entropy_loss import CrossEntropyLoss  # noqa: F401
from .ohem_ce_loss import OhemCELoss  # noqa: F401
from .ppyolo_loss import PPYoloELoss  # noqa: F401
from .shelfnet_ohem_loss import ShelfNetOHEMLoss  # noqa: F401
