from .regseg import (AdaptiveShortcutBlock, DBlock, RegSeg, RegSeg48, RegSeg53, RegSegBackbone, RegSegDecoder, RegSegHead,  # noqa: F401
                     SplitDilatedGroupConvBlock, SqueezeAndExcitationBlock)
from .ddrnet import DAPPM, DAPPMBranch  # noqa: F401
