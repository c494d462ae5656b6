from .model_factory import get, get_model_name, instantiate_model  # noqa: F401
from .detection_models.yolo_nas import YoloNAS, YoloNAS_L, YoloNAS_M, YoloNAS_S  # noqa: F401
from .detection_models.customizable_detector import CustomizableDetector  # noqa: F401
from .classification_models import ResNet, ResNet18, ResNet18Cifar, ResNet34, ResNet50, CifarResNet  # noqa: F401
from .classification_models import RepVGG, RepVggA0, RepVggA1, RepVggA2, RepVggB0, RepVggB1, RepVggB2, RepVggB3, RepVggCustom, RepVggD2SE  # noqa: F401
from .classification_models import CustomMobileNetV2, MobileNetV2, MobileNetV2_135, MobileNetV2Base  # noqa: F401
from .classification_models import MobileNetV3, mobilenetv3_custom, mobilenetv3_large, mobilenetv3_small  # noqa: F401
from .classification_models import AnyNetX, CustomAnyNet, CustomRegNet, NASRegNet, RegNetX, RegNetY, RegNetY200, RegNetY400, RegNetY600, RegNetY800  # noqa: F401
from .classification_models import GroupedConvBlock, ResNeXt, ResNeXt50, ResNeXt101  # noqa: F401
from .classification_models import (CustomizedEfficientnet, EfficientNet, EfficientNetB0, EfficientNetB1, EfficientNetB2, EfficientNetB3, EfficientNetB4,  # noqa: F401
                                    EfficientNetB5, EfficientNetB6, EfficientNetB7, EfficientNetB8, EfficientNetL2)
from .classification_models import CustomizedDensnet, DenseNet, DenseNet121, DenseNet161, DenseNet169, DenseNet201  # noqa: F401
from .classification_models import (CustomizedShuffleNetV2, ShuffleNetV2Base, ShufflenetV2_x0_5, ShufflenetV2_x1_0, ShufflenetV2_x1_5,  # noqa: F401
                                    ShufflenetV2_x2_0)
from .classification_models import ViT, ViTBase, ViTHuge, ViTLarge  # noqa: F401
from .classification_models import Beit, BeitBasePatch16_224, BeitLargePatch16_224  # noqa: F401
from .detection_models.pp_yolo_e.pp_yolo_e import PPYoloE, PPYoloE_L, PPYoloE_M, PPYoloE_S, PPYoloE_X  # noqa: F401
