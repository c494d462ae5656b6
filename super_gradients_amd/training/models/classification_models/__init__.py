from .resnet import (BasicResNetBlock, Bottleneck, CifarResNet, ResNet, ResNet18, ResNet18Cifar, ResNet34, ResNet50, ResNet101,  # noqa: F401
                     ResNet152, ResNet50_3343)
from .repvgg import (RepVGG, RepVggA0, RepVggA1, RepVggA2, RepVggB0, RepVggB1, RepVggB2, RepVggB3, RepVggCustom, RepVggD2SE)  # noqa: F401
from .mobilenetv2 import CustomMobileNetV2, InvertedResidual, MobileNetV2, MobileNetV2_135, MobileNetV2Base  # noqa: F401
from .mobilenetv3 import MobileNetV3, mobilenetv3_custom, mobilenetv3_large, mobilenetv3_small  # noqa: F401
from .regnet import (AnyNetX, CustomAnyNet, CustomRegNet, Head, NASRegNet, RegNetX, RegNetY, RegNetY200, RegNetY400, RegNetY600, RegNetY800,  # noqa: F401
                     Stage, Stem, XBlock, regnet_params_to_blocks, verify_correctness_of_parameters)
from .resnext import GroupedConvBlock, ResNeXt, ResNeXt50, ResNeXt101  # noqa: F401
from .efficientnet import (BlockArgs, BlockDecoder, CustomizedEfficientnet, EfficientNet, EfficientNetB0, EfficientNetB1, EfficientNetB2,  # noqa: F401
                           EfficientNetB3, EfficientNetB4, EfficientNetB5, EfficientNetB6, EfficientNetB7, EfficientNetB8, EfficientNetL2,
                           MBConvBlock, round_filters, round_repeats)
from .vit import ViT, ViTBase, ViTHuge, ViTLarge  # noqa: F401
from .beit import Beit, BeitBasePatch16_224, BeitLargePatch16_224  # noqa: F401
from .densenet import (CustomizedDensnet, DenseBlock, DenseLayer, DenseNet, DenseNet121, DenseNet161, DenseNet169, DenseNet201, Transition)  # noqa: F401
from .shufflenetv2 import (ChannelShuffleInvertedResidual, CustomizedShuffleNetV2, ShuffleNetV2Base, ShufflenetV2_x0_5, ShufflenetV2_x1_0,  # noqa: F401
                           ShufflenetV2_x1_5, ShufflenetV2_x2_0)
