"""RepVGG classifiers on the HIP kernels.

Reference: training/models/classification_models/repvgg.py - RepVGG (:23-134), RepVggCustom / A0 / A1 / A2 / B0 / B1 / B2 / B3 / D2SE
(:137-204); defaults of recipes/arch_params/repvgg_arch_params.yaml.  Same constructor arguments, `struct` / `width_multiplier` tables
and state_dict keys (stem.*, stage{1..4}.{j}.*, linear.*), so checkpoints interchange both ways.

Kernel sequence (training): every block is a modules.RepVGGBlock.  The first block of a stage (stride 2) is the two-branch form, every
other block adds the identity-BatchNorm branch, whose batch statistics are those of the block's input: the forward sweep of the block
BEFORE leaves them (sgx_tri_affine_act_fwd's statistics rows), so inside a stage no statistics pass over an activation runs.  Then
global average pool -> linear, as in resnet.py.

Not built (each raises NotImplementedError): use_se=True - the reference builds its SEBlock with the block's INPUT width (repvgg.py:94-95),
so its forward fails as soon as a stage changes width; no named variant enables it (RepVggD2SE takes use_se from arch_params, default
False, and is built without SE exactly as the reference builds it); backbone_mode=True (as for ResNet); stage widths that are not
multiples of 4 (the sweeps move 16-byte channel groups; every named variant's widths are).
"""
from torch import nn

from ....common.registry import register_model
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.layers import LinearLayer, Numbered
from ....modules.repvgg_block import RepVGGBlock, fuse_repvgg_blocks_residual_branches
from ...utils.utils import get_param

_BRANCH_KEYS = ("branch_3x3.", "branch_1x1.", "no_conv_branch.")


def _training_form_key(key: str) -> bool:
    return any(b in key for b in _BRANCH_KEYS) or key.endswith(".alpha")


class RepVGG(SgxClassifier):
    _head_path = _finetune_key = "linear"

    def __init__(self, struct, num_classes=1000, width_multiplier=None, build_residual_branches=True, use_se=False, backbone_mode=False, in_channels=3):
        """
        :param struct: number of blocks per stage
        :param num_classes: outputs of the classification head
        :param width_multiplier: per-stage width multipliers, or one float for all four stages
        :param build_residual_branches: False builds the deployment form (one 3x3 convolution per block, inference only)
        """
        super().__init__()
        if use_se:
            raise NotImplementedError("RepVGG(use_se=True) is not on the HIP path: the reference sizes its SEBlock by the block's input width "
                                      "(repvgg.py:94-95), which fails in forward wherever a stage changes width; no named variant enables it")
        if backbone_mode:
            raise NotImplementedError("RepVGG on the HIP path: backbone_mode=False")
        if isinstance(width_multiplier, float):
            width_multiplier = [width_multiplier] * 4
        else:
            assert len(width_multiplier) == 4
        widths = [int(b * m) for b, m in zip((64, 128, 256, 512), width_multiplier)]
        if any(w % 4 for w in widths):
            raise NotImplementedError(f"RepVGG on the HIP path: stage widths must be multiples of 4 (16-byte channel groups), got {widths}")
        self.build_residual_branches = build_residual_branches
        self.use_se, self.backbone_mode = use_se, backbone_mode
        self.in_planes = widths[0]
        self.stem = RepVGGBlock(in_channels, self.in_planes, stride=2, build_residual_branches=build_residual_branches, activation_type=nn.ReLU)
        self.stage1 = self._make_stage(widths[0], struct[0], stride=2)
        self.stage2 = self._make_stage(widths[1], struct[1], stride=2)
        self.stage3 = self._make_stage(widths[2], struct[2], stride=2)
        self.stage4 = self._make_stage(widths[3], struct[3], stride=2)
        self.linear = LinearLayer(widths[3], num_classes)
        self.final_width_mult = width_multiplier[3]
        if not build_residual_branches:
            self.eval()  # (reference :75-77: a model without residual branches is built in eval mode)

    def _make_stage(self, planes, struct, stride):
        blocks = []
        for s in [stride] + [1] * (struct - 1):
            blocks.append(RepVGGBlock(self.in_planes, planes, stride=s, groups=1, build_residual_branches=self.build_residual_branches,
                                      activation_type=nn.ReLU))
            self.in_planes = planes
        return Numbered(blocks)  # (keys stage{i}.{j}.*)

    def _blocks(self):
        return [self.stem] + [b for s in (self.stage1, self.stage2, self.stage3, self.stage4) for b in s.blocks()]

    def _fwd(self, x):
        a = self._input_nhwc(x)
        blocks = self._blocks()
        stats = None
        for blk, nxt in zip(blocks, blocks[1:] + [None]):
            # the identity BatchNorm of the NEXT block normalises this block's output: its forward sweep leaves that tensor's statistics rows
            want = self.training and nxt is not None and getattr(nxt, "no_conv_branch", None) is not None
            a = blk.fwd(a, x_stats=stats, want_stats=want)
            stats = blk.take_stats() if want else None
        return (self._pool_head_fwd(a, self.linear),)

    def _bwd(self, d_logits):
        d = self._pool_head_bwd(d_logits, self.linear)
        ready = self._bucket_ready
        ready("linear.")
        for name in ("stage4", "stage3", "stage2", "stage1"):
            for blk in reversed(getattr(self, name).blocks()):
                d = blk.bwd(d)
            ready(f"{name}.")
        self.stem.bwd(d, need_dx=False)
        ready("stem.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["stem.", "stage1.", "stage2.", "stage3.", "stage4.", "linear."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.stem.in_channels

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        """Reference :114-116: every block -> one 3x3 convolution + bias (eval mode only); the model is inference-only afterwards."""
        if self.build_residual_branches:
            if not self.training:
                self.materialize()
            fuse_repvgg_blocks_residual_branches(self)
        return self

    def train(self, mode: bool = True):
        assert not mode or self.build_residual_branches, \
            "Trying to train a model without residual branches, set arch_params.build_residual_branches to True and retrain the model"
        return super().train(mode=mode)  # (the reference's override returns None, :118-123 - an oversight: nn.Module.train returns self)

    def state_dict(self, *args, **kwargs):
        """The deployment form's state is rbr_reparam.* (+ linear.*), as the reference's fused model's: there fusing deletes the branch
        modules; here they stay (the arenas own their storage) and are left out of the state."""
        sd = super().state_dict(*args, **kwargs)
        if not self.build_residual_branches:
            for k in [k for k in sd if _training_form_key(k)]:
                del sd[k]
        return sd

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        own = dict(nn.Module.state_dict(self))
        if self.build_residual_branches or not strict or not any(_training_form_key(k) for k in own):
            return super().load_state_dict(state_dict, strict=strict, **kw)
        # a fused training-form model: strict with respect to the deployment form's keys
        out = super().load_state_dict(state_dict, strict=False, **kw)
        missing = [k for k in out.missing_keys if not _training_form_key(k)]
        if missing or out.unexpected_keys:
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing keys {missing}, unexpected keys {list(out.unexpected_keys)}")
        return out


@register_model("repvgg_custom")
class RepVggCustom(RepVGG):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(struct=get_param(arch_params, "struct"), num_classes=num_classes_of(arch_params, num_classes),
                         width_multiplier=get_param(arch_params, "width_multiplier"),
                         build_residual_branches=get_param(arch_params, "build_residual_branches", True), use_se=get_param(arch_params, "use_se", False),
                         backbone_mode=get_param(arch_params, "backbone_mode", False), in_channels=get_param(arch_params, "in_channels", 3))


def _variant(name, cls_name, struct, width_multiplier):
    def init(self, arch_params, num_classes=None):
        arch_params.override(struct=list(struct), width_multiplier=list(width_multiplier))
        RepVggCustom.__init__(self, arch_params=arch_params, num_classes=num_classes)

    return register_model(name)(type(cls_name, (RepVggCustom,), {"__init__": init}))


RepVggA0 = _variant("repvgg_a0", "RepVggA0", [2, 4, 14, 1], [0.75, 0.75, 0.75, 2.5])
RepVggA1 = _variant("repvgg_a1", "RepVggA1", [2, 4, 14, 1], [1, 1, 1, 2.5])
RepVggA2 = _variant("repvgg_a2", "RepVggA2", [2, 4, 14, 1], [1.5, 1.5, 1.5, 2.75])
RepVggB0 = _variant("repvgg_b0", "RepVggB0", [4, 6, 16, 1], [1, 1, 1, 2.5])
RepVggB1 = _variant("repvgg_b1", "RepVggB1", [4, 6, 16, 1], [2, 2, 2, 4])
RepVggB2 = _variant("repvgg_b2", "RepVggB2", [4, 6, 16, 1], [2.5, 2.5, 2.5, 5])
RepVggB3 = _variant("repvgg_b3", "RepVggB3", [4, 6, 16, 1], [3, 3, 3, 5])
RepVggD2SE = _variant("repvgg_d2se", "RepVggD2SE", [8, 14, 24, 1], [2.5, 2.5, 2.5, 5])
