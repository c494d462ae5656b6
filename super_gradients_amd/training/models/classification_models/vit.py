"""Vision Transformer classifiers on the HIP kernels.

Reference: training/models/classification_models/vit.py - PatchEmbed (:19-43), FeedForward (:46-64), Attention (:67-98), TransformerBlock
(:101-113), Transformer (:116-126), ViT (:129-214) and the registered ViTBase / ViTLarge / ViTHuge (:217-268).  Same constructor arguments
and arch params (image_size, patch_size, in_channels, dropout_prob, emb_dropout_prob, num_classes), torch's default initial distributions
(randn for cls_token / pos_embedding) and the same state_dict keys and shapes (patch_embedding.proj.*, cls_token, pos_embedding,
transformer.blocks.{i}.norm1 / attn.to_qkv / attn.proj / norm2 / mlp.fc1 / mlp.fc2, pre_head_norm.*, head.*; linear weights [out, in]), so
checkpoints interchange both ways.

Tokens are pixels: the [B, T, D] sequence is the NHWC map [B, T, 1, D], and every nn.Linear over tokens is a 1x1 convolution with bias on the
tuned implicit-GEMM kernels (more than 95 % of the model's arithmetic).  New kernels (csrc/vit.h) are the glue only.

Kernel sequence (training; DESIGN.md 19 counts the passes):
    input_to_nhwc -> patch_rows (gather, (py, px, c) order) -> 1x1 conv + bias with the [D, Cin, ph, pw] filter in its OHWI storage
    -> token_assemble (class token, position embedding; one launch)
    per block:  LN1 -> to_qkv (1x1 + bias) -> attention (reads the q / k / v channel slices of the to_qkv output, writes heads side by side)
                -> proj (1x1 + bias, addend = block input) -> LN2 -> fc1 (1x1 + bias) -> GELU -> fc2 (1x1 + bias, addend = post-attention stream)
    head:       pre_head_norm on the class-token rows only (a [B, 1, 1, D] view with image stride T * D) -> nn.Linear
Backward of a block: g = gelu(h) recomputed; fc2 weight gradient and data gradient; gelu backward in place; fc1 weight / data gradient; LN2
backward with the skip gradient as its addend; proj weight / data gradient; attention backward straight into a [B, T, 1, 3D] buffer; to_qkv
weight / data gradient; LN1 backward with the skip gradient as its addend.  Weight gradients ride the network's grouped queue / side stream.

Stored per block for the backward (floats per token, D = hidden, F = mlp): the block input and the post-attention stream (2 D, LayerNorm
backward), both normalised maps (2 D, the weight gradients' operands), qkv (3 D), the attention output (D), the fc1 pre-activation (F), the
row statistics and the log-sum-exp (4 + heads).  Recomputed: gelu(h) (one sweep) and the attention probabilities (never stored).

Not built (each raises NotImplementedError): dropout_prob / emb_dropout_prob > 0 in training mode (eval is the identity), replace_head(new_head=...),
hidden_dim or hidden_dim / heads not a multiple of 4, in_channels neither 1..4 nor a multiple of 4, an input whose size differs from the
constructed image_size (the reference slices pos_embedding); supports_half_inference() is False.
"""
import math

import torch
from torch import nn

from .... import kernels as K
from ....common.registry import register_model
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import ConvLayer, LinearLayer
from ...utils.utils import get_param


def _not_built(msg):
    raise NotImplementedError(f"ViT on the HIP path: {msg}")


class TokenLinear(ConvLayer):
    """nn.Linear over tokens (weight [out, in], bias [out]) as a 1x1 convolution over [B, T, 1, in]: ConvLayer's conv / wgrad / dgrad on the
    [out, in, 1, 1] view of the same arena memory."""

    _param_kinds = {}

    def __init__(self, in_features, out_features, bias=True):
        SgxBlock.__init__(self)
        if in_features % 4 or out_features % 4:
            _not_built(f"token-wise linear layers need widths that are multiples of 4 (16-byte channel groups), got {in_features} -> {out_features}")
        self.in_features, self.out_features = in_features, out_features
        self.in_channels, self.out_channels = in_features, out_features
        self.kernel_size, self.stride, self.padding = 1, 1, 0
        w = torch.empty(out_features, in_features)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))  # nn.Linear default
        self.weight = nn.Parameter(w)
        bound = 1.0 / math.sqrt(in_features)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features).uniform_(-bound, bound))
        else:  # (BEiT's qkv: its owner passes a packed bias to the launch, or none)
            self.register_parameter("bias", None)
        self._w = self._gw = None

    def _filter_views(self, slot):
        return slot.kernel_view.view(self.out_features, self.in_features, 1, 1), slot.grad_kernel_view.view(self.out_features, self.in_features, 1, 1)

    def on_materialize(self):
        slots = {s.param: s for s in self._net.slots}
        self._w, self._gw = self._filter_views(slots[self.weight])
        self._wt = K.conv2d_wt_buffer(self._w, self._w.device) if self._net.wt_batch else None


class PatchProj(TokenLinear):
    """The reference's nn.Conv2d(in_channels, hidden_dim, kernel_size=patch, stride=patch): weight [D, Cin, ph, pw] in the arena's OHWI order
    with the input channels padded to a multiple of 4 (the pad weights are zero and stay zero: their inputs are).  Over patch rows in
    (py, px, c) order that storage IS the [D, ph * pw * Cp] matrix of a 1x1 convolution."""

    _param_kinds = {"weight": "conv"}

    def __init__(self, in_channels, hidden_dim, patch_size):
        SgxBlock.__init__(self)
        ph, pw = patch_size
        self.cin, self.cp = in_channels, (in_channels + 3) // 4 * 4
        self.in_features, self.out_features = ph * pw * self.cp, hidden_dim
        self.in_channels, self.out_channels = in_channels, hidden_dim
        self.kernel_size, self.stride, self.padding = 1, 1, 0
        w = torch.empty(hidden_dim, in_channels, ph, pw)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))  # nn.Conv2d default
        self.weight = nn.Parameter(w)
        bound = 1.0 / math.sqrt(in_channels * ph * pw)
        self.bias = nn.Parameter(torch.empty(hidden_dim).uniform_(-bound, bound))
        self._w = self._gw = None

    def _filter_views(self, slot):
        flat = lambda v: v.permute(0, 2, 3, 1).reshape(self.out_features, self.in_features, 1, 1)  # noqa: E731  ([D, Cp, ph, pw] view of [D][ph][pw][Cp])
        w, gw = flat(slot.kernel_view), flat(slot.grad_kernel_view)
        assert w.data_ptr() == slot.kernel_view.data_ptr() and gw.data_ptr() == slot.grad_kernel_view.data_ptr()  # views, not copies
        return w, gw


class PatchEmbed(SgxBlock):
    def __init__(self, img_size, patch_size, in_channels=3, hidden_dim=768):
        super().__init__()
        self.img_size, self.patch_size = tuple(img_size), tuple(patch_size)
        self.grid_size = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = PatchProj(in_channels, hidden_dim, self.patch_size)

    def on_materialize(self):
        pass

    def get_input_channels(self) -> int:
        return self.proj.cin

    def fwd(self, x_nhwc, out=None):
        rows = K.patch_rows(x_nhwc, *self.patch_size)
        self._rows = rows if self.training else None
        return self.proj.conv(rows, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        if need_dx:
            _not_built("the patch embedding is the first layer and returns no input gradient")
        rows, self._rows = self._rows, None
        self.proj.wgrad(rows, dy)


class LayerNorm(SgxBlock):
    """nn.LayerNorm(C, eps) over the channels of every token."""

    def __init__(self, num_features, eps=1e-6):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        if not self.training:
            return K.layernorm_fwd(x, self.weight, self.bias, self.eps, out=out, want_stats=False)
        y, mean, rstd = K.layernorm_fwd(x, self.weight, self.bias, self.eps, out=out)
        self._ctx = (x, mean, rstd)
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x, mean, rstd), self._ctx = self._ctx, None
        return K.layernorm_bwd(dy, x, self.weight, mean, rstd, self.weight.grad, self.bias.grad, addend=addend, out=dx_out)


class Attention(SgxBlock):
    def __init__(self, hidden_dim, heads=8):
        super().__init__()
        self.heads, self.dim_head = heads, hidden_dim // heads
        self.scale = self.dim_head ** -0.5
        self.to_qkv = TokenLinear(hidden_dim, hidden_dim * 3)
        self.proj = TokenLinear(hidden_dim, hidden_dim)

    def on_materialize(self):
        pass

    @staticmethod
    def _slices(t):
        D = t.shape[3] // 3
        return t[..., :D], t[..., D:2 * D], t[..., 2 * D:]

    def fwd(self, n1, out=None, residual=None):
        qkv = self.to_qkv.conv(n1)
        o, lse = K.attn_fwd(*self._slices(qkv), self.heads, self.scale)
        self._ctx = (n1, qkv, o, lse) if self.training else None
        return self.proj.conv(o, out=out, addend=residual)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (n1, qkv, o, lse), self._ctx = self._ctx, None
        self.proj.wgrad(o, dy)
        do = self.proj.dgrad(dy, tuple(o.shape))
        dqkv = torch.empty(qkv.shape, device=qkv.device, dtype=torch.float32)
        K.attn_bwd(*self._slices(qkv), o, do, lse, self.heads, self.scale, *self._slices(dqkv))
        self.to_qkv.wgrad(n1, dqkv)
        return self.to_qkv.dgrad(dqkv, tuple(n1.shape))


class FeedForward(SgxBlock):
    def __init__(self, hidden_dim, mlp_dim):
        super().__init__()
        self.fc1 = TokenLinear(hidden_dim, mlp_dim)
        self.fc2 = TokenLinear(mlp_dim, hidden_dim)

    def on_materialize(self):
        pass

    def fwd(self, n2, out=None, residual=None):
        h = self.fc1.conv(n2)
        self._ctx = (n2, h) if self.training else None
        g = K.gelu_fwd(h, out=None if self.training else h)  # (training keeps the pre-activation; gelu(h) is recomputed in the backward)
        return self.fc2.conv(g, out=out, addend=residual)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (n2, h), self._ctx = self._ctx, None
        self.fc2.wgrad(K.gelu_fwd(h), dy)
        dg = self.fc2.dgrad(dy, tuple(h.shape))
        dh = K.gelu_bwd(dg, h, out=dg)
        self.fc1.wgrad(n2, dh)
        return self.fc1.dgrad(dh, tuple(n2.shape))


class TransformerBlock(SgxBlock):
    def __init__(self, hidden_dim, heads, mlp_dim, dropout_prob=0.0):
        super().__init__()
        self.norm1 = LayerNorm(hidden_dim, eps=1e-6)
        self.attn = Attention(hidden_dim, heads=heads)
        self.norm2 = LayerNorm(hidden_dim, eps=1e-6)
        self.mlp = FeedForward(hidden_dim, mlp_dim)
        self._dropout_prob = float(dropout_prob)

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        if self.training and self._dropout_prob > 0:
            _not_built(f"dropout_prob = {self._dropout_prob} in training mode (the recipes use 0; eval is the identity and works)")
        mid = self.attn.fwd(self.norm1.fwd(x), residual=x)           # attn(norm1(x)) + x
        return self.mlp.fwd(self.norm2.fwd(mid), out=out, residual=mid)  # mlp(norm2(.)) + .

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        d_mid = self.norm2.bwd(self.mlp.bwd(dy), addend=dy)          # the skip's gradient joins in the LayerNorm backward
        return self.norm1.bwd(self.attn.bwd(d_mid), addend=d_mid, dx_out=dx_out)


class Transformer(SgxBlock):
    def __init__(self, hidden_dim, depth, heads, mlp_dim, dropout_prob=0.0):
        super().__init__()
        self.blocks = nn.ModuleList([TransformerBlock(hidden_dim, heads, mlp_dim, dropout_prob=dropout_prob) for _ in range(depth)])

    def on_materialize(self):
        pass


class ViT(SgxClassifier):
    _head_path = _finetune_key = "head"

    def __init__(self, image_size: tuple, patch_size: tuple, num_classes: int, hidden_dim: int, depth: int, heads: int, mlp_dim: int, in_channels=3,
                 dropout_prob=0.0, emb_dropout_prob=0.0, backbone_mode=False):
        super().__init__()
        image_height, image_width = image_size
        patch_height, patch_width = patch_size
        assert image_height % patch_height == 0 and image_width % patch_width == 0, "Image dimensions must be divisible by the patch size."
        assert hidden_dim % heads == 0, "Hidden dimension must be divisible by the number of heads."
        if hidden_dim % 4 or (hidden_dim // heads) % 4:
            _not_built(f"hidden_dim and hidden_dim / heads must be multiples of 4 (16-byte channel groups), got {hidden_dim} / {heads} heads")
        if mlp_dim % 4:
            _not_built(f"mlp_dim must be a multiple of 4 (16-byte channel groups), got {mlp_dim}")
        if hidden_dim // heads > 128:
            _not_built(f"the attention kernels hold head widths up to 128, got {hidden_dim // heads}")
        if not (1 <= in_channels <= 4 or in_channels % 4 == 0):
            _not_built(f"in_channels must be 1..4 (padded to 4 as the stems do) or a multiple of 4, got {in_channels}")
        num_patches = (image_height // patch_height) * (image_width // patch_width)
        self.image_size, self.patch_size = tuple(image_size), tuple(patch_size)
        self.hidden_dim = hidden_dim
        self.patch_embedding = PatchEmbed(img_size=self.image_size, patch_size=self.patch_size, in_channels=in_channels, hidden_dim=hidden_dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, hidden_dim))
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, hidden_dim))
        self.emb_dropout_prob = float(emb_dropout_prob)
        self.transformer = Transformer(hidden_dim, depth, heads, mlp_dim, dropout_prob)
        self.backbone_mode = backbone_mode
        self.pre_head_norm = LayerNorm(hidden_dim, eps=1e-6)
        self.head = LinearLayer(hidden_dim, num_classes)

    # ---- forward / backward --------------------------------------------------------------------------------------
    def _fwd(self, img):
        xh = self._input_nhwc(img)
        if tuple(img.shape[2:]) != self.image_size:
            _not_built(f"the model was built for {self.image_size} images and received {tuple(img.shape[2:])} (the reference slices pos_embedding; no recipe needs it)")
        if self.training and self.emb_dropout_prob > 0:
            _not_built(f"emb_dropout_prob = {self.emb_dropout_prob} in training mode (the recipes use 0; eval is the identity and works)")
        x = K.token_assemble_fwd(self.patch_embedding.fwd(xh), self.cls_token, self.pos_embedding)
        for blk in self.transformer.blocks:
            x = blk.fwd(x)
        self._stream_shape = tuple(x.shape)
        cls = self.pre_head_norm.fwd(x[:, :1])  # LayerNorm is per row: the class-token rows alone
        n = cls.shape[0]
        if self.backbone_mode:
            return (cls.view(n, self.hidden_dim),)
        return (self.head.fwd(cls.view(n, self.hidden_dim)).contiguous(),)

    def _bwd(self, d_out):
        ready = self._bucket_ready
        n, t, _, D = self._stream_shape
        if self.backbone_mode:
            d = d_out.contiguous().view(n, 1, 1, D)
        else:
            d = self.head.bwd(d_out.contiguous()).contiguous().view(n, 1, 1, D)
            ready("head.")
        dx = torch.empty(n, t, 1, D, device=d.device, dtype=torch.float32)
        K.fill(dx, 0.0)  # the last block's output gradient is zero except in the class-token rows
        self.pre_head_norm.bwd(d, dx_out=dx[:, :1])
        ready("pre_head_norm.")
        blocks = self.transformer.blocks
        for i in range(len(blocks) - 1, -1, -1):
            dx = blocks[i].bwd(dx)
            ready(f"transformer.blocks.{i}.")
        K.token_assemble_bwd(dx, self.cls_token.grad, self.pos_embedding.grad)
        self.patch_embedding.bwd(dx[:, 1:], need_dx=False)  # the patch rows' gradient is a view: no copy
        ready("patch_embedding.")
        ready("pos_embedding")
        ready("cls_token")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["cls_token", "pos_embedding", "patch_embedding."] + [f"transformer.blocks.{i}." for i in range(len(self.transformer.blocks))] + \
               ["pre_head_norm.", "head."]

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        """Nothing folds: no BatchNorm, no re-parameterised branch."""
        return self

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.patch_embedding.get_input_channels()


def _variant(name, cls_name, hidden_dim, depth, heads, mlp_dim):
    def init(self, arch_params, num_classes=None, backbone_mode=None):
        ViT.__init__(self, image_size=get_param(arch_params, "image_size", (224, 224)), patch_size=get_param(arch_params, "patch_size", (16, 16)),
                     num_classes=num_classes_of(arch_params, num_classes), hidden_dim=hidden_dim, depth=depth, heads=heads, mlp_dim=mlp_dim,
                     in_channels=get_param(arch_params, "in_channels", 3), dropout_prob=get_param(arch_params, "dropout_prob", 0),
                     emb_dropout_prob=get_param(arch_params, "emb_dropout_prob", 0), backbone_mode=backbone_mode)

    return register_model(name)(type(cls_name, (ViT,), {"__init__": init, "__doc__": f"hidden {hidden_dim}, depth {depth}, {heads} heads, mlp {mlp_dim}"}))


ViTBase = _variant("vit_base", "ViTBase", 768, 12, 12, 3072)
ViTLarge = _variant("vit_large", "ViTLarge", 1024, 24, 16, 4096)
ViTHuge = _variant("vit_huge", "ViTHuge", 1280, 32, 16, 5120)
