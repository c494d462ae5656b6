"""BEiT classifiers on the HIP kernels.

Reference: training/models/classification_models/beit.py - Mlp (:118-138), gen_relative_position_index (:141-164), Attention (:167-230), Block
(:233-273), RelativePositionBias (:276-290), Beit (:293-465) and the registered BeitBasePatch16_224 / BeitLargePatch16_224 (:468-494).  Same
constructor arguments and defaults, the reference's initial distributions (truncated normal, std 0.02; fix_init_weight's 1 / sqrt(2 layer)
rescale; head_init_scale; gamma = init_values) and the same state_dict keys, shapes and order (cls_token, [pos_embed], patch_embed.proj.*,
[rel_pos_bias.*], blocks.{i}: gamma_1, gamma_2, norm1.*, attn.q_bias / v_bias / relative_position_bias_table / relative_position_index /
qkv.weight / proj.*, norm2.*, mlp.fc1 / fc2.*, then norm.* or fc_norm.*, head.*), so checkpoints interchange both ways.

What BEiT adds to the ViT sequence (vit.py; DESIGN.md 20 counts the passes):
    attention   s_ij = scale q_i k_j + table[index(i, j)][h] inside the attention kernels (sgx_attn_rpb_*): the table column sits in LDS, the
                index is computed from the token grid, the table's gradient is binned inside the dq pass.  relative_position_index stays a
                persistent int64 buffer for checkpoint parity and is only CHECKED against the closed form (materialize, load_state_dict:
                ValueError if it differs) - the kernels never read it.
    qkv bias    q_bias and v_bias are parameters, k_bias a constant zero (a non-persistent buffer).  The bias-free qkv filter runs with a packed
                [3D] bias (q_bias, 0, v_bias) refreshed by two device copies per forward; the q and v thirds of the bias gradient are column
                sums of the dqkv slices, the k third is dropped (zero mathematically: softmax is shift-invariant along a row).
    layer scale x + m_b (gamma * branch(x)) in one sweep (sgx_layerscale_*), m the per-image stochastic-depth multiplier (0 or 1 / keep; block i
                of depth runs at linspace(0, drop_path_rate, depth)[i], training only, one draw per branch).  Without gamma and without drop
                path the branch rides the projection's addend as in ViT and no layer-scale launch happens.  The [B] multipliers are
                sgx_dropout_fwd on a row of ones seeded from torch's default generator; `Block._test_keep_masks` injects masks for the tests.
    head        global_pool = "avg": mean over the patch tokens (sgx_token_mean_*) -> fc_norm -> head; otherwise norm on the class-token rows
                only -> head.
    tokens      use_abs_pos_emb = False: the token assembly runs without a position embedding.

Stored per block for the backward beside ViT's: the two branch outputs (2 D floats per token, dgamma's operand) when layer scale is on.

Not built (each raises NotImplementedError): drop_rate / attn_drop_rate > 0 in training mode (eval is the identity), set_grad_checkpointing(True),
replace_head(new_head=...), widths or head widths that are not multiples of 4, head widths above 128, an input size other than the constructed
one, use_rel_pos_bias together with use_shared_rel_pos_bias; supports_half_inference() is False.
"""
import math

import torch
from torch import nn

from .... import kernels as K
from ....common.registry import register_model
from ....modules.classifier import SgxClassifier
from ....modules.engine import SgxBlock
from ....modules.layers import LinearLayer
from ...utils.utils import HpmStruct
from .vit import FeedForward, LayerNorm, PatchEmbed, TokenLinear


def _not_built(msg):
    raise NotImplementedError(f"BEiT on the HIP path: {msg}")


def _trunc_normal(t, std=0.02):
    return nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2.0, b=2.0)


def relative_position_index(grid) -> torch.Tensor:
    """index(i, j) over the tokens of a gh x gw grid behind one class token - the closed form the attention kernels compute:
    N - 1 for i = j = 0, N - 3 for i = 0, N - 2 for j = 0, otherwise (y_i - y_j + gh - 1)(2 gw - 1) + (x_i - x_j + gw - 1)."""
    gh, gw = grid
    n = K.rpb_rows(grid)
    tok = torch.arange(gh * gw)
    y, x = torch.div(tok, gw, rounding_mode="floor"), tok % gw
    idx = torch.empty(gh * gw + 1, gh * gw + 1, dtype=torch.int64)
    idx[1:, 1:] = (y[:, None] - y[None, :] + gh - 1) * (2 * gw - 1) + (x[:, None] - x[None, :] + gw - 1)
    idx[0, :] = n - 3
    idx[:, 0] = n - 2
    idx[0, 0] = n - 1
    return idx


def _check_index(buf, grid, name):
    if buf.device.type == "meta":
        return
    if tuple(buf.shape) != (grid[0] * grid[1] + 1,) * 2 or not torch.equal(buf.cpu(), relative_position_index(grid)):
        raise ValueError(f"{name} differs from the relative position index of a {grid[0]} x {grid[1]} token grid: the attention kernels compute the "
                         "index in closed form and would apply another bias than this checkpoint's")


class RelativePositionBias(SgxBlock):
    """The table shared by all blocks (use_shared_rel_pos_bias)."""

    def __init__(self, window_size, num_heads):
        super().__init__()
        self.window_size = tuple(window_size)
        self.relative_position_bias_table = nn.Parameter(torch.zeros(K.rpb_rows(self.window_size), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(self.window_size))

    def on_materialize(self):
        pass


class Attention(SgxBlock):
    def __init__(self, dim, num_heads=8, qkv_bias=False, window_size=None):
        super().__init__()
        self.num_heads, self.dim = num_heads, dim
        self.scale = (dim // num_heads) ** -0.5
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(dim))
            self.register_buffer("k_bias", torch.zeros(dim), persistent=False)
            self.v_bias = nn.Parameter(torch.zeros(dim))
        else:
            self.q_bias = self.k_bias = self.v_bias = None
        self.window_size = tuple(window_size) if window_size else None
        if self.window_size:
            self.relative_position_bias_table = nn.Parameter(torch.zeros(K.rpb_rows(self.window_size), num_heads))
            self.register_buffer("relative_position_index", relative_position_index(self.window_size))
        else:
            self.relative_position_bias_table = self.relative_position_index = None
        self.qkv = TokenLinear(dim, dim * 3, bias=False)
        self.proj = TokenLinear(dim, dim)

    def on_materialize(self):
        # the launch's bias operand [3D] = (q_bias, 0, v_bias): the middle third is written here, once, and never again
        self._packed = torch.zeros(3 * self.dim, device=self._net._device, dtype=torch.float32) if self.q_bias is not None else None

    @staticmethod
    def _slices(t):
        D = t.shape[3] // 3
        return t[..., :D], t[..., D:2 * D], t[..., 2 * D:]

    def fwd(self, n1, out=None, residual=None, shared=None, grid=None):
        D = self.dim
        if self._packed is not None:
            self._packed[:D].copy_(self.q_bias.data)
            self._packed[2 * D:].copy_(self.v_bias.data)
        qkv = K.conv2d_fwd(n1, self.qkv._w, bias=self._packed, stride=1, pad=0)
        table = self.relative_position_bias_table if self.relative_position_bias_table is not None else shared
        if table is not None:
            o, lse = K.attn_rpb_fwd(*self._slices(qkv), self.num_heads, self.scale, table.data, self.window_size or grid)
        else:
            o, lse = K.attn_fwd(*self._slices(qkv), self.num_heads, self.scale)
        self._ctx = (n1, qkv, o, lse, table, self.window_size or grid) if self.training else None
        return self.proj.conv(o, out=out, addend=residual)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (n1, qkv, o, lse, table, grid), self._ctx = self._ctx, None
        D = self.dim
        self.proj.wgrad(o, dy)
        do = self.proj.dgrad(dy, tuple(o.shape))
        dqkv = torch.empty(qkv.shape, device=qkv.device, dtype=torch.float32)
        if table is not None:  # (a shared table: every block adds onto the same gradient view, in backward order)
            K.attn_rpb_bwd(*self._slices(qkv), o, do, lse, self.num_heads, self.scale, table.data, grid, *self._slices(dqkv), table.grad)
        else:
            K.attn_bwd(*self._slices(qkv), o, do, lse, self.num_heads, self.scale, *self._slices(dqkv))
        if self.q_bias is not None:
            dq, _, dv = self._slices(dqkv)
            gq, gv = self.q_bias.grad, self.v_bias.grad
            self._net.fork_side(lambda: (K.colsum(dq, gq), K.colsum(dv, gv)), dqkv)
        self.qkv.wgrad(n1, dqkv)
        return self.qkv.dgrad(dqkv, tuple(n1.shape))


class Block(SgxBlock):
    _test_keep_masks = None  # tests only: a pair of [B] keep masks (0 / 1) the next training forward uses instead of its own Philox draws

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, drop=0.0, attn_drop=0.0, drop_path=0.0, init_values=None, window_size=None):
        super().__init__()
        if init_values:
            self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
            self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))
        else:
            self.gamma_1 = self.gamma_2 = None
        self.norm1 = LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, window_size=window_size)
        self.norm2 = LayerNorm(dim, eps=1e-6)
        self.mlp = FeedForward(dim, int(dim * mlp_ratio))
        self._drop, self._attn_drop, self._drop_path = float(drop), float(attn_drop), float(drop_path)
        self._last_multipliers = None

    def on_materialize(self):
        pass

    def _multipliers(self, n, dev):
        """Two [B] rows of 0 or 1 / keep (one per branch), or (None, None) outside training / at rate 0"""
        p = self._drop_path
        if not self.training or p <= 0:
            return None, None
        if self._test_keep_masks is not None:
            ms = tuple(torch.as_tensor(k, dtype=torch.float32, device=dev).view(n) * (1.0 / (1.0 - p)) for k in self._test_keep_masks)
        else:
            np4 = (n + 3) // 4 * 4
            seeds = torch.randint(0, 2 ** 62, (2,))  # torch's default generator: torch.manual_seed repeats a step
            ms = tuple(K.dropout(torch.ones(1, np4, device=dev), p, int(s)).view(np4)[:n] for s in seeds)
        self._last_multipliers = ms
        return ms

    def fwd(self, x, out=None, shared=None, grid=None):
        if self.training and (self._drop > 0 or self._attn_drop > 0):
            _not_built(f"drop_rate = {self._drop} / attn_drop_rate = {self._attn_drop} in training mode (the recipes use 0; eval is the identity and works)")
        m1, m2 = self._multipliers(x.shape[0], x.device)
        n1 = self.norm1.fwd(x)
        if self.gamma_1 is None and m1 is None:  # the branch rides the projection's addend: no layer-scale launch
            mid = self.attn.fwd(n1, residual=x, shared=shared, grid=grid)
            y = self.mlp.fwd(self.norm2.fwd(mid), out=out, residual=mid)
            self._ctx = (None, None, None, None) if self.training else None
            return y
        t1 = self.attn.fwd(n1, shared=shared, grid=grid)
        mid = K.layerscale_fwd(x, t1, self.gamma_1, m1)
        t2 = self.mlp.fwd(self.norm2.fwd(mid))
        y = K.layerscale_fwd(mid, t2, self.gamma_2, m2, out=out)
        self._ctx = (t1, t2, m1, m2) if self.training else None
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (t1, t2, m1, m2), self._ctx = self._ctx, None
        if t1 is None:
            d_mid = self.norm2.bwd(self.mlp.bwd(dy), addend=dy)
            return self.norm1.bwd(self.attn.bwd(d_mid), addend=d_mid, dx_out=dx_out)
        g1, g2 = (self.gamma_1, self.gamma_2) if self.gamma_1 is not None else (None, None)
        dt2 = K.layerscale_bwd(dy, t2, g2, m2, g2.grad if g2 is not None else None)
        d_mid = self.norm2.bwd(self.mlp.bwd(dt2), addend=dy)  # the skip's gradient is dy itself: it joins in the LayerNorm backward
        dt1 = K.layerscale_bwd(d_mid, t1, g1, m1, g1.grad if g1 is not None else None)
        return self.norm1.bwd(self.attn.bwd(dt1), addend=d_mid, dx_out=dx_out)


class Beit(SgxClassifier):
    _head_path = _finetune_key = "head"

    def __init__(self, image_size=(224, 224), patch_size=16, in_chans=3, num_classes=1000, global_pool="avg", embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, qkv_bias=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, init_values=None, use_abs_pos_emb=True,
                 use_rel_pos_bias=False, use_shared_rel_pos_bias=False, head_init_scale=0.001, **kwargs):
        super().__init__()
        image_size = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        assert image_size[0] % patch_size[0] == 0 and image_size[1] % patch_size[1] == 0, "Image dimensions must be divisible by the patch size."
        if use_rel_pos_bias and use_shared_rel_pos_bias:
            _not_built("use_rel_pos_bias together with use_shared_rel_pos_bias (two tables added to one score; no registered variant does)")
        if embed_dim % num_heads or embed_dim % 4 or (embed_dim // num_heads) % 4 or int(embed_dim * mlp_ratio) % 4:
            _not_built(f"embed_dim, embed_dim / num_heads and the mlp width must be multiples of 4 (16-byte channel groups), got {embed_dim} / {num_heads} "
                       f"heads, mlp {int(embed_dim * mlp_ratio)}")
        if embed_dim // num_heads > 128:
            _not_built(f"the attention kernels hold head widths up to 128, got {embed_dim // num_heads}")
        if not (1 <= in_chans <= 4 or in_chans % 4 == 0):
            _not_built(f"in_chans must be 1..4 (padded to 4 as the stems do) or a multiple of 4, got {in_chans}")
        self.num_classes, self.global_pool = num_classes, global_pool
        self.num_features = self.embed_dim = embed_dim
        self.grad_checkpointing = False
        self.image_size, self.patch_size = image_size, patch_size
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, (image_size[0] // patch_size[0]) * (image_size[1] // patch_size[1]) + 1, embed_dim)) if use_abs_pos_emb else None
        self.patch_embed = PatchEmbed(img_size=image_size, patch_size=patch_size, in_channels=in_chans, hidden_dim=embed_dim)
        grid = self.patch_embed.grid_size
        if (use_rel_pos_bias or use_shared_rel_pos_bias) and K.rpb_rows(grid) > 4096:
            _not_built(f"a {grid[0]} x {grid[1]} token grid has {K.rpb_rows(grid)} relative positions; the attention kernels stage up to 4096 in LDS")
        self.drop_rate = float(drop_rate)
        self.rel_pos_bias = RelativePositionBias(window_size=grid, num_heads=num_heads) if use_shared_rel_pos_bias else None
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, depth, device="cpu")]  # stochastic depth decay rule (the reference's fp32 values)
        self.blocks = nn.ModuleList([Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate, attn_drop=attn_drop_rate,
                                           drop_path=dpr[i], init_values=init_values, window_size=grid if use_rel_pos_bias else None) for i in range(depth)])
        use_fc_norm = self.global_pool == "avg"
        self.norm = nn.Identity() if use_fc_norm else LayerNorm(embed_dim, eps=1e-6)
        self.fc_norm = LayerNorm(embed_dim, eps=1e-6) if use_fc_norm else None
        self.head = LinearLayer(embed_dim, num_classes)
        self._head_init_scale = head_init_scale
        self._init_weights()

    def _init_weights(self):
        """The reference's: every nn.Linear weight truncated normal (std 0.02) with a zero bias - the patch filter keeps nn.Conv2d's default -
        then fix_init_weight and the head's scale."""
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, TokenLinear) and m is not self.patch_embed.proj:
                    _trunc_normal(m.weight)
                    if m.bias is not None:
                        m.bias.zero_()
            if self.pos_embed is not None:
                _trunc_normal(self.pos_embed)
            _trunc_normal(self.cls_token)
            for layer_id, blk in enumerate(self.blocks):
                blk.attn.proj.weight.div_(math.sqrt(2.0 * (layer_id + 1)))
                blk.mlp.fc2.weight.div_(math.sqrt(2.0 * (layer_id + 1)))
            self._init_head()

    def _init_head(self):
        with torch.no_grad():
            _trunc_normal(self.head.weight)
            self.head.weight.mul_(self._head_init_scale)
            self.head.bias.zero_()

    # ---- the index buffers: kept for checkpoint parity, checked against what the kernels compute -------------------------
    def _check_indices(self):
        for name, m in self.named_modules():
            buf = getattr(m, "relative_position_index", None)
            if isinstance(buf, torch.Tensor):
                _check_index(buf, m.window_size, f"{name}.relative_position_index")

    def materialize(self, device=None):
        if not self._materialized:
            self._check_indices()
        return super().materialize(device)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._check_indices()
        return out

    # ---- forward / backward --------------------------------------------------------------------------------------
    def _fwd(self, img):
        xh = self._input_nhwc(img)
        if tuple(img.shape[2:]) != self.image_size:
            _not_built(f"the model was built for {self.image_size} images and received {tuple(img.shape[2:])}")
        if self.training and self.drop_rate > 0:
            _not_built(f"drop_rate = {self.drop_rate} in training mode (the recipes use 0; eval is the identity and works)")
        x = K.token_assemble_fwd(self.patch_embed.fwd(xh), self.cls_token, self.pos_embed)
        shared = self.rel_pos_bias.relative_position_bias_table if self.rel_pos_bias is not None else None
        grid = self.patch_embed.grid_size
        for blk in self.blocks:
            x = blk.fwd(x, shared=shared, grid=grid)
        self._stream_shape = tuple(x.shape)
        n = x.shape[0]
        if self.fc_norm is not None:
            feat = self.fc_norm.fwd(K.token_mean_fwd(x))
        else:
            feat = self.norm.fwd(x[:, :1])  # LayerNorm is per row: the class-token rows alone
        return (self.head.fwd(feat.view(n, self.embed_dim)).contiguous(),)

    def _bwd(self, d_out):
        ready = self._bucket_ready
        n, t, _, D = self._stream_shape
        d = self.head.bwd(d_out.contiguous()).contiguous().view(n, 1, 1, D)
        ready("head.")
        if self.fc_norm is not None:
            dx = K.token_mean_bwd(self.fc_norm.bwd(d), t)  # the whole gradient: a zero class-token row, d / (T - 1) elsewhere
            ready("fc_norm.")
        else:
            dx = torch.empty(n, t, 1, D, device=d.device, dtype=torch.float32)
            K.fill(dx, 0.0)  # the last block's output gradient is zero except in the class-token rows
            self.norm.bwd(d, dx_out=dx[:, :1])
            ready("norm.")
        for i in range(len(self.blocks) - 1, -1, -1):
            dx = self.blocks[i].bwd(dx)
            ready(f"blocks.{i}.")
        if self.rel_pos_bias is not None:
            ready("rel_pos_bias.")  # every block has added onto the shared table's gradient
        K.token_assemble_bwd(dx, self.cls_token.grad, self.pos_embed.grad if self.pos_embed is not None else None)
        self.patch_embed.bwd(dx[:, 1:], need_dx=False)  # the patch rows' gradient is a view: no copy
        ready("patch_embed.")
        if self.pos_embed is not None:
            ready("pos_embed")
        ready("cls_token")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["cls_token"] + (["pos_embed"] if self.pos_embed is not None else []) + ["patch_embed."] + \
               (["rel_pos_bias."] if self.rel_pos_bias is not None else []) + [f"blocks.{i}." for i in range(len(self.blocks))] + \
               ["fc_norm." if self.fc_norm is not None else "norm.", "head."]

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        """Nothing folds: no BatchNorm, no re-parameterised branch."""
        return self

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def no_weight_decay(self):
        nwd = {"pos_embed", "cls_token"}
        for n, _ in self.named_parameters():
            if "relative_position_bias_table" in n:
                nwd.add(n)
        return nwd

    def set_grad_checkpointing(self, enable=True):
        if enable:
            _not_built("set_grad_checkpointing(True): the blocks keep their backward contexts (DESIGN.md 20.3)")
        self.grad_checkpointing = False

    def get_classifier(self):
        return self.head

    def _new_head(self, new_num_classes):
        super()._new_head(new_num_classes)  # (nn.Linear's default distribution, as the reference's replacement)
        self.num_classes = new_num_classes

    def replace_input_channels(self, in_channels: int, compute_new_weights_fn=None):
        if self._materialized:
            raise RuntimeError("replace_input_channels must be called before the model is materialized in HBM")
        if not (1 <= in_channels <= 4 or in_channels % 4 == 0):
            _not_built(f"in_chans must be 1..4 (padded to 4 as the stems do) or a multiple of 4, got {in_channels}")
        self.patch_embed = PatchEmbed(img_size=self.image_size, patch_size=self.patch_size, in_channels=in_channels, hidden_dim=self.embed_dim)

    def get_input_channels(self) -> int:
        return self.patch_embed.get_input_channels()


def _variant(name, cls_name, **defaults):
    def init(self, arch_params=None, **overrides):
        model_kwargs = HpmStruct(**defaults)
        model_kwargs.override(**(arch_params.to_dict() if hasattr(arch_params, "to_dict") else dict(arch_params or {})))
        model_kwargs.override(**{k: v for k, v in overrides.items() if v is not None})
        Beit.__init__(self, **model_kwargs.to_dict())

    return register_model(name)(type(cls_name, (Beit,), {"__init__": init, "__doc__": ", ".join(f"{k} {v}" for k, v in defaults.items())}))


BeitBasePatch16_224 = _variant("beit_base_patch16_224", "BeitBasePatch16_224", patch_size=(16, 16), embed_dim=768, depth=12, num_heads=12, mlp_ratio=4,
                               use_abs_pos_emb=False, use_rel_pos_bias=True, init_values=0.1)
BeitLargePatch16_224 = _variant("beit_large_patch16_224", "BeitLargePatch16_224", patch_size=(16, 16), embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4,
                                qkv_bias=True, use_abs_pos_emb=False, use_rel_pos_bias=True, init_values=1e-5)
