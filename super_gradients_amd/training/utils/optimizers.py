"""Arena optimizers: the seven names the reference's registry resolves (SGD, Adam, AdamW, RMSprop, RMSpropTF, Lamb, Lion) over the
network's flat parameter arena - one kernel launch per step (Lamb: three calls on the stream, per-tensor norms without a host synchronisation).

Reference behaviour mirrored: torch.optim.AdamW / SGD / Adam / RMSprop and training/utils/optimizers/{rmsprop_tf,lamb,lion}.py as built
by training/utils/optimizer_utils.py:88-143 with the zero-weight-decay grouping of :32-59 (BatchNorm affine parameters and every bias get weight_decay 0 when
`zero_weight_decay_on_bias_and_bn`).  They subclass torch.optim.Optimizer, so LR callbacks that write
`param_group["lr"]` (callbacks.py:374-392, 489-514) and `state_dict()` checkpointing keep working.
Dead parameters (QARepVGGBlock.rbr_reparam) are not in the arena and are never touched - torch.optim skips them too,
because they never receive a gradient.
"""
import torch

from ... import kernels as K
from ...common.registry import register_optimizer
from ...modules.engine import SgxNetwork


def _segments(net: SgxNetwork, weight_decay: float, zero_wd_on_bias_bn: bool):
    ends, wds = [], []
    for i, s in enumerate(net.slots):
        end = net.slots[i + 1].start if i + 1 < len(net.slots) else net.p_arena.size
        wd = 0.0 if (zero_wd_on_bias_bn and s.no_wd) else float(weight_decay)
        if wds and wds[-1] == wd:
            ends[-1] = end
        else:
            ends.append(end)
            wds.append(wd)
    dev = net.p_arena.buf.device
    return torch.tensor(ends, dtype=torch.int64, device=dev), torch.tensor(wds, dtype=torch.float32, device=dev)


class _ArenaOptimizer(torch.optim.Optimizer):
    state_names = ()  # the arena-sized state buffers (attributes of the optimizer) a checkpoint carries; a buffer may be None when its option is off
    takes_grad_scale = True  # step(grad_scale=<device scalar>) folds the data-parallel mean into the launch (False: the Trainer scales the arena)

    def __init__(self, net: SgxNetwork, defaults: dict, zero_weight_decay_on_bias_and_bn: bool):
        if not isinstance(net, SgxNetwork):
            raise TypeError("arena optimizers take the network itself (an SgxNetwork), not parameter lists: the step is one kernel over its arena")
        net.materialize()
        self.net = net
        decay = [s.param for s in net.slots if not (zero_weight_decay_on_bias_and_bn and s.no_wd)]
        no_decay = [s.param for s in net.slots if zero_weight_decay_on_bias_and_bn and s.no_wd]
        groups = [{"named_params": None, "params": decay, "name": "decay"}]
        if no_decay:
            groups.insert(0, {"params": no_decay, "weight_decay": 0.0, "name": "no_decay"})
        for g in groups:
            g.pop("named_params", None)
        super().__init__(groups, defaults)
        self._zero_wd = zero_weight_decay_on_bias_and_bn
        self._seg = None
        self._seg_wd_value = None
        self._steps = 0

    def _lr_wd(self):
        lrs = {float(g["lr"]) for g in self.param_groups}
        if len(lrs) != 1:
            raise NotImplementedError("per-group learning rates are not supported by the arena optimizers (one launch over the whole arena)")
        wd = float([g for g in self.param_groups if g.get("name") == "decay"][0]["weight_decay"])
        if self._seg is None or self._seg_wd_value != wd:
            self._seg = _segments(self.net, wd, self._zero_wd)
            self._seg_wd_value = wd
        return lrs.pop(), self._seg

    def zero_grad(self, set_to_none: bool = False):
        self.net.zero_grad()


@register_optimizer("AdamW")
class ArenaAdamW(_ArenaOptimizer):
    state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, zero_weight_decay_on_bias_and_bn=False):
        super().__init__(net, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), zero_weight_decay_on_bias_and_bn)
        n = net.p_arena.buf.numel()
        self.exp_avg = torch.zeros(n, device=net.p_arena.buf.device)
        self.exp_avg_sq = torch.zeros(n, device=net.p_arena.buf.device)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        lr, (seg_end, seg_wd) = self._lr_wd()
        b1, b2 = self.param_groups[0]["betas"]
        self._steps += 1
        K.adamw_step(self.net.p_arena.buf, self.net.g_arena.buf, self.exp_avg, self.exp_avg_sq, lr, b1, b2, self.param_groups[0]["eps"], self._steps,
                     seg_end, seg_wd, grad_scale)


@register_optimizer("SGD")
class ArenaSGD(_ArenaOptimizer):
    state_names = ("momentum_buffer",)
    takes_grad_scale = False

    def __init__(self, net, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, zero_weight_decay_on_bias_and_bn=False):
        super().__init__(net, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov),
                         zero_weight_decay_on_bias_and_bn)
        self.momentum_buffer = torch.zeros(net.p_arena.buf.numel(), device=net.p_arena.buf.device)

    @torch.no_grad()
    def step(self, closure=None):
        lr, (seg_end, seg_wd) = self._lr_wd()
        g = self.param_groups[0]
        self._steps += 1
        K.sgd_step(self.net.p_arena.buf, self.net.g_arena.buf, self.momentum_buffer, lr, g["momentum"], g["dampening"], g["nesterov"],
                   self._steps == 1, seg_end, seg_wd)


def _zeros(net, fill=0.0):
    return torch.full((net.p_arena.buf.numel(),), fill, dtype=torch.float32, device=net.p_arena.buf.device)


@register_optimizer("Adam")
class ArenaAdam(_ArenaOptimizer):
    """torch.optim.Adam: L2 weight decay added to the gradient, bias correction."""

    state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, zero_weight_decay_on_bias_and_bn=False):
        if amsgrad:
            raise NotImplementedError("Adam(amsgrad=True) is not available on the HIP path: the arena kernel keeps no running maximum of exp_avg_sq")
        super().__init__(net, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False), zero_weight_decay_on_bias_and_bn)
        self.exp_avg, self.exp_avg_sq = _zeros(net), _zeros(net)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        lr, (seg_end, seg_wd) = self._lr_wd()
        g = self.param_groups[0]
        self._steps += 1
        K.adam_step(self.net.p_arena.buf, self.net.g_arena.buf, self.exp_avg, self.exp_avg_sq, lr, g["betas"][0], g["betas"][1], g["eps"], self._steps,
                    seg_end, seg_wd, grad_scale)


class _ArenaRMSpropBase(_ArenaOptimizer):
    state_names = ("square_avg", "grad_avg", "momentum_buffer")
    _tf = False

    def _init_state(self, net, momentum, centered, square_avg_init):
        self.square_avg = _zeros(net, square_avg_init)
        self.grad_avg = _zeros(net) if centered else None  # (state only for what is enabled)
        self.momentum_buffer = _zeros(net) if momentum > 0 else None

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        lr, (seg_end, seg_wd) = self._lr_wd()
        g = self.param_groups[0]
        if (g["momentum"] > 0) != (self.momentum_buffer is not None) or bool(g["centered"]) != (self.grad_avg is not None):
            raise ValueError("momentum / centered cannot be switched after construction: their state buffers exist only when enabled")
        self._steps += 1
        K.rmsprop_step(self.net.p_arena.buf, self.net.g_arena.buf, self.square_avg, self.grad_avg, self.momentum_buffer, lr, g["alpha"], g["eps"],
                       g["momentum"], seg_end, seg_wd, tf=self._tf, decoupled_decay=bool(g.get("decoupled_decay", False)),
                       lr_in_momentum=bool(g.get("lr_in_momentum", False)), grad_scale=grad_scale)


@register_optimizer("RMSprop")
class ArenaRMSprop(_ArenaRMSpropBase):
    """torch.optim.RMSprop: eps outside the square root, square_avg*alpha + (1-alpha) g^2, learning rate at the parameter update."""

    def __init__(self, net, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, zero_weight_decay_on_bias_and_bn=False):
        for name, v in (("learning rate", lr), ("epsilon value", eps), ("momentum value", momentum), ("weight_decay value", weight_decay), ("alpha value", alpha)):
            if not 0.0 <= v:
                raise ValueError(f"Invalid {name}: {v}")
        super().__init__(net, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay), zero_weight_decay_on_bias_and_bn)
        self._init_state(net, momentum, centered, 0.0)


@register_optimizer("RMSpropTF")
class ArenaRMSpropTF(_ArenaRMSpropBase):
    """training/utils/optimizers/rmsprop_tf.py: eps inside the square root, square_avg starts at ones, avg += (1-alpha)(g^2 - avg),
    optional decoupled decay, learning rate accumulated in the momentum buffer (lr_in_momentum)."""

    _tf = True

    def __init__(self, net, lr=1e-2, alpha=0.9, eps=1e-10, weight_decay=0, momentum=0.0, centered=False, decoupled_decay=False, lr_in_momentum=True,
                 zero_weight_decay_on_bias_and_bn=False):
        for name, v in (("learning rate", lr), ("epsilon value", eps), ("momentum value", momentum), ("weight_decay value", weight_decay), ("alpha value", alpha)):
            if not 0.0 <= v:
                raise ValueError(f"Invalid {name}: {v}")
        super().__init__(net, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                                   decoupled_decay=decoupled_decay, lr_in_momentum=lr_in_momentum), zero_weight_decay_on_bias_and_bn)
        self._init_state(net, momentum, centered, 1.0)


@register_optimizer("Lion")
class ArenaLion(_ArenaOptimizer):
    """training/utils/optimizers/lion.py: one state buffer; decay, sign step, momentum - in that order."""

    state_names = ("exp_avg",)

    def __init__(self, net, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, zero_weight_decay_on_bias_and_bn=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        super().__init__(net, dict(lr=lr, betas=betas, weight_decay=weight_decay), zero_weight_decay_on_bias_and_bn)
        self.exp_avg = _zeros(net)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        lr, (seg_end, seg_wd) = self._lr_wd()
        b1, b2 = self.param_groups[0]["betas"]
        self._steps += 1
        K.lion_step(self.net.p_arena.buf, self.net.g_arena.buf, self.exp_avg, lr, b1, b2, seg_end, seg_wd, grad_scale)


@register_optimizer("Lamb")
class ArenaLamb(_ArenaOptimizer):
    """training/utils/optimizers/lamb.py: global gradient-norm clip, Adam moments, a per-tensor trust ratio |p| / |update| on tensors with weight
    decay (all tensors with always_adapt).  The per-tensor norms are reduced on the device in a fixed order (csrc/optim.hip); `trust` holds the
    last step's ratios, one per arena slot.  With a grad_scale (data parallel) every norm is that of the MEAN gradient.  The gradient arena is
    not written: the reference divides p.grad by the clip factor in place, the Trainer zeroes the arena right after the step."""

    state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, net, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True, max_grad_norm=1.0,
                 trust_clip=False, always_adapt=False, zero_weight_decay_on_bias_and_bn=False):
        super().__init__(net, dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay, grad_averaging=grad_averaging,
                                   max_grad_norm=max_grad_norm, trust_clip=trust_clip, always_adapt=always_adapt), zero_weight_decay_on_bias_and_bn)
        self.exp_avg, self.exp_avg_sq = _zeros(net), _zeros(net)
        dev = net.p_arena.buf.device
        ends = [s.start for s in net.slots[1:]] + [net.p_arena.buf.numel()]
        self.slot_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self.trust = torch.ones(len(ends), dtype=torch.float32, device=dev)
        self._ws = K.lamb_workspace(net.p_arena.buf.numel(), len(ends), dev)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        lr, (seg_end, seg_wd) = self._lr_wd()
        g = self.param_groups[0]
        self._steps += 1
        K.lamb_step(self.net.p_arena.buf, self.net.g_arena.buf, self.exp_avg, self.exp_avg_sq, lr, g["betas"][0], g["betas"][1], g["eps"],
                    self._steps if g["bias_correction"] else 0, seg_end, seg_wd, self.slot_end, self._ws, self.trust, grad_averaging=g["grad_averaging"],
                    max_grad_norm=self.defaults["max_grad_norm"], trust_clip=g["trust_clip"], always_adapt=g["always_adapt"], grad_scale=grad_scale)


def build_optimizer(net, lr: float, training_params) -> torch.optim.Optimizer:
    """optimizer_utils.py:88-143: `optimizer` is one of the registry's names (any letter case) with `optimizer_params`,
    `zero_weight_decay_on_bias_and_bn`."""
    from .utils import get_param

    name = get_param(training_params, "optimizer", "SGD")
    if not isinstance(name, str):
        return name  # an already-built optimizer
    zero = bool(get_param(training_params, "zero_weight_decay_on_bias_and_bn", False))
    cls = {k.lower(): v for k, v in OPTIMIZERS.items()}.get(name.lower())
    if cls is None:
        raise NotImplementedError(f"optimizer '{name}' is not available on the HIP path ({', '.join(OPTIMIZERS)})")
    # optimizer_utils.py:23-29,104-106: the recipe's optimizer_params are laid over per-optimizer defaults (SGD, RMSprop, RMSpropTF: weight decay
    # 1e-4 and momentum 0.9 - not the classes' zeros; Adam: weight decay 1e-4; AdamW, Lamb and Lion have no entry there and keep the classes' own
    # defaults), and the merged dictionary is written back
    params = dict(OPTIMIZERS_DEFAULT_PARAMS.get(cls, {}))
    params.update(get_param(training_params, "optimizer_params", {}) or {})
    if hasattr(training_params, "override"):
        training_params.override(optimizer_params=dict(params))
    elif isinstance(training_params, dict):
        training_params["optimizer_params"] = dict(params)
    return cls(net, lr=lr, zero_weight_decay_on_bias_and_bn=zero, **params)


OPTIMIZERS = {"SGD": ArenaSGD, "Adam": ArenaAdam, "AdamW": ArenaAdamW, "RMSprop": ArenaRMSprop, "RMSpropTF": ArenaRMSpropTF, "Lamb": ArenaLamb,
              "Lion": ArenaLion}  # common/object_names.py Optimizers
OPTIMIZERS_DEFAULT_PARAMS = {  # training/params.py:88-94, optimizer_utils.py:23-29
    ArenaSGD: {"weight_decay": 1e-4, "momentum": 0.9},
    ArenaAdam: {"weight_decay": 1e-4},
    ArenaRMSprop: {"weight_decay": 1e-4, "momentum": 0.9},
    ArenaRMSpropTF: {"weight_decay": 1e-4, "momentum": 0.9},
}
