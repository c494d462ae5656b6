"""The contract every classifier family gets from modules/classifier.py's SgxClassifier - input check, head replacement, fine-tuning
dictionary - and the one it keeps writing itself (gradient_buckets), on one small model per family.  CPU only: construction, plus the
host emulation where a forward or a materialised model is needed."""
import pytest
import torch

V3 = dict(width_mult=1.0, mode="small", structure=[[3, 1, 16, 1, 0, 2], [5, 4, 24, 1, 1, 1], [5, 3, 24, 0, 1, 1]])
ANYNET = dict(ls_num_blocks=[1, 2], ls_block_width=[24, 48], ls_bottleneck_ratio=[1, 1], ls_group_width=[8, 8], stride=2, se_ratio=4, dropout_prob=0.5)


def _get(name, **arch):
    from super_gradients_amd.training import models

    return models.get(name, arch_params=arch, num_classes=10)


def _resnet():
    from super_gradients_amd.training.models.classification_models.resnet import BasicResNetBlock, ResNet

    return ResNet(BasicResNetBlock, [1, 1, 1, 1], num_classes=10, width_mult=0.25)


def _resnext():
    from super_gradients_amd.training.models.classification_models.resnext import ResNeXt

    return ResNeXt([1, 1, 1, 1], 4, 4, num_classes=10)


def _vit():
    from super_gradients_amd.training.models.classification_models.vit import ViT

    return ViT(image_size=(32, 32), patch_size=(8, 8), num_classes=10, hidden_dim=64, depth=2, heads=4, mlp_dim=128)


def _beit():
    from super_gradients_amd.training.models.classification_models.beit import Beit

    return Beit(image_size=(32, 32), patch_size=(8, 8), num_classes=10, embed_dim=64, depth=2, num_heads=4, mlp_ratio=2, use_abs_pos_emb=False,
                use_rel_pos_bias=True, init_values=0.1)


# family: (constructor, dotted path of the replaced linear layer, the module(s) whose parameters are the classification head - written out here,
# not derived from the key under test -, image size)
FAMILIES = {
    "resnet": (_resnet, "linear", "linear", 32),
    "resnext": (_resnext, "fc", "fc", 32),
    "repvgg": (lambda: _get("repvgg_custom", struct=[1, 1, 1, 1], width_multiplier=[0.25, 0.25, 0.25, 0.25]), "linear", "linear", 32),
    "mobilenetv2": (lambda: _get("custom_mobilenet_v2", width_mult=1.0, structure=[[1, 16, 1, 1], [6, 24, 1, 2]]), "classifier.1", "classifier.1", 32),
    "mobilenetv3": (lambda: _get("mobilenet_v3_custom", **V3), "classifier.3", ("classifier.0", "classifier.3"), 32),
    "regnet": (lambda: _get("custom_anynet", **ANYNET), "net.head.fc", "net.head", 32),
    "efficientnet": (lambda: _get("CustomizedEfficientnet", width_coefficient=0.5, depth_coefficient=0.3, res=32, dropout_rate=0.2), "_fc", "_fc", 32),
    "vit": (_vit, "head", "head", 32),
    "beit": (_beit, "head", "head", 32),
    "densenet": (lambda: _get("custom_densenet", growth_rate=8, structure=[2, 3, 2], num_init_features=16, bn_size=2), "classifier", "classifier", 32),
    "shufflenetv2": (lambda: _get("shufflenet_v2_custom5", structure=[2, 3, 2], stages_out_channels=[8, 16, 32, 64, 128]), "fc", "fc", 32),
}
family = pytest.mark.parametrize("name", list(FAMILIES))


@family
def test_is_a_classifier_and_overrides_nothing_the_base_owns(name):
    from super_gradients_amd.modules.classifier import SgxClassifier

    net = FAMILIES[name][0]()
    assert isinstance(net, SgxClassifier)
    mro = type(net).__mro__
    for cls in mro[: mro.index(SgxClassifier)]:
        assert "replace_head" not in cls.__dict__ and "supports_half_inference" not in cls.__dict__, cls.__name__
    assert net.supports_half_inference() is False


@family
def test_replace_head(name):
    build, head_path, _, _ = FAMILIES[name]
    net = build()
    with pytest.raises(ValueError):
        net.replace_head()
    with pytest.raises(NotImplementedError):
        net.replace_head(new_head=object())
    before = {k: v.clone() for k, v in net.state_dict().items()}
    in_features = net.get_submodule(head_path).in_features
    net.replace_head(new_num_classes=7)
    head = net.get_submodule(head_path)
    assert head.out_features == 7 and head.in_features == in_features
    after = net.state_dict()
    assert set(after) == set(before)
    for k, v in after.items():
        if k.startswith(head_path + "."):
            assert v.shape[0] == 7, k
        else:
            assert torch.equal(v, before[k]), f"{k} changed with the head"


@family
def test_materialized_model_refuses_a_new_head_and_a_wrong_channel_count(name):
    import emu_env

    build, _, _, size = FAMILIES[name]
    net = build()
    cin = net.get_input_channels()
    emu_env.activate()
    try:
        net.materialize(torch.device("cpu")).eval()
        with pytest.raises(RuntimeError):
            net.replace_head(new_num_classes=7)
        with pytest.raises(ValueError, match=f"expected an NCHW batch with {cin} channels"):
            net(torch.zeros(2, cin + 1, size, size))
        with pytest.raises(ValueError, match=f"expected an NCHW batch with {cin} channels"):
            net(torch.zeros(cin, size, size))
    finally:
        emu_env.deactivate()


@family
def test_finetune_lr_dict_names_the_head(name):
    build, _, head_modules, _ = FAMILIES[name]
    head_modules = (head_modules,) if isinstance(head_modules, str) else head_modules
    net = build()
    d = net.get_finetune_lr_dict(0.1)
    assert set(d) - {"default"} and len(d) == 2 and d["default"] == 0
    (key,) = set(d) - {"default"}
    assert d[key] == 0.1
    names = [n for n, _ in net.named_parameters()]
    head = [n for n in names if any(n.startswith(m + ".") for m in head_modules)]
    assert len(head) == 2 * len(head_modules), "the table's head modules: a weight and a bias each"
    assert all(n.startswith(key) for n in head)
    assert not any(n.startswith(key) for n in names if n not in head)


@family
def test_gradient_buckets_partition_the_parameters_in_order(name):
    net = FAMILIES[name][0]()
    buckets = net.gradient_buckets()
    seen = []
    for n, _ in net.named_parameters():
        owners = [i for i, b in enumerate(buckets) if n.startswith(b)]
        assert len(owners) == 1, f"{n} starts with {len(owners)} bucket prefixes"
        if not seen or seen[-1] != owners[0]:
            seen.append(owners[0])
    assert seen == list(range(len(buckets))), f"buckets {buckets} against the parameter order: {seen}"
