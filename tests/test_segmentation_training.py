"""PixelAccuracy / IoU against their definitions (int64 counts, fp64 ratios, restated here), and the regseg48 recipe's loss, metrics and
schedule through Trainer.train.  IoU's definition is the one DESIGN.md 26.4 records."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_segloss_kernels import EPS


def _batches():
    """Two batches of 19-class logits and labels in [0, 19] (19: the ignored label); class 7 is never predicted and never a target."""
    g = torch.Generator().manual_seed(3)
    out = []
    for _ in range(2):
        x, y = torch.randn(2, 19, 5, 7, generator=g), torch.randint(0, 20, (2, 5, 7), generator=g)
        x[:, 7] = -50.0
        y[y == 7] = 8
        out.append((x, y))
    return out


def _pixel_accuracy(batches, ignored):
    pred, lab = torch.cat([x.argmax(1).reshape(-1) for x, _ in batches]), torch.cat([y.reshape(-1) for _, y in batches])
    keep = ~torch.isin(lab, torch.tensor(ignored))
    return np.float64((pred == lab)[keep].sum().item()) / (np.spacing(1) + np.float64(keep.sum().item()))


def _iou(batches, n, ignore):
    pred, lab = torch.cat([x.argmax(1).reshape(-1) for x, _ in batches]), torch.cat([y.reshape(-1) for _, y in batches])
    m = torch.bincount(lab * n + pred, minlength=n * n).reshape(n, n)
    m[ignore] = 0
    inter, union = m.diag().double(), (m.sum(0) + m.sum(1) - m.diag()).double()
    score = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(union))
    assert score[7] == 0 and union[7] == 0  # the absent class scores 0.0 and counts in the mean
    return float(score[[c for c in range(n) if c != ignore]].mean())


@pytest.mark.parametrize("name,kwargs", [("PixelAccuracy", {"ignore_label": 19}), ("PixelAccuracy", {"ignore_label": [0, 19]}),
                                         ("IoU", {"num_classes": 20, "ignore_index": 19})])
def test_segmentation_metric_against_definition(backend, name, kwargs):
    from super_gradients_amd.common.factories import MetricsFactory

    def expected(batches):
        if name == "IoU":
            return _iou(batches, 20, 19)
        return _pixel_accuracy(batches, np.atleast_1d(kwargs["ignore_label"]).tolist())

    batches = _batches()
    m = MetricsFactory().get({name: kwargs})
    assert m.greater_is_better
    m.update(batches[0][0].to(backend), batches[0][1].to(backend))
    m.update((batches[1][0].to(backend), "aux"), batches[1][1].to(backend))  # a tuple prediction: element 0
    assert m.compute() == pytest.approx(expected(batches), rel=1e-15)
    m.reset()
    m.update(batches[1][0].to(backend), batches[1][1].to(backend))
    assert m.compute() == pytest.approx(expected(batches[1:]), rel=1e-15)


@pytest.mark.parametrize("build,error", [(lambda M: M.IoU(20, ignore_index=[0, 19]), NotImplementedError), (lambda M: M.IoU(20, threshold=0.3), NotImplementedError),
                                         (lambda M: M.IoU(20, reduction="none"), NotImplementedError), (lambda M: M.IoU(1), ValueError),
                                         (lambda M: M.PixelAccuracy(metrics_args_prep_fn=lambda p, t: (p, t)), NotImplementedError),
                                         (lambda M: M.PixelAccuracy(ignore_label=[0, 1, 2, 3, 4]), NotImplementedError)])
def test_segmentation_metric_unsupported_options(build, error):
    from super_gradients_amd.training import metrics as M

    with pytest.raises(error):
        build(M)


def test_regseg48_recipe_trains(backend, tmp_path):
    """The settings of recipes/cityscapes_regseg48.yaml that touch the loss, the metrics and the schedule, on one fixed 2 x 3 x 64 x 96 batch
    repeated: two epochs of two batches.  The first step's loss against fp64 F.cross_entropy of the model's own logits at test_segloss_kernels'
    bar (twice ATen's fp32 distance, floor 4 epsilons); the last step's loss below the first's."""
    from super_gradients_amd.training import Trainer, models
    from super_gradients_amd.training.utils.callbacks import Callback

    g = torch.Generator().manual_seed(5)
    batch = (torch.randn(2, 3, 64, 96, generator=g), torch.randint(0, 20, (2, 64, 96), generator=g))
    steps = []

    class Record(Callback):
        def on_train_batch_loss_end(self, context):
            steps.append((context.preds.detach().cpu().clone(), context.loss_log_items.cpu().clone()))

    metrics = [{"PixelAccuracy": {"ignore_label": 19}}, {"IoU": {"num_classes": 20, "ignore_index": 19}}]
    tp = dict(max_epochs=2, lr_mode="PolyLRScheduler", initial_lr=0.02, optimizer="SGD", optimizer_params=dict(momentum=0.9, weight_decay=5e-4),
              loss="CrossEntropyLoss", criterion_params=dict(ignore_index=19), ema=True, ema_params=dict(decay=0.9, decay_type="threshold"),
              train_metrics_list=metrics, valid_metrics_list=metrics, metric_to_watch="IoU", phase_callbacks=[Record()], silent_mode=True, seed=3)
    net = models.get("regseg48", num_classes=19)
    res = Trainer("regseg48", ckpt_root_dir=str(tmp_path)).train(net, tp, [batch, batch], valid_loader=[batch])
    assert len(res) == 2 and len(steps) == 4
    for split in ("train", "valid"):
        row = res[-1][split]
        assert {"CrossEntropyLoss", "PixelAccuracy", "IoU"} <= set(row) and all(np.isfinite(float(row[k])) for k in row)
        assert 0.0 <= row["PixelAccuracy"] <= 1.0 and 0.0 <= row["IoU"] <= 1.0
    logits, loss = steps[0]
    l64, l32 = (F.cross_entropy(logits.to(t), batch[1], ignore_index=19).double() for t in (torch.float64, torch.float32))
    assert (loss.double() - l64).abs() <= max(2 * (l32 - l64).abs(), 4 * EPS * l64.abs())
    assert float(steps[-1][1]) < float(steps[0][1])
