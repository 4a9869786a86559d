"""The Python side of semantic-segmentation fine-tuning without a device: ``ConvertToSemanticSamInputs``' records, the argument checks of
``SemanticSamTrainer``, ``CustomDiceLoss`` and ``_compute_loss`` against the closed form (tests/semantic_loss_ref.py in fp64) for
``dice_weight`` in None, 0, 0.3 and 1 with the device call replaced by the host build of csrc/semloss.hip (so the autograd function, the
weights and the statistics run as they do on the device), a whole train step of a toy model, and ``SemanticMapsSamTrainer``'s argument
order.  tests/test_gpu_semantic_training.py trains the real model on the device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import semantic_loss_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_semantic_trainer")), ROOT, files=["semloss.hip"])
    lib.msam_semantic_loss_workspace_bytes.restype = C.c_int64
    lib.emu_last_error.restype = C.c_char_p
    return lib


@pytest.fixture()
def host_loss(lib, monkeypatch):
    """``ops.semantic_loss`` / ``ops.semantic_loss_backward`` on host tensors through the host build of the same entry points."""
    from micro_sam_amd import _semloss, ops
    vp = C.c_void_p
    calls = {"forward": 0, "backward": 0}

    def args(logits, target, dw, cw, softmax):
        assert logits.dtype == torch.float32 and logits.is_contiguous() and target.dtype == torch.int32 and target.is_contiguous()
        b, c, h, w = logits.shape
        assert target.numel() == b * h * w
        return b, c, h * w, (vp(logits.data_ptr()), vp(target.data_ptr()), b, c, h * w, C.c_float(dw), C.c_float(cw), int(softmax),
                             C.c_double(_semloss.SEMLOSS_EPS))

    def forward(logits, target, dice_weight=1.0, ce_weight=1.0, softmax=True):
        target = _semloss.class_ids(target)
        b, c, hw, a = args(logits, target, dice_weight, ce_weight, softmax)
        need = int(lib.msam_semantic_loss_workspace_bytes(b, c, hw))
        ws = torch.empty(need // 8 + 1, dtype=torch.int64)
        loss, raw = torch.empty((), dtype=torch.float32), torch.empty(3 * c + 5, dtype=torch.int64)
        rc = lib.msam_semantic_loss_forward(*a, vp(ws.data_ptr()), C.c_int64(need), vp(loss.data_ptr()), vp(raw.data_ptr()), None)
        assert rc == 0, lib.emu_last_error().decode()
        calls["forward"] += 1
        return loss, _semloss.stats_views(raw, c)

    def backward(logits, target, stats, grad_output, dice_weight=1.0, ce_weight=1.0, softmax=True):
        raw = stats.raw if isinstance(stats, _semloss.SemanticLossStats) else stats
        _, _, _, a = args(logits, target, dice_weight, ce_weight, softmax)
        assert grad_output.dtype == torch.float32 and grad_output.numel() == 1
        out = torch.empty_like(logits)
        rc = lib.msam_semantic_loss_backward(*a, vp(raw.data_ptr()), vp(grad_output.data_ptr()), vp(out.data_ptr()), None)
        assert rc == 0, lib.emu_last_error().decode()
        calls["backward"] += 1
        return out
    monkeypatch.setattr(ops, "semantic_loss", forward)
    monkeypatch.setattr(ops, "semantic_loss_backward", backward)
    return calls


class Toy(nn.Module):
    """A model without ``image_embeddings_oft``: three class maps from a 1 x 1 convolution of the image."""

    def __init__(self, classes=3):
        super().__init__()
        torch.manual_seed(0)
        self.conv = nn.Conv2d(3, classes, 1)

    def forward(self, batched_inputs, multimask_output=False):
        assert multimask_output is True
        return [{"masks": self.conv(rec["image"][None])} for rec in batched_inputs]


def trainer(dice_weight=None, cls=None, classes=3, **kw):
    from micro_sam_amd.training import ConvertToSemanticSamInputs, SemanticSamTrainer
    model = Toy(classes)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    return (cls or SemanticSamTrainer)(ConvertToSemanticSamInputs(), classes, dice_weight, model=model, optimizer=opt, device="cpu", **kw)


def data(classes=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 3, 12, 10, generator=g)
    y = torch.randint(0, classes, (2, 1, 12, 10), generator=g)
    return x, y


def test_convert_to_semantic_sam_inputs():
    from micro_sam_amd.training import ConvertToSemanticSamInputs
    x, y = data()
    recs = ConvertToSemanticSamInputs()(x, y)
    assert len(recs) == 2
    for rec, image in zip(recs, x):
        assert set(rec) == {"image", "original_size"} and rec["image"] is not None and torch.equal(rec["image"], image)
        assert tuple(rec["original_size"]) == (12, 10)


def test_trainer_argument_checks():
    from micro_sam_amd.training import ConvertToSemanticSamInputs, SemanticSamTrainer
    for bad in (1, 0, -3, 2.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            SemanticSamTrainer(ConvertToSemanticSamInputs(), bad, model=Toy(), optimizer=torch.optim.SGD(Toy().parameters(), lr=0.1))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="between 0 and 1"):
            trainer(dice_weight=bad)
    with pytest.raises(TypeError, match="model="):
        SemanticSamTrainer(ConvertToSemanticSamInputs(), 3, optimizer=None)
    with pytest.raises(TypeError, match="train_loader"):
        trainer(train_loader=[])
    t = trainer(classes=3)
    with pytest.raises(ValueError, match="channels"):
        t._compute_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 4, 4, 4))
    for ok in (None, 0, 0.3, 1):
        assert trainer(dice_weight=ok).dice_weight == ok


@pytest.mark.parametrize("dice_weight", [None, 0, 0.3, 1])
def test_compute_loss_is_the_closed_form(host_loss, dice_weight):
    t = trainer(dice_weight)
    g = torch.Generator().manual_seed(1)
    masks = (2.0 * torch.randn(2, 3, 12, 10, generator=g)).requires_grad_()
    _, y = data(seed=2)
    y[0, 0, 3, :] = -100
    wd, wc = (1.0, 1.0) if dice_weight is None else (dice_weight, 1 - dice_weight)
    want = R.loss_and_gradient(masks.detach().numpy(), y[:, 0].numpy(), torch.float64, wd, wc)
    yard = R.loss_and_gradient(masks.detach().numpy(), y[:, 0].numpy(), torch.float32, wd, wc)
    bl, bg, _, _ = R.bounds(want, yard)
    loss = t._compute_loss(y, masks)
    loss.backward()
    assert host_loss == {"forward": 1, "backward": 1}                      # ONE fused call each way
    assert abs(float(loss.detach()) - want["loss"]) <= bl
    assert np.abs(masks.grad.double().numpy() - want["grad"]).max() <= bg
    d, ce = t.last_parts
    assert abs(float(d) - want["dice"]) <= bl and abs(float(ce) - want["ce"]) <= bl


def test_custom_dice_loss_is_the_dice_part(host_loss):
    from micro_sam_amd.training import CustomDiceLoss
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(2, 4, 9, 7, generator=g).requires_grad_()
    y = torch.randint(0, 4, (2, 1, 9, 7), generator=g)
    for softmax in (True, False):
        want = R.loss_and_gradient(pred.detach().numpy(), y[:, 0].numpy(), torch.float64, 1.0, 0.0, softmax)
        yard = R.loss_and_gradient(pred.detach().numpy(), y[:, 0].numpy(), torch.float32, 1.0, 0.0, softmax)
        bl, bg, _, _ = R.bounds(want, yard)
        pred.grad = None
        loss = CustomDiceLoss(4, softmax=softmax)(pred, y)
        loss.backward()
        assert loss.shape == () and abs(float(loss.detach()) - want["dice"]) <= bl and abs(want["dice"] - want["loss"]) == 0
        assert np.abs(pred.grad.double().numpy() - want["grad"]).max() <= bg
    with pytest.raises(ValueError, match="CustomDiceLoss"):
        CustomDiceLoss(3)(pred, y)


def test_a_users_loss_takes_the_two_term_form(host_loss):
    """``loss=``: the reference's formulation, that loss plus torch's cross-entropy - here with the torch composite as the loss."""
    _, y = data(seed=2)
    g = torch.Generator().manual_seed(1)
    masks = torch.randn(2, 3, 12, 10, generator=g)

    def dice_composite(pred, target):
        return R.dice(torch.softmax(pred, dim=1), R.one_hot(target, 3).float())
    for w in (None, 0.3):
        fused = float(trainer(w)._compute_loss(y, masks))
        composite = float(trainer(w, loss=dice_composite)._compute_loss(y, masks))
        print(w, fused, composite)
        assert abs(fused - composite) <= 4 * float(np.spacing(np.float32(fused)))
    assert host_loss["forward"] == 2                                      # the user's loss does not go through the fused call


def test_train_iteration_record_and_validate(host_loss):
    t = trainer(0.3)
    x, y = data()
    before = [p.detach().clone() for p in t.model.parameters()]
    rec = t.train_iteration(x, y)
    assert set(rec) == {"iteration", "loss", "dice_loss", "ce_loss", "allreduce_bytes"} and rec["iteration"] == 0 and rec["allreduce_bytes"] == 0
    assert abs(rec["loss"] - (0.3 * rec["dice_loss"] + 0.7 * rec["ce_loss"])) <= 4 * float(np.spacing(np.float32(rec["loss"])))
    assert all(not torch.equal(a, b) for a, b in zip(before, t.model.parameters()))
    t.fit(2, [(x, y)])
    assert [r["iteration"] for r in t.history] == [0, 1, 2] and t.history[2]["loss"] < t.history[0]["loss"]
    calls = dict(host_loss)
    metric = t.validate([(x, y), (x, y)])
    assert host_loss["forward"] == calls["forward"] + 2 and host_loss["backward"] == calls["backward"]
    assert np.isfinite(metric) and t.last_metric == 1 - metric / 3
    with pytest.raises(ValueError, match="empty"):
        t.validate([])


def test_checkpoint_round_trip(host_loss, tmp_path):
    t = trainer()
    x, y = data()
    t.fit(2, [(x, y)])
    path = str(tmp_path / "semantic.pt")
    t.save_checkpoint(path, note=7)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert state["iteration"] == 2 and state["note"] == 7 and set(state["model_state"]) == {"conv.weight", "conv.bias"}
    kept = [p.detach().clone() for p in t.model.parameters()]
    with torch.no_grad():
        for p in t.model.parameters():
            p.zero_()
    t._iteration = 0
    t.load_checkpoint(path)
    assert t._iteration == 2 and all(torch.equal(a, b) for a, b in zip(kept, t.model.parameters()))


def test_semantic_maps_trainer_argument_order():
    from micro_sam_amd.training import SemanticMapsSamTrainer
    seen = []

    def loss(a, b):
        seen.append((a, b))
        return (b * 0.5).sum()
    t = trainer(cls=SemanticMapsSamTrainer, loss=loss)
    masks = torch.ones(2, 3, 4, 4)
    y = torch.zeros(2, 3, 4, 4)
    out = t._compute_loss(y, masks)
    assert float(out) == 48.0 and len(seen) == 1 and torch.equal(seen[0][0], y) and seen[0][1] is masks
