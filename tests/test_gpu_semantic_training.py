"""``SemanticSamTrainer`` on the device: two iterations on two 64 x 64 images with three-class label images (synthetic vit_b, image encoder
and prompt encoder frozen so that the test stays within seconds; the mask decoder trains).  The records against the torch composite on
the masks the trainer saw (the bound of tests/semantic_loss_ref.py), the fused default against ``loss=`` with the torch composite, which
parameters move, validation under ``no_grad`` on the promptless records (the decoder without a tape and without a sparse token), the
checkpoint round trip, and two runs from the same seeds."""
import random

import numpy as np
import pytest
import torch

import semantic_loss_ref as R

pytestmark = pytest.mark.gpu
ITERATIONS = 2


def _data():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:64, :64]
    labels = np.stack([(xx > 20).astype(np.int64) + (xx + yy > 80), (yy > 30).astype(np.int64) + ((xx - 32) ** 2 + (yy - 32) ** 2 < 150)])
    image = np.clip(60 + 70 * labels + rng.normal(0, 8, labels.shape), 0, 255).astype(np.float32)
    x = torch.as_tensor(image)[:, None].repeat(1, 3, 1, 1)
    return x, torch.as_tensor(labels)[:, None]


def _dice_composite(pred, target):
    """The reference's ``CustomDiceLoss`` with torch operators."""
    return R.dice(torch.softmax(pred, dim=1), R.one_hot(target, 3).float())


def _run(sd, x, y, **kw):
    """Two iterations from fixed seeds -> (trainer, the masks every ``_compute_loss`` saw, parameters before, parameters after)."""
    from micro_sam_amd import util
    from micro_sam_amd.training import ConvertToSemanticSamInputs, SemanticSamTrainer, TrainableSAM
    np.random.seed(3); random.seed(3); torch.manual_seed(3)
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=sd)
    model = TrainableSAM(predictor.model)
    for n, p in model.sam.named_parameters():
        p.requires_grad_(n.startswith("mask_decoder."))
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    trainer = SemanticSamTrainer(ConvertToSemanticSamInputs(), 3, model=model, optimizer=opt, **kw)
    seen = []
    inner = trainer._compute_loss

    def compute_loss(y_, masks):
        seen.append(masks.detach().clone())
        return inner(y_, masks)
    trainer._compute_loss = compute_loss
    before = {n: p.detach().clone() for n, p in model.sam.named_parameters()}
    trainer.fit(ITERATIONS, [(x, y)])
    after = {n: p.detach().clone() for n, p in model.sam.named_parameters()}
    return trainer, seen, before, after


@pytest.fixture(scope="module")
def runs(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    x, y = _data()
    return x, y, _run(vit_b_sd, x, y), _run(vit_b_sd, x, y), _run(vit_b_sd, x, y, loss=_dice_composite)


def _reference(masks, y):
    m, t = masks.cpu().numpy(), y[:, 0].numpy()
    want = R.loss_and_gradient(m, t, torch.float64)
    yard = R.loss_and_gradient(m, t, torch.float32, device="cuda")
    return want, R.bounds(want, yard)


def test_records_equal_the_composite_on_the_masks(runs):
    x, y, (trainer, seen, before, after), _, _ = runs
    assert set(np.unique(y.numpy())) == {0, 1, 2} and len(seen) == ITERATIONS and seen[0].shape == (2, 3, 64, 64)
    assert [r["iteration"] for r in trainer.history] == list(range(ITERATIONS))
    for rec, masks in zip(trainer.history, seen):
        want, (bl, _, yl, _) = _reference(masks, y)
        print(rec, "composite fp64:", want["loss"], want["dice"], want["ce"], "bound", bl, "composite's own error", yl)
        assert set(rec) == {"iteration", "loss", "dice_loss", "ce_loss", "allreduce_bytes"}
        assert all(np.isfinite(rec[k]) for k in ("loss", "dice_loss", "ce_loss"))
        assert abs(rec["loss"] - want["loss"]) <= bl and abs(rec["dice_loss"] - want["dice"]) <= bl and abs(rec["ce_loss"] - want["ce"]) <= bl
    moved = [n for n in before if not torch.equal(before[n], after[n])]
    assert moved and all(n.startswith("mask_decoder.") for n in moved)
    trained = [n for n in before if n.startswith("mask_decoder.")]
    print(len(moved), "of", len(trained), "mask decoder tensors moved")
    assert len(moved) >= len(trained) // 2


def test_a_users_torch_composite_gives_the_same_first_loss(runs):
    x, y, (fused, seen, _, _), _, (composite, seen_c, _, _) = runs
    assert torch.equal(seen[0], seen_c[0])                                # the same model on the same input
    want, (bl, _, yl, _) = _reference(seen[0], y)
    a, b = fused.history[0], composite.history[0]
    print("fused", a, "composite", b, "bound", bl)
    for k in ("loss", "dice_loss", "ce_loss"):
        assert abs(a[k] - want[k.replace("_loss", "")]) <= bl and abs(b[k] - want[k.replace("_loss", "")]) <= bl
        assert abs(a[k] - b[k]) <= 2 * bl


def test_two_runs_from_the_same_seed_give_the_same_record(runs):
    _, _, (a, seen_a, _, after_a), (b, seen_b, _, after_b), _ = runs
    assert a.history == b.history
    assert all(torch.equal(p, q) for p, q in zip(seen_a, seen_b))
    assert all(torch.equal(after_a[n], after_b[n]) for n in after_a)


def test_validate_without_a_tape_and_checkpoint_round_trip(runs, tmp_path):
    x, y, (trainer, seen, _, _), _, _ = runs
    calls = []
    inner = trainer.model.sam.mask_decoder.forward

    def spy(*a, **k):
        calls.append(torch.is_grad_enabled())
        return inner(*a, **k)
    trainer.model.sam.mask_decoder.forward = spy
    try:
        metric = trainer.validate([(x, y)])
    finally:
        del trainer.model.sam.mask_decoder.forward
    print("validation metric:", metric, "score:", trainer.last_metric)
    assert calls == [False, False]                                        # both records through the inference decoder, no tape
    want, (bl, _, _, _) = _reference(seen[-1], y)                          # (the masks the validation pass gave to ``_compute_loss``)
    assert np.isfinite(metric) and abs(metric - want["loss"]) <= bl and trainer.last_metric == 1 - metric / 3
    assert metric == trainer.validate([(x, y)])
    path = str(tmp_path / "semantic.pt")
    trainer.save_checkpoint(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert state["iteration"] == ITERATIONS and any(k.startswith("sam.mask_decoder.") for k in state["model_state"])
    name, p = next((n, p) for n, p in trainer.model.named_parameters() if n.startswith("sam.mask_decoder.iou_token"))
    kept = p.detach().clone()
    with torch.no_grad():
        p.zero_()
    trainer._iteration = 0
    trainer.load_checkpoint(path)
    assert torch.equal(p, kept) and trainer._iteration == ITERATIONS
    assert metric == trainer.validate([(x, y)])                           # (the inference decoder's operand copies follow the parameters)
