"""``models.simple_sam_3d_wrapper`` on the device: the convolutional decoder alone (``decoders`` + ``out_conv``) on random features
against a fresh fp64 restatement from ``F.conv3d``, ``F.instance_norm``, ``F.leaky_relu`` and ``F.interpolate`` - forward and every
parameter gradient - and ``SemanticSamTrainer`` steps of a ``SimpleSam3DWrapper`` on the two-block test encoder of
tests/test_gpu_sam3d.py with D = 2 and four classes."""
import hashlib
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_sam3d import _small_encoder

pytestmark = pytest.mark.gpu
CLASSES, DEPTH = 4, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def restate_decoder(sd, x, rd):
    """The decoder with torch's own operators, channels-first, in the dtype of ``sd`` and ``x``: x [B, 256, D, h, w] -> logits
    [B, classes, D, 16 h, 16 w].  ``rd`` is applied to both operands of every convolution (identity, or rounding to bf16)."""
    def conv(t, name, padding):
        return F.conv3d(rd(t), rd(sd[name + ".weight"]), sd[name + ".bias"], padding=padding)

    def norm(t):
        return F.instance_norm(t, eps=1e-5)
    for i in range(4):
        p = f"decoders.{i}."
        residual = norm(conv(x, p + "downsample.0", 0))
        out = F.leaky_relu(norm(conv(x, p + "conv1.0", 1)), 0.01)
        out = norm(conv(out, p + "conv2.0", 1))
        x = F.interpolate(F.leaky_relu(out + residual, 0.01), scale_factor=(1, 2, 2), mode="nearest")
    x = F.leaky_relu(norm(conv(x, "out_conv.conv_pred.0", 1)), 0.01)
    return conv(x, "out_conv.segmentation_head", 0)


@pytest.mark.parametrize("shape", [(1, 256, 2, 4, 4), (2, 256, 1, 2, 3)], ids=str)
def test_decoder_and_gradients_against_the_fp64_restatement(dev, shape):
    """The error of the decoder is the rounding of the convolution operands to bf16, which has no derivable bound.  The yardstick is
    therefore measured: the SAME restatement run in fp32 with both operands of every convolution rounded to bf16, against its fp64 self;
    the product may be 4 times as far from the fp64 restatement.  Errors are l2 norms of the difference (the ratio of two
    of them is the ratio of the relative errors).

    Measured on an MI355X: profiles/r10_simple_sam3d.md."""
    from micro_sam_amd.models.simple_sam_3d_wrapper import BasicBlock, SegmentationHead
    torch.manual_seed(0)
    model = torch.nn.Module()
    model.decoders = torch.nn.ModuleList([BasicBlock(256, 128), BasicBlock(128, 64), BasicBlock(64, 32), BasicBlock(32, 16)])
    model.out_conv = SegmentationHead(16, 5)
    model.to(dev)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(*shape, generator=g).to(dev)
    B, _, D, h, w = shape
    gout = torch.randn(B, 5, D, 16 * h, 16 * w, generator=g).to(dev)
    out = feats.permute(0, 2, 3, 4, 1)
    for block in model.decoders:
        out = block(out)
    out = model.out_conv(out).permute(0, 4, 1, 2, 3)
    assert out.shape == gout.shape
    (out * gout).sum().backward()
    got = {k: p.grad for k, p in model.named_parameters()}
    assert len(got) == 28 and all(v is not None for v in got.values())

    def run(dtype, rd):
        sd = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in model.state_dict().items()}
        with torch.backends.cudnn.flags(enabled=False):
            o = restate_decoder(sd, feats.to(dtype), rd)
            (o * gout.to(dtype)).sum().backward()
        return o.detach(), {k: v.grad for k, v in sd.items()}
    want, want_g = run(torch.float64, lambda t: t)
    yard, yard_g = run(torch.float32, lambda t: t.to(torch.bfloat16).to(torch.float32))

    def errs(mine, yardstick, ref):
        ref = ref.detach().double()
        return (mine.detach().double() - ref).norm().item(), (yardstick.detach().double() - ref).norm().item(), ref.norm().item()
    figures = {"logits": errs(out, yard, want)}
    for k in got:
        figures[k] = errs(got[k], yard_g[k], want_g[k])
    # (a bias in front of an InstanceNorm has a gradient of exactly zero: there both errors are rounding noise and `scale` is ~ 0)
    for k, (mine, yardstick, scale) in figures.items():
        print(f"{k}: |product - fp64| {mine:.3e}, |fp32 restatement with bf16 operands - fp64| {yardstick:.3e}, |fp64| {scale:.3e}, "
              f"ratio {mine / yardstick:.2f}")
    for k, (mine, yardstick, scale) in figures.items():
        assert yardstick > 0, k
        assert mine <= 4 * yardstick, (k, mine, yardstick)


def _data():
    rng = np.random.default_rng(0)
    zz, yy, xx = np.mgrid[:DEPTH, :64, :64]
    labels = (xx > 20).astype(np.int64) + (xx + yy + 8 * zz > 80) + (yy > 50)
    image = np.clip(40 + 60 * labels + rng.normal(0, 8, labels.shape), 0, 255).astype(np.float32)
    return torch.as_tensor(image)[None, None].repeat(1, 3, 1, 1, 1), torch.as_tensor(labels)[None, None]       # [1, 3, D, H, W], [1, 1, D, H, W]


def _train(dev, freeze_encoder: bool, steps: int = 2):
    from micro_sam_amd import modeling
    from micro_sam_amd.models.simple_sam_3d_wrapper import SimpleSam3DWrapper
    from micro_sam_amd.training import ConvertToSemanticSamInputs, SemanticSamTrainer
    np.random.seed(3); random.seed(3); torch.manual_seed(3)
    sam = modeling.Sam(_small_encoder(), modeling.PromptEncoder(), modeling.MaskDecoder())
    model = SimpleSam3DWrapper(sam, num_classes=CLASSES, freeze_encoder=freeze_encoder).to(dev)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = torch.optim.AdamW([p for n, p in model.named_parameters() if p.requires_grad and not n.startswith(("sam.prompt_", "sam.mask_"))],
                            lr=1e-3)
    trainer = SemanticSamTrainer(ConvertToSemanticSamInputs(), CLASSES, model=model, optimizer=opt, device=dev)
    x, y = _data()
    records = [trainer.train_iteration(x, y) for _ in range(steps)]
    digest = hashlib.sha256()
    for _, p in sorted(model.named_parameters()):
        digest.update(p.detach().cpu().numpy().tobytes())
    return model, before, records, digest.hexdigest()


def test_semantic_trainer_steps_on_the_simple_3d_model(dev):
    model, before, records, digest = _train(dev, freeze_encoder=True)
    assert all(np.isfinite(r["loss"]) and np.isfinite(r["dice_loss"]) and np.isfinite(r["ce_loss"]) for r in records)
    assert records[1]["loss"] < records[0]["loss"]                          # a fixed batch
    for n, p in model.named_parameters():
        if n.startswith("sam.image_encoder."):
            assert not p.requires_grad and p.grad is None and torch.equal(p, before[n]), n      # a frozen encoder gets no gradient
        elif n.startswith(("decoders.", "out_conv.")):
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
            if n.endswith(".weight"):
                assert float(p.grad.abs().sum()) > 0 and not torch.equal(p, before[n]), n       # the decoder's parameters change
    # the same seed, a fresh model: the same parameters after two steps, bit for bit
    assert _train(dev, freeze_encoder=True)[3] == digest
    with torch.no_grad():
        x, _ = _data()
        out = model([{"image": x[0], "original_size": (64, 64)}], multimask_output=True)
    assert len(out) == 1 and out[0]["masks"].shape == (1, CLASSES, DEPTH, 64, 64) and torch.isfinite(out[0]["masks"]).all()


def test_a_trained_encoder_gets_gradients(dev):
    model, _, records, _ = _train(dev, freeze_encoder=False, steps=1)
    assert np.isfinite(records[0]["loss"])
    enc = [(n, p) for n, p in model.named_parameters() if n.startswith("sam.image_encoder.")]
    assert enc and all(p.grad is not None and torch.isfinite(p.grad).all() for _, p in enc)
    assert any(float(p.grad.abs().sum()) > 0 for _, p in enc)
