"""``models.simple_sam_3d_wrapper`` without a device: the reference's ``state_dict`` keys and shapes for two class counts, which
parameters train under ``freeze_encoder`` and LoRA, the refusals, and the COMPOSITION of the channels-last decoder - with the
``functional`` primitives replaced by torch stand-ins - against a channels-first restatement from ``nn.Conv3d``, ``nn.InstanceNorm3d``,
``nn.LeakyReLU`` and ``nn.Upsample``.  The kernels themselves run in tests/test_conv3d_host.py and tests/test_instnorm_host.py, the model
on the device in tests/test_gpu_simple_sam3d.py."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from micro_sam_amd import modeling
from micro_sam_amd.training import functional as HF

CHANNELS = [(256, 128), (128, 64), (64, 32), (32, 16)]


def small_sam():
    torch.manual_seed(0)
    return modeling.Sam(modeling.ImageEncoderViT(embed_dim=64, depth=2, num_heads=2, global_attn_indexes=(1,)), modeling.PromptEncoder(),
                        modeling.MaskDecoder())


def decoder_keys(n_classes: int):
    want = {}
    for i, (ci, co) in enumerate(CHANNELS):
        want[f"decoders.{i}.conv1.0.weight"], want[f"decoders.{i}.conv1.0.bias"] = (co, ci, 3, 3, 3), (co,)
        want[f"decoders.{i}.conv2.0.weight"], want[f"decoders.{i}.conv2.0.bias"] = (co, co, 3, 3, 3), (co,)
        want[f"decoders.{i}.downsample.0.weight"], want[f"decoders.{i}.downsample.0.bias"] = (co, ci, 1, 1, 1), (co,)
    want["out_conv.conv_pred.0.weight"], want["out_conv.conv_pred.0.bias"] = (8, 16, 3, 3, 3), (8,)
    want["out_conv.segmentation_head.weight"], want["out_conv.segmentation_head.bias"] = (n_classes, 8, 1, 1, 1), (n_classes,)
    return want


@pytest.mark.parametrize("n_classes", [2, 5])
def test_state_dict_keys_and_shapes_are_the_references(n_classes):
    from micro_sam_amd.models.simple_sam_3d_wrapper import BasicBlock, SegmentationHead, SimpleSam3DWrapper
    sam = small_sam()
    sam_keys = {"sam." + k: tuple(v.shape) for k, v in sam.state_dict().items()}
    model = SimpleSam3DWrapper(sam, num_classes=n_classes, freeze_encoder=False)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = decoder_keys(n_classes)
    assert len(want) == 28                                                  # 4 blocks of 3 convolutions, 2 in the head: weight and bias
    assert got == {**sam_keys, **want}
    assert all(isinstance(b, BasicBlock) for b in model.decoders) and isinstance(model.out_conv, SegmentationHead)
    assert all(p.requires_grad for p in model.parameters())


def test_freeze_and_lora_requires_grad_pattern(monkeypatch):
    from micro_sam_amd import util
    from micro_sam_amd.models import peft_sam
    from micro_sam_amd.models.simple_sam_3d_wrapper import SimpleSam3DWrapper, get_simple_sam_3d_model
    frozen = SimpleSam3DWrapper(small_sam(), num_classes=3, freeze_encoder=True)
    assert all(p.requires_grad != n.startswith("sam.image_encoder.") for n, p in frozen.named_parameters())
    assert any(n.startswith("sam.image_encoder.") for n, _ in frozen.named_parameters())
    seen = {}

    def fake_get_sam_model(model_type, device, checkpoint_path, return_sam, flexible_load_checkpoint, peft_kwargs, state_dict):
        seen.update(model_type=model_type, peft_kwargs=peft_kwargs, flexible=flexible_load_checkpoint, return_sam=return_sam)
        sam = small_sam()
        if peft_kwargs:
            sam = peft_sam.PEFT_Sam(sam, **peft_kwargs).sam
        return None, sam
    monkeypatch.setattr(util, "get_sam_model", fake_get_sam_model)
    lora = get_simple_sam_3d_model("cpu", n_classes=7, image_size=1024, lora_rank=4, freeze_encoder=True)        # LoRA overrides the freeze
    assert seen["peft_kwargs"] == {"rank": 4, "peft_module": peft_sam.LoRASurgery} and seen["flexible"] and seen["return_sam"]
    assert lora.freeze_encoder is False and lora.out_conv.segmentation_head.weight.shape[0] == 7
    for n, p in lora.named_parameters():
        in_enc = n.startswith("sam.image_encoder.")
        assert p.requires_grad == ((not in_enc) or ".w_a_linear_" in n or ".w_b_linear_" in n), n
    assert any(".attn.qkv.w_a_linear_q." in n for n, _ in lora.named_parameters())
    plain = get_simple_sam_3d_model("cpu", n_classes=2, image_size=1024, freeze_encoder=True)
    assert seen["peft_kwargs"] == {} and plain.freeze_encoder is True
    assert not any(p.requires_grad for p in plain.sam.image_encoder.parameters())
    assert all(p.requires_grad for n, p in plain.named_parameters() if n.startswith(("decoders.", "out_conv.")))


def test_refusals():
    from micro_sam_amd.models.simple_sam_3d_wrapper import get_simple_sam_3d_model
    with pytest.raises(NotImplementedError, match="build_sam"):
        get_simple_sam_3d_model("cpu", n_classes=3, image_size=512)
    with pytest.raises(ValueError, match="vit_t"):
        get_simple_sam_3d_model("cpu", n_classes=3, image_size=1024, model_type="vit_t")
    with pytest.raises(ValueError, match="n_classes"):
        get_simple_sam_3d_model("cpu", n_classes=0, image_size=1024)


def restate_decoder(sd, x):
    """The reference's decoder from torch's modules, channels-first: x [B, 256, D, h, w] -> logits [B, classes, D, 16 h, 16 w]."""
    norm, act, up = nn.InstanceNorm3d(1), nn.LeakyReLU(), nn.Upsample(scale_factor=(1, 2, 2), mode="nearest")
    for i in range(4):
        p = f"decoders.{i}."
        residual = norm(F.conv3d(x, sd[p + "downsample.0.weight"], sd[p + "downsample.0.bias"]))
        out = act(norm(F.conv3d(x, sd[p + "conv1.0.weight"], sd[p + "conv1.0.bias"], padding=1)))
        out = norm(F.conv3d(out, sd[p + "conv2.0.weight"], sd[p + "conv2.0.bias"], padding=1))
        x = up(act(out + residual))
    x = act(norm(F.conv3d(x, sd["out_conv.conv_pred.0.weight"], sd["out_conv.conv_pred.0.bias"], padding=1)))
    return F.conv3d(x, sd["out_conv.segmentation_head.weight"], sd["out_conv.segmentation_head.bias"])


def conv_stand_in(x, weight, bias=None):
    return F.conv3d(x.permute(0, 4, 1, 2, 3), weight, bias, padding=1).permute(0, 2, 3, 4, 1)


def norm_stand_in(a, residual=None, negative_slope=0.01, eps=1e-5):
    def norm(t):
        return F.instance_norm(t.permute(0, 4, 1, 2, 3), eps=eps).permute(0, 2, 3, 4, 1)
    y = norm(a) if residual is None else norm(a) + norm(residual)
    return y if negative_slope is None else F.leaky_relu(y, negative_slope)


def test_the_channels_last_decoder_is_the_references_composition(monkeypatch):
    from micro_sam_amd.models.simple_sam_3d_wrapper import SimpleSam3DWrapper
    monkeypatch.setattr(HF, "linear", lambda x, w, b=None: F.linear(x, w, b))
    monkeypatch.setattr(HF, "conv3d_k3", conv_stand_in)
    monkeypatch.setattr(HF, "instance_norm_act", norm_stand_in)
    model = SimpleSam3DWrapper(small_sam(), num_classes=5, freeze_encoder=True).double()
    feats = torch.randn(2, 256, 2, 2, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        got = model.decode(feats.permute(0, 2, 3, 4, 1))
        want = restate_decoder(model.state_dict(), feats)
    assert got.shape == (2, 2, 32, 48, 5)
    assert torch.allclose(got.permute(0, 4, 1, 2, 3), want, rtol=1e-9, atol=1e-9)
