"""``models.sam_3d_wrapper`` without a device: the ``functional`` primitives are replaced by torch stand-ins (as
tests/test_training_encoders_host.py does) and the COMPOSITION is checked - the reference's ``state_dict`` keys and shapes, the output
shapes, which parameters train under ``freeze_encoder`` and LoRA, and the refusals - plus the trainer's 5-d loss against the 4-d loss of
the folded tensors, through the host build of csrc/semloss.hip (the fixtures of tests/test_semantic_trainer_host.py).  The depth
convolution kernel itself runs in tests/test_depth_conv_host.py, the model on the device in tests/test_gpu_sam3d.py."""
import pytest
import torch
import torch.nn.functional as F

from micro_sam_amd import modeling
from micro_sam_amd.training import functional as HF
from test_semantic_trainer_host import host_loss, lib, trainer  # noqa: F401  (fixtures)
from test_training_encoders_host import _dense_relpos_attention

WIDTH, HEADS, ADAPTER = 64, 2, 384


def conv3_stand_in(x, weight, bias, depth):
    """``functional.depth_conv3`` as the reference computes it: channels-first and torch's conv3d."""
    n, h, w, c = x.shape
    v = x.reshape(n // depth, depth, h, w, c).permute(0, 4, 1, 2, 3)
    return F.conv3d(v, weight, bias, padding="same").permute(0, 2, 3, 4, 1).reshape(n, h, w, weight.shape[0])


@pytest.fixture()
def torch_primitives(monkeypatch):
    monkeypatch.setattr(HF, "linear", lambda x, w, b=None: F.linear(x, w, b))
    monkeypatch.setattr(HF, "layer_norm", lambda x, w, b, eps: F.layer_norm(x, (x.shape[-1],), w, b, eps))
    monkeypatch.setattr(HF, "relpos_attention", _dense_relpos_attention)
    monkeypatch.setattr(HF, "RELPOS_ATTENTION_IMPL", "kernel")
    monkeypatch.setattr(HF, "attention", lambda q, k, v: F.scaled_dot_product_attention(q, k, v))
    monkeypatch.setattr(HF, "depth_conv3", conv3_stand_in)

    def never(self, *a, **k):
        raise AssertionError("the 3-d model must not call modeling.ImageEncoderViT.forward")
    monkeypatch.setattr(modeling.ImageEncoderViT, "forward", never)


def small_encoder():
    torch.manual_seed(0)
    return modeling.ImageEncoderViT(embed_dim=WIDTH, depth=2, num_heads=HEADS, global_attn_indexes=(1,))


def small_sam():
    sam = modeling.Sam(small_encoder(), modeling.PromptEncoder(), modeling.MaskDecoder())
    with torch.no_grad():
        for n, p in sam.named_parameters():
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() < 2 else p[0].numel() ** -0.5))
            if "norm" in n and n.endswith("weight"):
                p.add_(1.0)
    pe = torch.randn(1, 256, 64, 64, generator=torch.Generator().manual_seed(5))
    sam.prompt_encoder._dense_pe_fn = lambda: pe                         # (the device computes it in the decoder's constant pass)
    return sam


def test_state_dict_keys_and_shapes_are_the_references():
    from micro_sam_amd.models.sam_3d_wrapper import ImageEncoderViT3DWrapper, NDBlockWrapper, Sam3DWrapper
    plain = small_encoder().state_dict()
    enc = ImageEncoderViT3DWrapper(small_encoder(), num_heads=HEADS, embed_dim=WIDTH)
    assert all(isinstance(b, NDBlockWrapper) for b in enc.image_encoder.blocks) and enc.img_size == 1024
    want = {}
    for k, v in plain.items():
        parts = k.split(".")
        want["image_encoder." + (".".join(parts[:2] + ["block"] + parts[2:]) if parts[0] == "blocks" else k)] = tuple(v.shape)
    for i in range(2):
        for tag in ("", "_2"):
            pre = f"image_encoder.blocks.{i}."
            want[pre + f"adapter_linear_down{tag}.weight"] = (ADAPTER, WIDTH)
            want[pre + f"adapter_linear_up{tag}.weight"] = (WIDTH, ADAPTER)
            want[pre + f"adapter_conv{tag}.weight"] = (ADAPTER, ADAPTER, 3, 1, 1)
            want[pre + f"adapter_conv{tag}.bias"] = (ADAPTER,)
            want[pre + f"adapter_norm{tag}.weight"] = (WIDTH,)
            want[pre + f"adapter_norm{tag}.bias"] = (WIDTH,)
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == want
    # the order inside a block is the reference's order of construction
    names = [k for k in enc.state_dict() if k.startswith("image_encoder.blocks.0.adapter")]
    assert names == [f"image_encoder.blocks.0.adapter_{n}" for n in
                     ("linear_down.weight", "linear_up.weight", "conv.weight", "conv.bias", "norm.weight", "norm.bias", "linear_down_2.weight",
                      "linear_up_2.weight", "conv_2.weight", "conv_2.bias", "norm_2.weight", "norm_2.bias")]
    model = Sam3DWrapper(small_sam(), freeze_encoder=False)
    keys = set(model.state_dict())
    assert {"sam_model.image_encoder." + k for k in want} <= keys
    assert "sam_model.image_encoder.image_encoder.blocks.1.block.attn.rel_pos_h" in keys
    assert "sam_model.image_encoder.image_encoder.blocks.1.adapter_conv_2.weight" in keys
    assert all(k.startswith("sam_model.") for k in keys)


@pytest.mark.parametrize("depth", [1, 2])
def test_forward_shapes_and_gradients(torch_primitives, depth):
    from micro_sam_amd.models.sam_3d_wrapper import Sam3DWrapper
    model = Sam3DWrapper(small_sam(), freeze_encoder=False)
    g = torch.Generator().manual_seed(1)
    batch = [{"image": torch.rand(3, depth, 64, 64, generator=g) * 255, "original_size": (50, 40)}]
    out = model(batch, multimask_output=True)
    assert len(out) == 1 and set(out[0]) == {"masks", "iou_predictions", "low_res_logits"}
    assert out[0]["masks"].shape == (1, 3, depth, 50, 40)
    assert out[0]["low_res_logits"].shape == (1, 3, depth, 256, 256) and out[0]["iou_predictions"].shape == (depth, 3)
    out[0]["masks"].square().mean().backward()
    for n, p in model.named_parameters():
        if "adapter" in n and (depth > 1 or "conv" not in n):
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n
    with torch.no_grad():                                                  # evaluation: the same composition without a tape
        again = model(batch, multimask_output=True)
    assert not again[0]["masks"].requires_grad and torch.equal(again[0]["masks"], out[0]["masks"].detach())
    assert model(batch, multimask_output=False)[0]["masks"].shape == (1, 1, depth, 50, 40)
    with pytest.raises(ValueError, match="original_size"):
        model(batch + [{"image": batch[0]["image"], "original_size": (50, 41)}], multimask_output=True)


def test_a_slice_sees_its_neighbours_and_not_the_next_volume(torch_primitives):
    """Changing one slice of a volume changes the embeddings of the volume's other slices (the adapters mix along depth) and leaves the
    other volume of the batch alone."""
    from micro_sam_amd.models.sam_3d_wrapper import ImageEncoderViT3DWrapper
    enc = ImageEncoderViT3DWrapper(small_encoder(), num_heads=HEADS, embed_dim=WIDTH)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() < 2 else p[0].numel() ** -0.5))
        x = torch.randn(4, 3, 1024, 1024, generator=torch.Generator().manual_seed(2))
        a = enc(x, 2)
        x[1] += 1.0
        b = enc(x, 2)
    assert a.shape == (4, 256, 64, 64)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    assert torch.equal(a[2:], b[2:])
    with pytest.raises(ValueError, match="volumes"):
        enc(x[:3], 2)


def test_freeze_and_lora_requires_grad_pattern(monkeypatch):
    from micro_sam_amd import util
    from micro_sam_amd.models import peft_sam
    from micro_sam_amd.models.sam_3d_wrapper import Sam3DWrapper, get_sam_3d_model
    frozen = Sam3DWrapper(small_sam(), freeze_encoder=True)
    enc = {n for n, p in frozen.named_parameters() if n.startswith("sam_model.image_encoder.")}
    assert any("adapter_conv" in n for n in enc)
    assert all(p.requires_grad != n.startswith("sam_model.image_encoder.") for n, p in frozen.named_parameters())   # the adapters too
    assert all(p.requires_grad for p in Sam3DWrapper(small_sam(), freeze_encoder=False).parameters())

    seen = {}

    def fake_get_sam_model(model_type, device, checkpoint_path, return_sam, flexible_load_checkpoint, peft_kwargs, state_dict):
        seen.update(model_type=model_type, peft_kwargs=peft_kwargs, flexible=flexible_load_checkpoint, return_sam=return_sam)
        sam = small_sam()
        if peft_kwargs:
            sam = peft_sam.PEFT_Sam(sam, **peft_kwargs).sam
        return None, sam
    monkeypatch.setattr(util, "get_sam_model", fake_get_sam_model)
    lora = get_sam_3d_model("cpu", n_classes=3, image_size=1024, lora_rank=4, freeze_encoder=True)      # LoRA un-freezes
    assert seen["peft_kwargs"] == {"rank": 4, "peft_module": peft_sam.LoRASurgery} and seen["flexible"] and seen["return_sam"]
    assert lora.freeze_encoder is False
    for n, p in lora.named_parameters():
        in_enc = n.startswith("sam_model.image_encoder.")
        want = (not in_enc) or "adapter" in n or ".w_a_linear_" in n or ".w_b_linear_" in n
        assert p.requires_grad == want, n
    assert any(".block.attn.qkv.w_a_linear_q." in n for n, _ in lora.named_parameters())
    plain = get_sam_3d_model("cpu", n_classes=3, image_size=1024, freeze_encoder=True)
    assert seen["peft_kwargs"] == {} and plain.freeze_encoder is True
    assert not any(p.requires_grad for p in plain.sam_model.image_encoder.parameters())


def test_refusals():
    from micro_sam_amd.models.sam_3d_wrapper import Sam3DWrapper, get_sam_3d_model
    with pytest.raises(NotImplementedError, match="modeling.MaskDecoder"):
        get_sam_3d_model("cpu", n_classes=2, image_size=1024)
    with pytest.raises(NotImplementedError, match="build_sam"):
        get_sam_3d_model("cpu", n_classes=3, image_size=512)
    with pytest.raises(ValueError, match="vit_t"):
        get_sam_3d_model("cpu", n_classes=3, image_size=1024, model_type="vit_t")
    with pytest.raises(ValueError, match="vit_t"):
        Sam3DWrapper(small_sam(), freeze_encoder=False, model_type="vit_t")


def test_the_5d_loss_is_the_4d_loss_of_the_folded_tensors(host_loss):
    from micro_sam_amd.training import CustomDiceLoss
    g = torch.Generator().manual_seed(3)
    B, C, D, H, W = 2, 3, 3, 10, 12
    m5 = (2.0 * torch.randn(B, C, D, H, W, generator=g)).transpose(1, 2).contiguous().transpose(1, 2)     # as the model gives it
    y5 = torch.randint(0, C, (B, 1, D, H, W), generator=g)
    y5[0, 0, 1, 2, :] = -100
    assert not m5.is_contiguous()
    a5, a4 = m5.clone().requires_grad_(), m5.reshape(B, C, D * H, W).clone().requires_grad_()
    for w in (None, 0.3):
        a5.grad = a4.grad = None
        t5, t4 = trainer(w), trainer(w)
        l5 = t5._compute_loss(y5, a5)
        l4 = t4._compute_loss(y5.reshape(B, 1, D * H, W), a4)
        l5.backward()
        l4.backward()
        assert torch.equal(l5, l4) and torch.equal(a5.grad.reshape(a4.shape), a4.grad)                   # bit for bit
        assert all(torch.equal(p, q) for p, q in zip(t5.last_parts, t4.last_parts))
        assert torch.equal(t5._compute_loss(y5[:, 0], a5.detach()), l5.detach())                        # target [B, D, H, W]
    dice = CustomDiceLoss(C)
    assert torch.equal(dice(m5, y5), dice(m5.reshape(B, C, D * H, W), y5.reshape(B, D * H, W)))
    # the statistics of the volume are the per-slice statistics summed: counts exactly, the fp64 sums to their rounding
    _, whole = HF.semantic_loss(m5.reshape(B, C, D * H, W), y5.reshape(B, D * H, W))
    parts = [HF.semantic_loss(m5[:, :, z].contiguous(), y5[:, 0, z].contiguous())[1] for z in range(D)]
    assert torch.equal(whole.count, sum(p.count for p in parts))
    assert int(whole.n_valid) == sum(int(p.n_valid) for p in parts) and int(whole.n_ignored) == sum(int(p.n_ignored) for p in parts) == W
    for name in ("num", "psq", "ce_sum"):
        tot = sum(getattr(p, name) for p in parts)
        assert torch.allclose(getattr(whole, name), tot, rtol=1e-13, atol=0), name
    with pytest.raises(ValueError, match="target"):
        trainer()._compute_loss(y5[:, :, :2], m5)
    with pytest.raises(ValueError, match="channels"):
        trainer(classes=4)._compute_loss(y5, m5)
