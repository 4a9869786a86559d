"""FacT, SSF and AdaptFormer models on the device (vit_b, synthetic weights, blocks 0 and 2 operated, non-trivial random PEFT parameters):

* the restated block loop of tests/peft_ref.py IS the oracle's when no PEFT key is present (CPU, ``torch.equal`` taps), and its separate
  branches give what the oracle gives on the merged parameters;
* FacT / SSF: the embedding equals that of a plain model loaded with the test's own merged weights, bit for bit, and differs visibly from
  the un-adapted model;
* AdaptFormer: the residual stream after block 2 of the bf16 encoder (the fused adapter kernel inside msam_encoder_forward) against the
  restatement in the oracle's "bf16" policy at the bound tests/test_gpu_model.py::test_encoder_vs_oracle uses for that tap; the strict and
  split16 modes against the fp32 restatement at the bound of tests/test_gpu_strict.py; the fp8 mode refuses;
* one taped step of ``get_trainable_sam_model`` per method: exactly the method's parameters receive gradients."""
import numpy as np
import pytest
import torch

import peft_ref as PR

LAYERS = [0, 2]
D = 768


def fact_state_dict(sd, rank=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for i in LAYERS:
        a = f"image_encoder.blocks.{i}.attn.qkv."
        out[a + "qkv_proj.weight"], out[a + "qkv_proj.bias"] = out.pop(a + "weight"), out.pop(a + "bias")
        out[a + "q_FacTs.weight"] = torch.randn(rank, rank, generator=g) * 0.3
        out[a + "v_FacTs.weight"] = torch.randn(rank, rank, generator=g) * 0.3
        out[a + "FacTu.weight"] = torch.randn(rank, D, generator=g) * 0.2
        out[a + "FacTv.weight"] = torch.randn(D, rank, generator=g) * 0.2
    return out


def ssf_state_dict(sd, seed=2):
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for i in LAYERS:
        for name in ("attn.qkv", "attn.proj", "mlp.lin1", "mlp.lin2", "norm1", "norm2"):
            m = f"image_encoder.blocks.{i}.{name}."
            out[m + "layer.weight"], out[m + "layer.bias"] = out.pop(m + "weight"), out.pop(m + "bias")
            n = out[m + "layer.weight"].shape[0]
            out[m + "scale"] = 1.0 + 0.2 * torch.randn(n, generator=g)
            out[m + "shift"] = 0.2 * torch.randn(n, generator=g)
    return out


def adapt_state_dict(sd, P=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for i in LAYERS:
        m = f"image_encoder.blocks.{i}.mlp."
        for j in ("1", "2"):
            out[m + f"mlp_proj.lin{j}.weight"], out[m + f"mlp_proj.lin{j}.bias"] = out.pop(m + f"lin{j}.weight"), out.pop(m + f"lin{j}.bias")
        out[m + "down_proj.weight"] = torch.randn(P, D, generator=g) * D ** -0.5
        out[m + "down_proj.bias"] = torch.randn(P, generator=g) * 0.3
        out[m + "up_proj.weight"] = torch.randn(D, P, generator=g) * 0.5
        out[m + "up_proj.bias"] = torch.randn(D, generator=g) * 0.5
        out[m + "alpha"] = torch.tensor([0.8])
    return out


@pytest.fixture(scope="module")
def inputs():
    from micro_sam_amd.synthetic import synthetic_tile
    from oracle import amg_ref as A
    from oracle import sam_ref as S
    img = A.to_image(synthetic_tile(0))
    return img, S.preprocess(torch.as_tensor(img).permute(2, 0, 1)[None])


def test_restated_loop_is_the_oracles(vit_b_sd, inputs):
    from oracle import sam_ref as S
    with torch.no_grad():
        _, want = S.image_encoder(vit_b_sd, inputs[1], precision="bf16", return_blocks=True, stop_after_block=2)
        out, got = PR.image_encoder_peft(vit_b_sd, inputs[1], None, stop_after_block=2, precision="bf16")
    assert out is None and len(got) == len(want) == 3
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("method,build", [("fact", fact_state_dict), ("ssf", ssf_state_dict)])
def test_separate_branches_equal_the_merged_parameters(vit_b_sd, inputs, method, build):
    """fp32: "layer, then branch" through blocks 0 .. 2 against the oracle on the merged state dict (the merge identities)."""
    from oracle import sam_ref as S
    sd = build(vit_b_sd)
    with torch.no_grad():
        _, got = PR.image_encoder_peft(sd, inputs[1], method, stop_after_block=2, precision="fp32")
        _, want = S.image_encoder(PR.merged_state_dict(sd, method), inputs[1], precision="fp32", return_blocks=True, stop_after_block=2)
        _, plain = S.image_encoder(vit_b_sd, inputs[1], precision="fp32", return_blocks=True, stop_after_block=2)
    scale = want[2].abs().max().item()
    assert (got[2] - want[2]).abs().max().item() <= 1e-4 * scale
    assert (plain[2] - want[2]).abs().max().item() > 1e-2 * scale


def _model(sd, **peft_kwargs):
    from micro_sam_amd import util
    return util.get_sam_model("vit_b", device="cuda", state_dict=sd, peft_kwargs=peft_kwargs or None)


@pytest.fixture(scope="module")
def plain(vit_b_sd, inputs):
    p = _model(dict(vit_b_sd))
    p.set_image(inputs[0])
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["fact", "ssf"])
def test_fact_and_ssf_run_their_merged_weights(vit_b_sd, inputs, plain, method):
    from micro_sam_amd.models import peft_sam
    if method == "fact":
        sd = fact_state_dict(vit_b_sd)
        p = _model(sd, rank=4, peft_module=peft_sam.FacTSurgery, attention_layers_to_update=LAYERS)
    else:
        sd = ssf_state_dict(vit_b_sd)
        p = _model(sd, peft_module=peft_sam.SSFSurgery, attention_layers_to_update=LAYERS)
    merged = _model(PR.merged_state_dict(sd, method, device="cuda"))
    for m in (p, merged):
        m.set_image(inputs[0])
    assert torch.equal(p.features, merged.features)
    assert (p.features - plain.features).abs().max().item() > 1e-2         # the update is visible
    assert any(("FacTu" if method == "fact" else ".scale") in k for k in p.model.state_dict())


@pytest.fixture(scope="module")
def adapt(vit_b_sd, inputs):
    from micro_sam_amd.models import peft_sam
    sd = adapt_state_dict(vit_b_sd)
    p = _model(sd, peft_module=peft_sam.AdaptFormer, attention_layers_to_update=LAYERS, projection_size=64)
    return sd, p


@pytest.mark.gpu
def test_adaptformer_block_tap_vs_the_restatement(vit_b_sd, inputs, adapt, plain):
    sd, p = adapt
    with torch.no_grad():
        _, taps = PR.image_encoder_peft(sd, inputs[1], "adaptformer", stop_after_block=2, precision="bf16")
    r = taps[2].reshape(-1, D)
    bound = 0.01 * r.abs().max().item() + 0.02                                # test_encoder_vs_oracle's bound for this tap
    enc = p.model.image_encoder
    _, tap = enc(inputs[1].cuda(), tap_block=2)
    err = (tap.cpu() - r).abs().max().item()
    _, tap0 = plain.model.image_encoder(inputs[1].cuda(), tap_block=2)
    moved = (tap - tap0).abs().max().item()
    print(f"adaptformer tap 2: max |error| {err:.4f}, bound {bound:.4f}, moved by the adapters {moved:.3f}")
    assert err <= bound
    assert moved > 10 * bound                                                 # the branch is visibly there
    # the fp16 mode runs the kernel's other instantiation: the same restatement with fp16 rounding points
    from oracle import sam_ref as S
    enc.set_precision("fp16")
    try:
        S.ENCODER_DTYPE = torch.float16
        with torch.no_grad():
            _, taps16 = PR.image_encoder_peft(sd, inputs[1], "adaptformer", stop_after_block=2, precision="bf16")
        _, tap16 = enc(inputs[1].cuda(), tap_block=2)
    finally:
        S.ENCODER_DTYPE = torch.bfloat16
        enc.set_precision("bf16")
    assert (tap16.cpu() - taps16[2].reshape(-1, D)).abs().max().item() <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "split16"])
def test_adaptformer_strict_modes_vs_the_fp32_restatement(inputs, adapt, mode):
    sd, p = adapt
    with torch.no_grad():
        want, _ = _fp32_reference(sd, inputs[1])
    enc = p.model.image_encoder
    enc.set_precision(mode)
    try:
        got = enc(inputs[1].cuda()).cpu()
    finally:
        enc.set_precision("bf16")
    d = (got - want).abs()
    print(f"adaptformer {mode}: max |error| {d.max().item():.2e}, mean {d.mean().item():.2e}")
    assert d.max().item() <= 1e-3 and d.mean().item() <= 2e-5               # tests/test_gpu_strict.py's encoder bound


_REF32 = {}


def _fp32_reference(sd, x):
    """Computed once, shared by the two strict modes."""
    if "out" not in _REF32:
        _REF32["out"] = PR.image_encoder_peft(sd, x, "adaptformer", precision="fp32")
    return _REF32["out"]


@pytest.mark.gpu
def test_adaptformer_is_refused_in_fp8(inputs, adapt):
    enc = adapt[1].model.image_encoder
    enc.set_precision("fp8")
    try:
        with pytest.raises(NotImplementedError, match="fp8"):
            enc(inputs[1].cuda())
    finally:
        enc.set_precision("bf16")
    assert torch.isfinite(enc(inputs[1].cuda())).all()                       # and the model is usable afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["adaptformer", "fact", "ssf"])
def test_one_taped_step_trains_the_methods_parameters_only(vit_b_sd, method):
    from micro_sam_amd.models import peft_sam
    from micro_sam_amd.synthetic import synthetic_tile
    from micro_sam_amd.training import get_trainable_sam_model
    kwargs = {"adaptformer": {"peft_module": peft_sam.AdaptFormer}, "fact": {"peft_module": peft_sam.FacTSurgery, "rank": 4},
              "ssf": {"peft_module": peft_sam.SSFSurgery}}[method]
    m = get_trainable_sam_model("vit_b", device="cuda", state_dict=vit_b_sd, peft_kwargs=kwargs, freeze=["prompt_encoder", "mask_decoder"])
    m.train()
    if method == "fact":                                                      # FacT starts from random factors; its dropout is active
        assert m.sam.image_encoder.blocks[0].attn.qkv.dp_q.training
    img = torch.as_tensor(np.repeat(synthetic_tile(3)[None], 3, axis=0).astype(np.float32))
    emb, _ = m.image_embeddings_oft([{"image": img, "original_size": (1024, 1024)}])
    assert emb.requires_grad
    emb.square().mean().backward()
    seen = 0
    for n, p in m.sam.named_parameters():
        if method == "adaptformer":
            if ".mlp.up_proj." in n:
                assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n
            elif ".mlp.down_proj." in n:
                assert p.grad is not None and float(p.grad.abs().sum()) == 0, n          # up_proj starts at zero
            elif n.endswith(".mlp.alpha"):
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
            else:
                assert p.grad is None, n
                continue
        elif method == "fact":
            if any(t in n for t in (".FacTv.", ".FacTu.", ".q_FacTs.", ".v_FacTs.")):
                assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n
            else:
                assert p.grad is None, n
                continue
        else:
            if n.endswith((".scale", ".shift")):
                assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n
            else:
                assert p.grad is None, n
                continue
        seen += 1
    assert seen == {"adaptformer": 12 * 5, "fact": 12 * 4, "ssf": 12 * 12}[method]
