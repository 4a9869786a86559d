"""The PEFT surgeries of micro_sam_amd.models.peft_sam beyond LoRA, on the CPU (no library needed): the state-dict names of the operated
encoder against hand-written lists of the reference's names, the merged parameters the inference path reads against the fp64 evaluation
of "layer, then branch", the ``requires_grad`` patterns of the selective surgeries, the argument errors of ``PEFT_Sam``, and the taped
composition of training/encoders.py (primitives replaced by torch stand-ins, as tests/test_training_encoders_host.py does) against a
plain-torch fp64 restatement of the three equations."""
import pytest
import torch
import torch.nn.functional as F

from micro_sam_amd import modeling
from micro_sam_amd.models import peft_sam as P
from micro_sam_amd.training import encoders as E
from micro_sam_amd.training import functional as HF

D = 128
BLOCK_KEYS = ["norm1.weight", "norm1.bias", "attn.rel_pos_h", "attn.rel_pos_w", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
              "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.lin1.weight", "mlp.lin1.bias", "mlp.lin2.weight", "mlp.lin2.bias"]
# the reference's names of an operated block, written out by hand
FACT_KEYS = ["norm1.weight", "norm1.bias", "attn.rel_pos_h", "attn.rel_pos_w", "attn.qkv.qkv_proj.weight", "attn.qkv.qkv_proj.bias",
             "attn.qkv.q_FacTs.weight", "attn.qkv.v_FacTs.weight", "attn.qkv.FacTu.weight", "attn.qkv.FacTv.weight", "attn.proj.weight",
             "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.lin1.weight", "mlp.lin1.bias", "mlp.lin2.weight", "mlp.lin2.bias"]
SSF_KEYS = ["attn.rel_pos_h", "attn.rel_pos_w",
            "norm1.layer.weight", "norm1.layer.bias", "norm1.scale", "norm1.shift",
            "attn.qkv.layer.weight", "attn.qkv.layer.bias", "attn.qkv.scale", "attn.qkv.shift",
            "attn.proj.layer.weight", "attn.proj.layer.bias", "attn.proj.scale", "attn.proj.shift",
            "norm2.layer.weight", "norm2.layer.bias", "norm2.scale", "norm2.shift",
            "mlp.lin1.layer.weight", "mlp.lin1.layer.bias", "mlp.lin1.scale", "mlp.lin1.shift",
            "mlp.lin2.layer.weight", "mlp.lin2.layer.bias", "mlp.lin2.scale", "mlp.lin2.shift"]
ADAPT_KEYS = ["norm1.weight", "norm1.bias", "attn.rel_pos_h", "attn.rel_pos_w", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
              "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.alpha", "mlp.mlp_proj.lin1.weight", "mlp.mlp_proj.lin1.bias",
              "mlp.mlp_proj.lin2.weight", "mlp.mlp_proj.lin2.bias", "mlp.down_proj.weight", "mlp.down_proj.bias", "mlp.up_proj.weight",
              "mlp.up_proj.bias"]
OUTSIDE = ["pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "neck.0.weight", "neck.1.weight", "neck.1.bias", "neck.2.weight",
           "neck.3.weight", "neck.3.bias"]


def small_sam(seed: int = 0) -> modeling.Sam:
    """Two blocks (one windowed, one global) of width 128 / 2 heads, random parameters."""
    torch.manual_seed(seed)
    enc = modeling.ImageEncoderViT(embed_dim=D, depth=2, num_heads=2, global_attn_indexes=(1,))
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "norm" in n and n.endswith("weight") or n in ("neck.1.weight", "neck.3.weight"):
                p.copy_(1 + 0.2 * torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) * (0.5 if "rel_pos" in n or "pos_embed" in n or n.endswith("bias") else p[0].numel() ** -0.5))
    return modeling.Sam(enc, modeling.PromptEncoder(), modeling.MaskDecoder())


def randomise(params, std: float = 0.3) -> None:
    with torch.no_grad():
        for p in params:
            p.copy_(torch.randn_like(p) * std + (1.0 if p.dim() == 1 and p.numel() > 1 else 0.0))


def encoder_keys(sam, block: int):
    pre = f"blocks.{block}."
    return sorted(k[len(pre):] for k in sam.image_encoder.state_dict() if k.startswith(pre))


@pytest.mark.parametrize("module,kwargs,keys", [
    (P.FacTSurgery, dict(rank=4), FACT_KEYS), (P.SSFSurgery, dict(), SSF_KEYS), (P.AdaptFormer, dict(), ADAPT_KEYS),
    (P.AttentionSurgery, dict(), BLOCK_KEYS), (P.BiasSurgery, dict(), BLOCK_KEYS), (P.LayerNormSurgery, dict(), BLOCK_KEYS),
    (P.ClassicalSurgery, dict(), BLOCK_KEYS)], ids=lambda v: getattr(v, "__name__", ""))
def test_state_dict_names_are_the_references(module, kwargs, keys):
    sam = small_sam()
    before = set(sam.image_encoder.state_dict())
    wrapped = P.PEFT_Sam(sam, peft_module=module, attention_layers_to_update=[1], **kwargs)
    assert wrapped.sam is sam
    assert encoder_keys(sam, 1) == sorted(keys)
    assert encoder_keys(sam, 0) == sorted(BLOCK_KEYS)                       # the other block is as it was
    outside = sorted(k for k in sam.image_encoder.state_dict() if not k.startswith("blocks."))
    assert outside == sorted(OUTSIDE)                                       # SSF adds nothing at the patch embedding
    if keys is BLOCK_KEYS:
        assert set(sam.image_encoder.state_dict()) == before
    # an upstream checkpoint of these names loads: a state dict with every tensor replaced goes in strictly
    sd = {k: torch.full_like(v, 0.5) for k, v in sam.image_encoder.state_dict().items()}
    sam.image_encoder.load_state_dict(sd, strict=True)


def test_adaptformer_fixed_alpha_has_no_parameter():
    sam = small_sam()
    P.PEFT_Sam(sam, peft_module=P.AdaptFormer, alpha=0.25, projection_size=32, dropout=0.1)
    assert encoder_keys(sam, 0) == sorted(k for k in ADAPT_KEYS if k != "mlp.alpha")
    mlp = sam.image_encoder.blocks[0].mlp
    assert mlp.alpha == 0.25 and mlp.down_proj.weight.shape == (32, D) and mlp.up_proj.weight.shape == (D, 32)
    assert not mlp.up_proj.weight.any() and not mlp.up_proj.bias.any() and not mlp.down_proj.bias.any()     # the reference's initial state
    assert mlp.lin1 is mlp.mlp_proj.lin1 and mlp.lin2 is mlp.mlp_proj.lin2


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def test_fact_merged_weight_is_layer_then_branch():
    sam = small_sam(1)
    P.PEFT_Sam(sam, rank=4, peft_module=P.FacTSurgery)
    mod = sam.image_encoder.blocks[0].attn.qkv
    randomise([mod.q_FacTs.weight, mod.v_FacTs.weight, mod.FacTu.weight, mod.FacTv.weight])
    x = torch.randn(5, D, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    w, b = mod.qkv_proj.weight.double(), mod.qkv_proj.bias.double()
    low = x @ mod.FacTu.weight.double().T
    new_q = low @ mod.q_FacTs.weight.double().T @ mod.FacTv.weight.double().T
    new_v = low @ mod.v_FacTs.weight.double().T @ mod.FacTv.weight.double().T
    want = x @ w.T + b + torch.cat([new_q, torch.zeros_like(new_q), new_v], dim=-1)
    assert mod.weight.dtype == torch.float32 and mod.weight.shape == (3 * D, D) and (mod.in_features, mod.out_features) == (D, 3 * D)
    got = x @ mod.weight.double().T + mod.bias.double()
    assert rel(got, want) <= 1e-5
    assert rel(got, x @ w.T + b) > 1e-2                                     # and the branch is there
    assert torch.equal(mod.weight[D:2 * D], mod.qkv_proj.weight[D:2 * D])   # the k rows are untouched


def test_ssf_merged_parameters_are_layer_then_branch():
    sam = small_sam(3)
    P.PEFT_Sam(sam, peft_module=P.SSFSurgery)
    blk = sam.image_encoder.blocks[1]
    g = torch.Generator().manual_seed(4)
    for mod in (blk.attn.qkv, blk.attn.proj, blk.mlp.lin1, blk.mlp.lin2):
        assert isinstance(mod, P.ScaleShiftLayer) and mod.scale.shape == mod.shift.shape == (mod.layer.out_features,)
        x = torch.randn(5, mod.in_features, dtype=torch.float64, generator=g)
        want = (x @ mod.layer.weight.double().T + mod.layer.bias.double()) * mod.scale.double() + mod.shift.double()
        got = x @ mod.weight.double().T + mod.bias.double()
        assert mod.weight.dtype == mod.bias.dtype == torch.float32 and rel(got, want) <= 1e-5
        assert rel(got, x @ mod.layer.weight.double().T + mod.layer.bias.double()) > 1e-2
    for mod in (blk.norm1, blk.norm2):
        assert isinstance(mod, P.ScaleShiftLayer) and mod.eps == 1e-6 and tuple(mod.normalized_shape) == (D,)
        x = torch.randn(5, D, dtype=torch.float64, generator=g) * 2 + 1
        plain = F.layer_norm(x, (D,), mod.layer.weight.double(), mod.layer.bias.double(), mod.eps)
        want = plain * mod.scale.double() + mod.shift.double()
        got = F.layer_norm(x, (D,), mod.weight.double(), mod.bias.double(), mod.eps)
        assert rel(got, want) <= 1e-5 and rel(got, plain) > 1e-2


@pytest.mark.parametrize("module,chosen", [
    (P.AttentionSurgery, lambda n: n.startswith("attn")), (P.BiasSurgery, lambda n: n.endswith("bias")),
    (P.LayerNormSurgery, lambda n: n.startswith(("norm1", "norm2"))), (P.ClassicalSurgery, lambda n: True)],
    ids=lambda v: getattr(v, "__name__", ""))
def test_selective_surgeries_choose_what_trains(module, chosen):
    sam = small_sam()
    wrapped = P.PEFT_Sam(sam, peft_module=module, attention_layers_to_update=[1])
    assert len(wrapped.peft_blocks) == 1 and isinstance(wrapped.peft_blocks[0], P.SelectiveSurgery)
    for n, p in sam.image_encoder.named_parameters():
        inside = n.startswith("blocks.1.")
        assert p.requires_grad == (inside and chosen(n[len("blocks.1."):])), n
    assert any(p.requires_grad for p in sam.image_encoder.parameters())
    assert all(p.requires_grad for p in sam.mask_decoder.parameters())      # only the image encoder is frozen first


def test_argument_errors():
    with pytest.raises(ValueError, match="not a valid transformer block id"):
        P.PEFT_Sam(small_sam(), peft_module=P.AdaptFormer, attention_layers_to_update=[0, 2])
    with pytest.raises(ValueError, match="not a valid transformer block id"):
        P.PEFT_Sam(small_sam(), peft_module=P.AttentionSurgery, attention_layers_to_update=[-1])
    for rank in (None, 0, -2):
        with pytest.raises(RuntimeError, match="valid rank"):
            P.PEFT_Sam(small_sam(), rank=rank, peft_module=P.FacTSurgery)
    for bad in (torch.nn.Identity, torch.nn.Linear, "AdaptFormer", P.ScaleShiftLayer):
        with pytest.raises(NotImplementedError):
            P.PEFT_Sam(small_sam(), rank=4, peft_module=bad)
    with pytest.raises(NotImplementedError, match="QLoRA"):
        P.PEFT_Sam(small_sam(), rank=4, peft_module=P.FacTSurgery, quantize=True)
    # no rank is needed by the others
    for module in (P.SSFSurgery, P.AdaptFormer, P.BiasSurgery):
        P.PEFT_Sam(small_sam(), peft_module=module)


# ------------------------------------------------------------------------------------------------------------- the taped path

@pytest.fixture()
def torch_primitives(monkeypatch):
    monkeypatch.setattr(HF, "linear", lambda x, w, b=None: F.linear(x, w, b))
    monkeypatch.setattr(HF, "layer_norm", lambda x, w, b, eps: F.layer_norm(x, (x.shape[-1],), w, b, eps))


def d(t):
    return t.detach().double()


def test_taped_fact_projection(torch_primitives):
    sam = small_sam(5)
    P.PEFT_Sam(sam, rank=4, peft_module=P.FacTSurgery, dropout=0.0)
    attn = sam.image_encoder.blocks[0].attn
    mod = attn.qkv
    randomise([mod.q_FacTs.weight, mod.v_FacTs.weight, mod.FacTu.weight, mod.FacTv.weight])
    x = torch.randn(2, 7, D, generator=torch.Generator().manual_seed(6))
    low = d(x) @ d(mod.FacTu.weight).T
    want = d(x) @ d(mod.qkv_proj.weight).T + d(mod.qkv_proj.bias)
    want[..., :D] += low @ d(mod.q_FacTs.weight).T @ d(mod.FacTv.weight).T
    want[..., 2 * D:] += low @ d(mod.v_FacTs.weight).T @ d(mod.FacTv.weight).T
    mod.train()
    got = E._qkv_projection(attn, x)                                        # p = 0: the dropout is the identity in training mode too
    assert rel(got, want) <= 1e-5
    assert rel(got, d(x) @ d(mod.weight).T + d(mod.bias)) <= 1e-5           # ... which is what inference merges
    got.sum().backward()
    for n, p in mod.named_parameters():
        assert (p.grad is not None and bool(p.grad.abs().sum() > 0)) == (not n.startswith("qkv_proj")), n
    # p > 0: ignored by eval(), active in training mode
    mod.dropout, mod.dp_q.p, mod.dp_v.p = 0.5, 0.5, 0.5
    mod.eval()
    assert torch.equal(E._qkv_projection(attn, x), got)
    mod.train()
    torch.manual_seed(0)
    assert not torch.equal(E._qkv_projection(attn, x), got)
    mod.dropout = None                                                      # no dropout modules asked for: the same as p = 0
    assert torch.equal(E._qkv_projection(attn, x), got)


def test_taped_ssf_block(torch_primitives):
    sam = small_sam(7)
    P.PEFT_Sam(sam, peft_module=P.SSFSurgery)
    blk = sam.image_encoder.blocks[0]
    x = torch.randn(2, 7, D, generator=torch.Generator().manual_seed(8)) * 2 + 0.5

    def ssf(mod, v):
        return v * d(mod.scale) + d(mod.shift)
    for mod in (blk.norm1, blk.norm2):
        want = ssf(mod, F.layer_norm(d(x), (D,), d(mod.layer.weight), d(mod.layer.bias), mod.layer.eps))
        assert rel(E._norm(mod, x), want) <= 1e-5
    want = ssf(blk.attn.qkv, d(x) @ d(blk.attn.qkv.layer.weight).T + d(blk.attn.qkv.layer.bias))
    assert rel(E._qkv_projection(blk.attn, x), want) <= 1e-5
    want = ssf(blk.attn.proj, d(x) @ d(blk.attn.proj.layer.weight).T + d(blk.attn.proj.layer.bias))
    assert rel(E._linear(blk.attn.proj, x), want) <= 1e-5
    h = F.gelu(ssf(blk.mlp.lin1, d(x) @ d(blk.mlp.lin1.layer.weight).T + d(blk.mlp.lin1.layer.bias)))
    want = ssf(blk.mlp.lin2, h @ d(blk.mlp.lin2.layer.weight).T + d(blk.mlp.lin2.layer.bias))
    got = E._mlp(blk.mlp, x)
    assert rel(got, want) <= 1e-5
    (got.sum() + E._norm(blk.norm1, x).sum()).backward()
    for n, p in blk.named_parameters():
        trained = n.endswith(("scale", "shift")) and n.startswith(("mlp", "norm1"))
        assert (p.grad is not None) == trained, n                           # the wrapped layers are frozen


@pytest.mark.parametrize("alpha", ["learnable_scalar", 0.3])
def test_taped_adaptformer_mlp(torch_primitives, alpha):
    sam = small_sam(9)
    P.PEFT_Sam(sam, peft_module=P.AdaptFormer, alpha=alpha, dropout=0.0, projection_size=32)
    mlp = sam.image_encoder.blocks[1].mlp
    randomise([mlp.down_proj.weight, mlp.down_proj.bias, mlp.up_proj.weight, mlp.up_proj.bias], std=0.2)
    if alpha == "learnable_scalar":
        with torch.no_grad():
            mlp.alpha.fill_(0.7)
    a = 0.7 if alpha == "learnable_scalar" else alpha
    y = torch.randn(2, 7, D, generator=torch.Generator().manual_seed(10))
    base = F.gelu(d(y) @ d(mlp.mlp_proj.lin1.weight).T + d(mlp.mlp_proj.lin1.bias)) @ d(mlp.mlp_proj.lin2.weight).T + d(mlp.mlp_proj.lin2.bias)
    hidden = torch.relu(d(y) @ d(mlp.down_proj.weight).T + d(mlp.down_proj.bias))
    assert 0.2 <= float((hidden == 0).double().mean()) <= 0.8
    want = d(y) + base + a * (hidden @ d(mlp.up_proj.weight).T + d(mlp.up_proj.bias))      # the module's input is its own residual
    mlp.train()
    got = E._mlp(mlp, y)
    assert rel(got, want) <= 1e-5
    assert rel(got, base) > 1e-2
    got.sum().backward()
    for n, p in mlp.named_parameters():
        assert (p.grad is not None) == (not n.startswith("mlp_proj")), n
    mlp.dropout, mlp.dropout_layer.p = 0.5, 0.5
    mlp.eval()
    assert torch.equal(E._mlp(mlp, y), got)
    mlp.train()
    torch.manual_seed(0)
    assert not torch.equal(E._mlp(mlp, y), got)
    mlp.dropout = None
    assert torch.equal(E._mlp(mlp, y), got)


@pytest.mark.parametrize("module,kwargs", [(P.FacTSurgery, dict(rank=4, dropout=None)), (P.SSFSurgery, dict())], ids=["fact", "ssf"])
def test_taped_encoder_equals_the_plain_encoder_on_merged_parameters(torch_primitives, monkeypatch, module, kwargs):
    """Through the whole taped encoder: the separate branches give what the plain encoder gives on the merged parameters the inference
    path reads, and only the PEFT parameters receive gradients."""
    def dense_attention(q, k, v, bias_h, bias_w, scale):
        BH, N, _ = q.shape
        Gh, Gw = bias_h.shape[2], bias_w.shape[2]
        s = ((q * scale) @ k.transpose(1, 2)).view(BH, N, Gh, Gw) + bias_h[:, :, :, None] + bias_w[:, :, None, :]
        return s.view(BH, N, N).softmax(dim=-1) @ v
    monkeypatch.setattr(HF, "relpos_attention", dense_attention)
    monkeypatch.setattr(HF, "RELPOS_ATTENTION_IMPL", "kernel")
    sam, plain = small_sam(11), small_sam(11)
    P.PEFT_Sam(sam, peft_module=module, **kwargs)
    enc = sam.image_encoder
    new = [p for n, p in enc.named_parameters() if p.requires_grad]
    assert new and len(new) == (8 if module is P.FacTSurgery else 24)
    randomise(new, std=0.2)
    with torch.no_grad():
        for a, b in zip(plain.image_encoder.blocks, enc.blocks):
            for dst, src in ((a.attn.qkv, b.attn.qkv), (a.attn.proj, b.attn.proj), (a.mlp.lin1, b.mlp.lin1), (a.mlp.lin2, b.mlp.lin2),
                             (a.norm1, b.norm1), (a.norm2, b.norm2)):
                dst.weight.copy_(src.weight)
                dst.bias.copy_(src.bias)
    x = torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(12))
    out = E.image_encoder_forward(enc, x)
    with torch.no_grad():
        ref = E.image_encoder_forward(plain.image_encoder, x)
    assert (out - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()
    out.square().sum().backward()
    for n, p in enc.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
        else:
            assert p.grad is None, n
