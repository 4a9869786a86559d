"""``t2i_shared_kernel`` (csrc/decoder.hip): the layer-0 token->image attention on the shared K / V^T works on 4 prompts per
workgroup by default, on 16 or 8 with ``msam_tune_set("t2i_shared_group", 16 / 8)``.  A score column is one (prompt, token), the MFMA
treats columns independently, and the key quarter per wave, the 32-key step and the four-way merge are the same in every build: the
decoder's outputs must be the same BITS whatever the group size.

Cases: P = 1 (one column group of eight in use), 3 (a half-filled second tile), 16 (one full workgroup of 16), 17 (a one-prompt
tail workgroup in every build: 17 = 16 + 1 = 2 x 8 + 1 = 4 x 4 + 1), 130 (the chained route, "dec_chain_min_p" = 128, with a
two-prompt tail); Nt = 6, 7, 8 tokens per prompt (the kernel takes up to 8).  Nt = 6 is reached through the module call with one
sparse token and the broadcast ``no_mask_embed``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUP_DEFAULT = 4


@pytest.fixture(scope="module")
def ctx(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    predictor.set_image(util._to_image(synthetic_tile(5)))
    return dict(sam=predictor.model, feats=predictor.get_image_embedding())


def _decode(ctx, P, Nt, group):
    from micro_sam_amd import _lib
    lib = _lib.load()
    sam = ctx["sam"]
    g = torch.Generator().manual_seed(1000 * Nt + P)
    n = 2 if Nt == 8 else 1
    pts = (torch.rand(P, n, 2, generator=g) * 1000 + 12).cuda()
    lbl = (torch.rand(P, n, generator=g) > 0.35).to(torch.int).cuda()
    try:
        _lib.check(lib.msam_tune_set(b"t2i_shared_group", group), "msam_tune_set")
        if Nt == 6:                                      # the point's own token without its padding token: 5 + 1 tokens per prompt
            sparse, _ = sam.prompt_encoder((pts, lbl), None, None)
            dense = sam.prompt_encoder.no_mask_embed.weight.detach().reshape(1, -1, 1, 1).expand(P, -1, 64, 64)
            return sam.mask_decoder(image_embeddings=ctx["feats"], image_pe=sam.prompt_encoder.get_dense_pe(),
                                    sparse_prompt_embeddings=sparse[:, :1].contiguous(), dense_prompt_embeddings=dense,
                                    multimask_output=True)
        return sam.decode(ctx["feats"], pts, lbl)
    finally:
        lib.msam_tune_set(b"t2i_shared_group", GROUP_DEFAULT)


@pytest.mark.parametrize("Nt", [6, 7, 8])
@pytest.mark.parametrize("P", [1, 3, 16, 17, 130])
def test_group_of_16_gives_the_bits_of_the_group_of_4(ctx, P, Nt):
    low_4, iou_4 = _decode(ctx, P, Nt, 4)
    low_16, iou_16 = _decode(ctx, P, Nt, 16)
    assert low_4.shape == (P, 3, 256, 256) and bool(torch.isfinite(low_4).all())
    assert torch.equal(low_16, low_4) and torch.equal(iou_16, iou_4)


@pytest.mark.parametrize("P,Nt", [(17, 7), (130, 8)])
def test_group_of_8_gives_the_bits_of_the_group_of_4(ctx, P, Nt):
    """The third build, at the case with a tail in every build and on the chained route."""
    low_4, iou_4 = _decode(ctx, P, Nt, 4)
    low_8, iou_8 = _decode(ctx, P, Nt, 8)
    assert torch.equal(low_8, low_4) and torch.equal(iou_8, iou_4)
