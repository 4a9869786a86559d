"""The prompt prefix (``msam_decoder_prompt_prefix`` / ``msam_decoder_forward_masks_prefixed``, csrc/decoder.hip): what a decode
computes from the prompts and the weights alone - prompt tokens, layer 0's self attention, its out projection, norm1 and the q of the
token->image attention - is computed once, through the kernels a decode uses, and read in place afterwards.  A prefixed decode must
give the BITS of the plain one (low-res logits, IoU predictions, range map), must not write the block, and one block must serve any
embedding.

Cases: P = 1, 17 (stage-by-stage route, a tail in every grouping), 130 (chained route, "dec_chain_min_p" = 128); one point per
prompt (Nt = 7 tokens) and point + box (Nt = 8); once a mask input at P = 8 (own-source route: every prompt has its own stream)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    predictor.set_image(util._to_image(synthetic_tile(5)))
    feats = predictor.get_image_embedding().clone()
    predictor.set_image(util._to_image(synthetic_tile(6)))
    feats2 = predictor.get_image_embedding().clone()
    assert not torch.equal(feats, feats2)
    return dict(sam=predictor.model, feats=feats, feats2=feats2)


def _prompts(P, with_box):
    g = torch.Generator().manual_seed(31 * P + int(with_box))
    pts = (torch.rand(P, 1, 2, generator=g) * 1000 + 12).cuda()
    lbl = (torch.rand(P, 1, generator=g) > 0.35).to(torch.int).cuda()
    bx = None
    if with_box:
        x0 = torch.rand(P, 2, generator=g) * 600 + 20
        bx = torch.cat([x0, x0 + torch.rand(P, 2, generator=g) * 350 + 30], dim=1).cuda()
    return pts, lbl, bx


@pytest.mark.parametrize("with_box", [False, True], ids=["point", "point_box"])
@pytest.mark.parametrize("P", [1, 17, 130])
def test_prefixed_decode_gives_the_bits_of_the_plain_one(ctx, P, with_box):
    sam = ctx["sam"]
    pts, lbl, bx = _prompts(P, with_box)
    low0, iou0, rng0 = sam.decode(ctx["feats"], pts, lbl, boxes=bx, range_map=True)
    prefix = sam.make_prompt_prefix(pts, lbl, bx)
    Nt = 8 if with_box else 7
    from micro_sam_amd import _lib
    assert prefix.block.numel() == _lib.load().msam_decoder_prompt_prefix_bytes(P, Nt) >= P * Nt * (2 * 256 * 4 + 128 * 2)
    before = prefix.block.clone()
    low1, iou1, rng1 = sam.decode(ctx["feats"], None, None, range_map=True, prompt_prefix=prefix)
    assert low1.shape == (P, 3, 256, 256) and bool(torch.isfinite(low1).all())
    assert torch.equal(low1, low0) and torch.equal(iou1, iou0) and torch.equal(rng1, rng0)
    assert torch.equal(prefix.block, before), "a decode wrote the prefix block"
    # the same block against another embedding
    low2, iou2, rng2 = sam.decode(ctx["feats2"], pts, lbl, boxes=bx, range_map=True)
    low3, iou3, rng3 = sam.decode(ctx["feats2"], None, None, range_map=True, prompt_prefix=prefix)
    assert not torch.equal(low2, low0)
    assert torch.equal(low3, low2) and torch.equal(iou3, iou2) and torch.equal(rng3, rng2)
    assert torch.equal(prefix.block, before), "a decode wrote the prefix block"


def test_prefixed_decode_with_a_mask_input(ctx):
    sam = ctx["sam"]
    P = 8
    pts, lbl, _ = _prompts(P, False)
    masks = sam.decode(ctx["feats"], pts, lbl, multimask_output=False)[0].clone()          # [P, 1, 256, 256] low-res logits
    low0, iou0 = sam.decode(ctx["feats"], pts, lbl, mask_input=masks)
    prefix = sam.make_prompt_prefix(pts, lbl)
    before = prefix.block.clone()
    low1, iou1 = sam.decode(ctx["feats"], None, None, mask_input=masks, prompt_prefix=prefix)
    assert bool(torch.isfinite(low1).all())
    assert torch.equal(low1, low0) and torch.equal(iou1, iou0)
    assert torch.equal(prefix.block, before), "a decode wrote the prefix block"


def test_prefix_of_other_constants_is_refused(ctx):
    sam = ctx["sam"]
    pts, lbl, _ = _prompts(3, False)
    prefix = sam.make_prompt_prefix(pts, lbl)
    with pytest.raises(ValueError):
        sam.decode(ctx["feats"], pts, lbl, prompt_prefix=prefix)            # the prompts are the prefix's own
    sam.set_split_token_mlp(False)                                           # rebuilds the prepared constants
    try:
        with pytest.raises(ValueError):
            sam.decode(ctx["feats"], None, None, prompt_prefix=prefix)
    finally:
        sam.set_split_token_mlp(True)


@pytest.mark.parametrize("P,n_points", [(130, 1), (3, 10)], ids=["chained_Nt7", "unfolded_Nt16"])
def test_workspace_bytes_suffice_for_the_merged_groups(ctx, P, n_points):
    """The q / k / v of layer 1's self attention leave with layer 0's last grouped launch and wait in the workspace: a decode in a
    workspace of exactly msam_decoder_workspace_bytes(P) bytes (sized for 16 tokens per prompt = 10 points) writes nothing behind it."""
    from micro_sam_amd import _lib
    sam = ctx["sam"]
    need = _lib.load().msam_decoder_workspace_bytes(P)
    guard = 1 << 16
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(P)
    pts = (torch.rand(P, n_points, 2, generator=g) * 1000 + 12).cuda()
    lbl = torch.ones(P, n_points, dtype=torch.int).cuda()
    kept = sam._dec_ws
    sam._dec_ws = buf[:need]
    try:
        low, _ = sam.decode(ctx["feats"], pts, lbl)
        prefix = sam.make_prompt_prefix(pts, lbl)
        low1, _ = sam.decode(ctx["feats"], None, None, prompt_prefix=prefix)
        assert sam._dec_ws.data_ptr() == buf.data_ptr()
    finally:
        sam._dec_ws = kept
    assert bool(torch.isfinite(low).all()) and torch.equal(low1, low)
    assert bool((buf[need:] == 0xA5).all()), "a decode wrote behind msam_decoder_workspace_bytes(P)"
