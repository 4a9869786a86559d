"""The kernel sequences of ``decoder_run`` (csrc/decoder.hip) on the device, each as a whole decode against the CPU oracle.

``decoder_run`` picks its kernels from the launch's shape:

  * chained route (P >= "dec_chain_min_p" = 128 prompts, Nt <= 8 tokens per prompt, shared source): the layer-0 image stream is never
    written (csrc/decfold_tok.hip); this is what the automatic mask generator and the benchmark run;
  * stage-by-stage folded route (Nt <= 8, fewer prompts, or msam_tune_set("dec_chain", 0));
  * un-folded route (Nt = 9 .. 16);
  * own-source route (a mask / dense prompt: every prompt has its own source stream, never chained).

The other full-decoder comparisons with the oracle run 2 .. 8 prompts (stage-by-stage); the kernel tests of the chained forms
(tests/test_gpu_kernels.py::test_chained_layer0_forms) call the kernels one at a time on buffers of their own.  What is checked HERE is
the wiring of ``decoder_run`` around them - the blocked tables at the end of ``w.vT``, ``mfrag`` behind ``oper0``, ``oper1`` in
``w.attn_img``, the byte budget ``avail``, the blocked flag of the final attention and of the up-scaling kernel - at the prompt counts
where a grouping can go wrong (128 = the threshold; 129 / 131 = ragged tails past a 4-prompt group, a wave and a key-split step;
257 = one past two groups of 128 and one past the 256 workgroups of the persistent kernels), for every token count the route accepts
and both output forms.

Token counts: ``Sam.decode`` reaches Nt = 7 (one point + its padding point, or a box) and Nt = 8 (two points + padding, or a box and a
point).  Nt = 6 and Nt = 5 are reached with a shared source through the module call ``sam.mask_decoder`` (msam_decoder_forward_embeddings):
one sparse token / no sparse token and the broadcast ``no_mask_embed`` as the dense embedding, which ``Sam._decode_embeddings``
recognises as "no mask" - so those launches are chained as well and are covered below (kinds "one_token", "no_token").

References: the oracle (oracle.sam_ref, CPU) in its HIP-like rounding mode (precision="bf16": the decoder's 16-bit type at the decoder's
rounding points) and in fp32, with the tolerances of tests/test_gpu_model.py::test_decoder_vs_oracle; and the library's own
stage-by-stage decode of the same prompts.  Prompts are independent in the decoder (token self-attention is per prompt), so the oracle
runs on at most 8 rows per case - first, last, both sides of the group boundaries, one in the middle - and those rows of the device
result are compared; route-against-route comparisons use all rows.  Every oracle result is computed once and shared."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

# the library's defaults of every knob this module touches (include/msam_hip.h msam_tune_set)
TUNE_DEFAULTS = {"dec_chain": 1, "dec_chain_min_p": 128, "chain_variant": 9, "tok_fuse": 0, "mlp_split_fused": 1}

# tolerances of tests/test_gpu_model.py::test_decoder_vs_oracle (shares of the oracle's logit scale; IoU predictions absolute)
ORACLE_MAX, ORACLE_MEAN, ORACLE_IOU = 0.03, 0.006, 2e-3

# Route-to-route distance (chained vs stage-by-stage decode of the same prompts, ALL prompts; max / mean as shares of the logit scale,
# max IoU-prediction difference).  Measured on an MI355X, default library build (fp16 mask decoder), synthetic vit_b weights:
#     (P, Nt)      max        mean       IoU
#     (128, 7)     0.001726   0.0001679  9.423e-05
#     (128, 8)     0.001840   0.0001790  1.029e-04
#     (131, 7)     0.001843   0.0001826  1.041e-04
#     (131, 8)     0.001614   0.0001670  8.982e-05
# The bound is twice the largest measured value of each column: the two routes round at different points (the chained form recomputes
# the layer-0 stream tile by tile from the shared source instead of reading it back from memory), and which values land on a rounding boundary shifts
# with the operands.  It may not exceed the tolerance against the oracle (asserted below): two routes further apart than each is from
# the oracle would be a finding.  The same bound holds the threshold pair (127 | 128 prompts; measured max 0.001839, mean 0.0001778,
# IoU 1.040e-04) and the builds of the chained kernels against build 9 (measured max 0.001763, mean 0.0001672, IoU 1.019e-04).
ROUTE_MAX, ROUTE_MEAN, ROUTE_IOU = 2 * 0.001843, 2 * 0.0001826, 2 * 1.041e-04
assert ROUTE_MAX <= ORACLE_MAX and ROUTE_MEAN <= ORACLE_MEAN and ROUTE_IOU <= ORACLE_IOU

KINDS = {"point": 7, "box": 7, "two_points": 8, "box_point": 8, "one_token": 6, "no_token": 5}        # kind -> Nt
MODULE_KINDS = ("one_token", "no_token")                                                               # through sam.mask_decoder
# label patterns laid over the rows the oracle sees, so that every label value is among them whatever the random draw gives
LABELS_1 = [1, 0, 1, 0, -1, 1, 0, 1]
LABELS_2 = [(1, 1), (1, 0), (0, 1), (1, -1), (0, -1), (0, 0), (1, 1), (-1, 1)]


@contextlib.contextmanager
def _tune(**knobs):
    """msam_tune_set for the duration of a block; every knob of TUNE_DEFAULTS is back at the library's default afterwards."""
    from micro_sam_amd import _lib
    lib = _lib.load()
    try:
        for key, value in knobs.items():
            assert key in TUNE_DEFAULTS
            _lib.check(lib.msam_tune_set(key.encode(), value), "msam_tune_set")
        yield
    finally:
        for key, value in TUNE_DEFAULTS.items():
            lib.msam_tune_set(key.encode(), value)


@pytest.fixture(scope="module")
def ctx(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    predictor.set_image(util._to_image(synthetic_tile(5)))
    feats = predictor.get_image_embedding()
    with _tune():                                        # start from the defaults whatever ran before
        pass
    return dict(sd=vit_b_sd, predictor=predictor, sam=predictor.model, feats=feats, feats_cpu=feats.float().cpu(), oracle={},
                decoded={})


def _select(P):
    """Rows the oracle runs on (at most 8): first, last, both sides of the 4-prompt group boundary, of the 128-prompt boundary and of
    the 256-workgroup boundary where the launch has them, of the wave boundary, and one from the middle."""
    want = [0, P - 1, 3, 4, 127, 128, 255, 256, 63, 64, (P * 5) // 8 + 1, P - 2, P // 3]
    rows = []
    for r in want:
        if 0 <= r < P and r not in rows:
            rows.append(r)
    return sorted(rows[:8])


def _prompts(kind, P):
    """CPU prompts of a case: (points [P, n, 2] | None, labels [P, n] | None, boxes [P, 4] | None); labels mixed 1 / 0 / -1."""
    g = torch.Generator().manual_seed(7919 * list(KINDS).index(kind) + P)
    pts = lbl = bx = None
    if kind != "box" and kind != "no_token":
        n = 2 if kind == "two_points" else 1
        pts = torch.rand(P, n, 2, generator=g) * 1000 + 12
        lbl = (torch.rand(P, n, generator=g) > 0.35).to(torch.int)
        for k, r in enumerate(_select(P)):
            lbl[r] = torch.tensor(LABELS_2[k] if n == 2 else [LABELS_1[k]], dtype=torch.int)
    if kind in ("box", "box_point"):
        x0 = torch.rand(P, 2, generator=g) * 600 + 20
        bx = torch.cat([x0, x0 + torch.rand(P, 2, generator=g) * 350 + 30], dim=1)
    return pts, lbl, bx


def _decode(ctx, kind, P, multimask=True, rows=None, **kw):
    """Device decode of the case's prompts (the first ``rows`` of them when given) -> (low_res [P, C, 256, 256], iou [P, C])."""
    sam = ctx["sam"]
    pts, lbl, bx = _prompts(kind, P)
    n = P if rows is None else rows
    if kind in MODULE_KINDS:
        assert not kw
        if kind == "one_token":                          # the point's own token without its padding token: 5 + 1 tokens per prompt
            sparse, _ = sam.prompt_encoder((pts[:n].cuda(), lbl[:n].cuda()), None, None)
            sparse = sparse[:, :1].contiguous()
        else:
            sparse = torch.zeros(n, 0, 256, device="cuda")
        dense = sam.prompt_encoder.no_mask_embed.weight.detach().reshape(1, -1, 1, 1).expand(n, -1, 64, 64)
        return sam.mask_decoder(image_embeddings=ctx["feats"], image_pe=sam.prompt_encoder.get_dense_pe(),
                                sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=multimask)
    return sam.decode(ctx["feats"], None if pts is None else pts[:n].cuda(), None if lbl is None else lbl[:n].cuda(),
                      boxes=None if bx is None else bx[:n].cuda(), multimask_output=multimask, **kw)


def _oracle(ctx, kind, P, multimask):
    """(rows, logits of the HIP-like mode, its IoU predictions, logits of the fp32 mode) on the selected rows; computed once."""
    key = (kind, P, multimask)
    if key not in ctx["oracle"]:
        from oracle import sam_ref as S
        sd, feats = ctx["sd"], ctx["feats_cpu"]
        rows = _select(P)
        pts, lbl, bx = _prompts(kind, P)
        pts, lbl, bx = (None if t is None else t[rows] for t in (pts, lbl, bx))
        with torch.no_grad():
            if kind in MODULE_KINDS:
                if kind == "one_token":
                    sparse, dense = S.prompt_encoder(sd, (pts, lbl), None, None)
                    sparse = sparse[:, :1]
                else:
                    sparse = torch.zeros(len(rows), 0, 256)
                    dense = sd["prompt_encoder.no_mask_embed.weight"].reshape(1, -1, 1, 1).expand(len(rows), -1, 64, 64)
                pe = S.get_dense_pe(sd)
                low_b, iou_b = S.mask_decoder(sd, feats, pe, sparse, dense, multimask, precision="bf16")
                low_f, _ = S.mask_decoder(sd, feats, pe, sparse, dense, multimask, precision="fp32")
            else:
                _, iou_b, low_b = S.predict_torch(sd, feats, (1024, 1024), (1024, 1024), pts, lbl, boxes=bx, multimask_output=multimask,
                                                  return_logits=True, precision="bf16")
                _, _, low_f = S.predict_torch(sd, feats, (1024, 1024), (1024, 1024), pts, lbl, boxes=bx, multimask_output=multimask,
                                              return_logits=True)
        ctx["oracle"][key] = (rows, low_b, iou_b, low_f)
    return ctx["oracle"][key]


def _check_vs_oracle(ctx, kind, P, multimask, low, iou, what):
    """The assertions of test_decoder_vs_oracle on the selected rows of a device result."""
    rows, low_b, iou_b, low_f = _oracle(ctx, kind, P, multimask)
    assert low.shape == (P, 3 if multimask else 1, 256, 256) and iou.shape == (P, 3 if multimask else 1)
    assert bool(torch.isfinite(low).all()) and bool(torch.isfinite(iou).all()), f"{what}: non-finite output"
    lo, io = low[rows].float().cpu(), iou[rows].cpu()
    scale = low_b.abs().max().item()
    d = (lo - low_b).abs()
    per_row = {r: round(d[k].max().item() / scale, 4) for k, r in enumerate(rows)}
    d_iou = (io - iou_b).abs().max().item()
    dis_hip = ((lo > 0) != (low_f > 0)).float().mean().item()
    dis_orc = ((low_b > 0) != (low_f > 0)).float().mean().item()
    print(f"{what}: vs oracle max {d.max().item() / scale:.5f} mean {d.mean().item() / scale:.6f} of scale {scale:.2f}, iou {d_iou:.2e}, "
          f"sign disagreement with fp32 {dis_hip:.5f} (oracle's own {dis_orc:.5f}); per-row max {per_row}")
    assert d.max().item() <= ORACLE_MAX * scale and d.mean().item() <= ORACLE_MEAN * scale, (what, per_row)
    assert d_iou <= ORACLE_IOU, (what, (io - iou_b).abs().amax(dim=1).tolist(), rows)
    assert dis_hip <= 1.5 * dis_orc + 1e-3, (what, dis_hip, dis_orc)


def _distance(low_a, iou_a, low_b, iou_b):
    """(max, mean) |a - b| as shares of b's logit scale, max IoU-prediction difference; over all rows, on the device."""
    scale = low_b.abs().max().item()
    d = (low_a.float() - low_b.float()).abs()
    return d.max().item() / scale, d.mean().item() / scale, (iou_a - iou_b).abs().max().item()


def _check_distance(what, low_a, iou_a, low_b, iou_b):
    mx, mean, diou = _distance(low_a, iou_a, low_b, iou_b)
    worst = int((low_a.float() - low_b.float()).abs().flatten(1).amax(dim=1).argmax().item())
    print(f"{what}: max {mx:.6f} mean {mean:.7f} of the logit scale, iou {diou:.3e} (worst row {worst})")
    assert mx <= ROUTE_MAX and mean <= ROUTE_MEAN and diou <= ROUTE_IOU, (what, mx, mean, diou, worst)


# ---- 1. the chained decode against the oracle, over shape and output form

@pytest.mark.parametrize("multimask", [True, False])
@pytest.mark.parametrize("P", [128, 129, 131, 257])
@pytest.mark.parametrize("kind", list(KINDS))
def test_chained_decode_matches_the_oracle(ctx, kind, P, multimask):
    with _tune():
        low, iou = _decode(ctx, kind, P, multimask)
    _check_vs_oracle(ctx, kind, P, multimask, low, iou, f"chained {kind} Nt={KINDS[kind]} P={P} multimask={multimask}")


# ---- 2. the same prompts through both routes

@pytest.mark.parametrize("kind", ["point", "two_points"])
@pytest.mark.parametrize("P", [128, 131])
def test_chained_and_stage_by_stage_routes_agree(ctx, P, kind):
    with _tune(dec_chain=1):
        low1, iou1 = _decode(ctx, kind, P)
    with _tune(dec_chain=0):
        low0, iou0 = _decode(ctx, kind, P)
    _check_vs_oracle(ctx, kind, P, True, low1, iou1, f"chained Nt={KINDS[kind]} P={P}")
    _check_vs_oracle(ctx, kind, P, True, low0, iou0, f"stage-by-stage Nt={KINDS[kind]} P={P}")
    _check_distance(f"route distance Nt={KINDS[kind]} P={P}", low1, iou1, low0, iou0)      # bound: see ROUTE_MAX above


@pytest.mark.parametrize("kind", ["point", "two_points"])
def test_routes_agree_across_the_prompt_count_threshold(ctx, kind):
    """The same 127 prompts as a launch of 127 (stage-by-stage) and as the first 127 rows of a launch of 128 (chained)."""
    with _tune():
        low_c, iou_c = _decode(ctx, kind, 128)
        low_s, iou_s = _decode(ctx, kind, 128, rows=127)
    assert low_s.shape[0] == 127
    _check_distance(f"threshold 127 | 128 Nt={KINDS[kind]}", low_c[:127], iou_c[:127], low_s, iou_s)


# ---- 3. every build of the chained kernels inside the whole decoder

@pytest.mark.parametrize("variant", list(range(10)))
def test_every_chained_build_inside_the_decoder(ctx, variant):
    """decoder_run's two chained branches: "chain_variant" 9 = msam_i2t0_t2i_fused_v2 + msam_i2t_fold_operands_values, every other
    build = msam_i2t0_t2i_fused + msam_i2t_fold_operands (layer 0 as well)."""
    kind, P = "two_points", 129
    if "variant9" not in ctx["decoded"]:
        with _tune(chain_variant=9):
            ctx["decoded"]["variant9"] = _decode(ctx, kind, P)
    low9, iou9 = ctx["decoded"]["variant9"]
    with _tune(chain_variant=variant):
        low, iou = _decode(ctx, kind, P)
    _check_vs_oracle(ctx, kind, P, True, low, iou, f"chain_variant {variant}")
    _check_distance(f"chain_variant {variant} vs 9", low, iou, low9, iou9)


# ---- 4. fp16 logits on the chained route

@pytest.mark.parametrize("multimask", [True, False])
def test_fp16_logits_are_the_rounded_fp32_logits(ctx, multimask):
    """up_fused_kernel's output stage (csrc/upfused.hip, store_previous) holds one fp32 value per pixel and either stores it or stores
    pack2h of it - v_cvt_pk_f16_f32, round to nearest even (csrc/common.h) - so the fp16 logits are the rounded fp32 logits, bit for bit."""
    with _tune():
        low32, iou32 = _decode(ctx, "two_points", 129, multimask)
        low16, iou16 = _decode(ctx, "two_points", 129, multimask, low_res_dtype=torch.float16)
    assert low16.dtype == torch.float16 and low32.dtype == torch.float32
    assert torch.equal(low16, low32.to(torch.float16))
    assert torch.equal(iou16, iou32)


# ---- 5. workspace reuse and run-to-run state

def test_a_smaller_launch_after_a_larger_one_reads_nothing_stale(ctx):
    """The workspace only grows, and tables / tables2 / mfrag are carved relative to R = P * 4096: after a launch of 257 prompts a launch
    of 128 finds its constants' places full of the larger launch's data, and after an un-folded launch (Nt = 12) of the stage buffers'."""
    sam = ctx["sam"]
    g = torch.Generator().manual_seed(77)
    pts12 = (torch.rand(5, 6, 2, generator=g) * 1000 + 12).cuda()
    lbl12 = (torch.rand(5, 6, generator=g) > 0.3).to(torch.int).cuda()
    with _tune():
        sam._dec_ws = None                                               # (the order below decides what the buffer holds)
        low_a, iou_a = _decode(ctx, "two_points", 257)                   # chained, sizes the workspace
        size = sam._dec_ws.numel()
        low_b, iou_b = _decode(ctx, "point", 128)                        # chained
        low_c, iou_c = sam.decode(ctx["feats"], pts12, lbl12)            # un-folded: 5 + 6 + 1 tokens per prompt
        low_d, iou_d = _decode(ctx, "point", 128)                        # chained, the prompts of the second call
        assert sam._dec_ws.numel() == size
    assert low_c.shape == (5, 3, 256, 256) and bool(torch.isfinite(low_c).all())
    assert torch.equal(low_d, low_b) and torch.equal(iou_d, iou_b)
    _check_vs_oracle(ctx, "point", 128, True, low_d, iou_d, "chained P=128 after P=257 and an un-folded launch")
    _check_vs_oracle(ctx, "two_points", 257, True, low_a, iou_a, "chained P=257 on a fresh workspace")


def test_a_mask_prompt_decode_between_two_chained_decodes(ctx):
    """A mask prompt gives every prompt its own source: that launch writes w.keys itself and is never chained; the chained launch after
    it must not depend on anything it left behind."""
    sam = ctx["sam"]
    g = torch.Generator().manual_seed(78)
    pts = (torch.rand(3, 1, 2, generator=g) * 1000 + 12).cuda()
    lbl = torch.ones(3, 1, dtype=torch.int).cuda()
    masks = (torch.randn(3, 1, 256, 256, generator=g) * 4).cuda()
    with _tune():
        low_a, iou_a = _decode(ctx, "box_point", 129)
        low_m, iou_m = sam.decode(ctx["feats"], pts, lbl, mask_input=masks)
        low_b, iou_b = _decode(ctx, "box_point", 129)
    assert low_m.shape == (3, 3, 256, 256) and bool(torch.isfinite(low_m).all())
    assert torch.equal(low_b, low_a) and torch.equal(iou_b, iou_a)
    _check_vs_oracle(ctx, "box_point", 129, True, low_b, iou_b, "chained P=129 after a mask-prompt launch")
