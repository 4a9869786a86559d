"""The range map of the low-res logits on the device: msam_upscale_fused_range writes the exact {min, max} of every 64-pixel segment
next to unchanged logits, msam_postprocess_masks_range gives msam_postprocess_masks16's outputs word for word (x4 path and fallback),
and the mask generator's records do not depend on the "amg_range_map" knob."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def test_upscale_fused_range_writes_the_exact_map_next_to_the_same_logits():
    _gpu()
    from micro_sam_amd import _lib, ops
    lib, dev = _lib.load(), torch.device("cuda")
    d16 = _lib.decoder_dtype()
    g = torch.Generator().manual_seed(31)
    P, mask0, nmask = 3, 1, 3
    keys = torch.randn(P, 4096, 256, generator=g).to(d16).to(dev)
    w1f = torch.randn(256, 256, generator=g) / 16; b1f = torch.randn(64, generator=g).repeat(4)
    lw = (torch.randn(64, generator=g) * 0.2 + 1).to(dev); lb = (torch.randn(64, generator=g) * 0.3).to(dev)
    w2 = (torch.randn(128, 64, generator=g) / 8).to(d16).to(dev); b2 = torch.randn(32, generator=g).to(dev)
    hyper = torch.randn(P, 4, 128, generator=g).to(dev)
    for centred in (True, False):
        if centred:
            w1, b1 = ops.upscale_centre_weights(w1f, b1f)
            w1, b1 = w1.to(dev), b1.to(dev)
        else:
            w1, b1 = w1f.to(d16).to(dev), b1f.to(dev)
        plain = ops.upscale_fused(keys, w1, b1, lw, lb, w2, b2, hyper, mask0, nmask, centred=centred)
        SENT = -12345.5
        guard = 64
        buf = torch.full((guard + P * nmask * 256 * 4 * 2 + guard,), SENT, dtype=torch.float32, device=dev)
        rng = buf[guard:-guard]
        out = torch.full((P, nmask, 256, 256), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(lib.msam_upscale_fused_range(keys.data_ptr(), 2 if centred else 0, P, w1.data_ptr(), b1.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-6,
                                                w2.data_ptr(), b2.data_ptr(), hyper.data_ptr(), 128, mask0, nmask, out.data_ptr(), _lib.F32,
                                                rng.data_ptr(), _lib.stream_ptr()), "msam_upscale_fused_range")
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), "the map launch changed the logits"
        assert bool((buf[:guard] == SENT).all()) and bool((buf[-guard:] == SENT).all()), "a store outside the map"
        assert bool((rng != SENT).all()), "map entries that were never written"
        seg = out.reshape(P, nmask, 256, 4, 64)
        want = torch.stack([seg.amin(-1), seg.amax(-1)], -1)
        assert torch.equal(rng.reshape(P, nmask, 256, 4, 2), want)
    # fp16 logits carry no map
    out16 = torch.empty((P, nmask, 256, 256), dtype=torch.float16, device=dev)
    assert lib.msam_upscale_fused_range(keys.data_ptr(), 0, P, w1.data_ptr(), b1.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-6, w2.data_ptr(),
                                        b2.data_ptr(), hyper.data_ptr(), 128, mask0, nmask, out16.data_ptr(), _lib.F16, rng.data_ptr(),
                                        _lib.stream_ptr()) == 1


def _masks(dev):
    from test_range_map_host_emulation import crafted_masks, true_map
    low = crafted_masks(0.0, 1.0)
    g = torch.Generator().manual_seed(41)
    smooth = F.avg_pool2d(torch.randn(1, 6, 256, 256, generator=g) * 3, 9, stride=1, padding=4)[0] * 12 - 6          # object-like: mostly far from 0
    smooth[4] = smooth[4] * 0.1                                                                                # ... and one inside the +-1 band
    low = np.concatenate([low, smooth.numpy().astype(np.float32)])
    return torch.from_numpy(low).to(dev), torch.from_numpy(true_map(low)).to(dev)


def test_postprocess_masks_range_equals_postprocess_masks16():
    _gpu()
    from micro_sam_amd import ops
    low, rng = _masks(torch.device("cuda"))
    assert low.shape[0] >= 8
    for thr, off in ((0.0, 1.0), (0.0, 0.0)):
        ref = ops.postprocess_masks(low, (1024, 1024), (1024, 1024), thr, off)
        loose = rng.clone()
        loose[..., 0] -= 0.75; loose[..., 1] += 0.75
        for m in (rng, loose):
            got = ops.postprocess_masks(low, (1024, 1024), (1024, 1024), thr, off, range_map=m)
            for k in ("counts", "boxes", "bits"):
                assert torch.equal(got[k], ref[k]), (k, thr, off)
    assert ref["counts"][1].tolist() == [1024 * 1024] * 3 and ref["boxes"][1].tolist() == [0, 0, 1023, 1023]
    from test_range_map_host_emulation import edge_words_are_set
    assert edge_words_are_set(ref["bits"].cpu().numpy().view(np.uint32))      # the words only the row halo / the neighbour segment reaches
    # a NaN entry of the map leaves its words unsettled
    nan_map = rng.clone()
    nan_map[0, 100:104, 1, 0] = float("nan"); nan_map[1, 17, 2, 1] = float("nan")
    got = ops.postprocess_masks(low, (1024, 1024), (1024, 1024), 0.0, 0.0, range_map=nan_map)
    for k in ("counts", "boxes", "bits"):
        assert torch.equal(got[k], ref[k]), (k, "NaN map")
    # not 1024 x 1024: the map is ignored (the two-stage kernel, and the x4 kernel on a smaller frame)
    for in_hw, out_hw in (((683, 1024), (400, 600)), ((1024, 768), (1024, 768))):
        ref = ops.postprocess_masks(low[-2:], in_hw, out_hw, 0.0, 1.0)
        got = ops.postprocess_masks(low[-2:], in_hw, out_hw, 0.0, 1.0, range_map=rng[-2:].contiguous())
        for k in ("counts", "boxes", "bits"):
            assert torch.equal(got[k], ref[k]), (k, in_hw, out_hw)
    with pytest.raises((ValueError, TypeError)):
        ops.postprocess_masks(low, (1024, 1024), (1024, 1024), 0.0, 1.0, range_map=rng[:, :, :2])


def test_mask_generator_records_do_not_depend_on_the_range_map(vit_b_sd):
    _gpu()
    from micro_sam_amd import _lib, ops, util
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator
    from micro_sam_amd.synthetic import synthetic_tile
    p = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    tile = synthetic_tile(0)
    emb = util.precompute_image_embeddings(p, tile, verbose=False)
    recs, maps = {}, {1: [], 0: []}
    real = ops.postprocess_masks
    knob = [1]

    def spy(low_res, *a, range_map=None, **kw):          # what predict_masks_device hands the post-processing
        if range_map is not None:
            seg = low_res.reshape(-1, 256, 4, 64)
            assert torch.equal(range_map, torch.stack([seg.amin(-1), seg.amax(-1)], -1)), "the map handed over is not that of the logits"
        maps[knob[0]].append(range_map is not None)
        return real(low_res, *a, range_map=range_map, **kw)

    ops.postprocess_masks = spy
    try:
        for knob[0] in (1, 0):
            _lib.check(_lib.load().msam_tune_set(b"amg_range_map", knob[0]), "msam_tune_set")
            assert _lib.tune_get("amg_range_map") == knob[0]
            amg = AutomaticMaskGenerator(p, points_per_side=8)
            amg.initialize(tile, emb)
            recs[knob[0]] = amg.crop_list[0]
    finally:
        ops.postprocess_masks = real
        _lib.load().msam_tune_set(b"amg_range_map", 1)
    assert maps[1] and all(maps[1]), "knob 1: the generator's calls must take the map path"
    assert maps[0] and not any(maps[0]), "knob 0: none may"
    a, b = recs[1], recs[0]
    assert len(a["iou_preds"]) == len(b["iou_preds"]) > 0
    for k in ("iou_preds", "stability_score", "boxes", "bits"):
        assert torch.equal(a[k], b[k]), k
