"""multi_dimensional_segmentation.segment_objects_in_volume and evaluation/multi_dimensional_segmentation.py on the device.

The device path is compared, bit for bit, with a loop written here that walks the same slices with the same active sets but takes its
prompts and its gate from the HOST functions (``_compute_box_from_mask``, ``util.compute_iou``; the mask prompts from ``ops.mask_logits``
after asserting that they agree with the host's outside the tie band), decodes with one ``predict_torch`` call per slice and composes
in numpy.  With one object and the box projection the result is pinned to ``segment_mask_in_volume`` itself (a batch of one on both
sides).  Whether N > 1 objects equal N per-object calls depends on the decoder being batch-invariant; that is measured,
not asserted here."""
import os

import numpy as np
import pytest
import torch

import propagate_ref as R

pytestmark = pytest.mark.gpu
SHAPE = (480, 500)
Z = 4


def _disk(center, radius, shape=SHAPE):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((yy - center[0]) ** 2 + (xx - center[1]) ** 2 < radius * radius).astype("uint8")


@pytest.fixture(scope="module")
def ctx(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    volume = np.stack([synthetic_tile(60 + z, SHAPE) for z in range(Z)])
    emb = util.precompute_image_embeddings(predictor, volume, ndim=3, verbose=False)
    seeds = np.stack([_disk((250, 260), 70), _disk((100, 390), 41), _disk((400, 80), 9)])
    return dict(predictor=predictor, volume=volume, emb=emb, seeds=seeds, slices=np.array([1, 2, 1]), ids=np.array([4, 9, 30]))


def _manual(ctx, seeds, seed_slices, ids, thr, projection, ext=0.0, log=None):
    """The walk of segment_objects_in_volume with host prompts, a host gate and numpy composition."""
    from micro_sam_amd import multi_dimensional_segmentation as M
    from micro_sam_amd import ops, util
    from micro_sam_amd.prompt_based_segmentation import _compute_box_from_mask
    p, emb = ctx["predictor"], ctx["emb"]
    use_box, use_mask, use_points, _ = M._validate_projection(projection)
    assert not use_points
    n_obj, h, w = seeds.shape
    vols = np.zeros((n_obj, Z, h, w), np.uint8)
    vols[np.arange(n_obj), seed_slices] = seeds == 1
    ranges = np.stack([seed_slices, seed_slices], axis=1).astype(np.int64)
    for direction in (1, -1):
        cur = [s == 1 for s in seeds]
        alive = [bool(c.any()) for c in cur]
        for z in (range(1, Z) if direction == 1 else range(Z - 2, -1, -1)):
            active = [n for n in range(n_obj) if alive[n] and (seed_slices[n] < z if direction == 1 else seed_slices[n] > z)]
            if not active:
                continue
            util.set_precomputed(p, emb, i=z)
            prev = np.stack([cur[n] for n in active]).astype(np.uint8)
            boxes = lg = None
            if use_box:
                host = np.stack([_compute_box_from_mask(m, box_extension=ext) for m in prev])
                boxes = torch.as_tensor(p.transform.apply_boxes(host, p.original_size), dtype=torch.float, device=p.device)
            if use_mask:
                lg = ops.mask_logits(ops.pack_bits(torch.from_numpy(prev).cuda()), h, w)
                values = R.resized64(prev)
                R.check_logits(lg.cpu().numpy(), values, f"slice {z}")
                R.check_logits(R.host_logits(prev), values, f"slice {z} (host)")         # so both agree outside the band
                lg = lg[:, None]
            masks, _, _ = p.predict_torch(None, None, boxes, lg, multimask_output=False)
            new = masks[:, 0].cpu().numpy()
            for k, n in enumerate(active):
                iou = util.compute_iou(prev[k], new[k])
                if log is not None:
                    log.append((n, z, direction, iou))
                if iou < thr:
                    alive[n] = False
                    continue
                vols[n, z] = new[k]
                ranges[n, 1 if direction == 1 else 0] = z
                cur[n] = new[k]
                alive[n] = bool(new[k].any())
    labels = np.zeros((Z, h, w), np.int32)
    for n in np.argsort(ids):
        labels[vols[n] == 1] = ids[n]
    return labels, ranges


def test_tie_band_of_the_seed_disks_is_empty(ctx):
    values = R.resized64(ctx["seeds"][:2])
    assert not R.tie_band(values).any()


@pytest.mark.parametrize("projection", ["mask", "box", {"use_box": False, "use_mask": True, "use_points": False}],
                         ids=["mask", "box", "dict-mask-only"])
def test_same_batches_with_host_prompts(ctx, projection):
    from micro_sam_amd import multi_dimensional_segmentation as M
    seeds, slices, ids = ctx["seeds"], ctx["slices"], ctx["ids"]
    log = []
    want, want_ranges = _manual(ctx, seeds, slices, ids, 1e-6, projection, 0.025, log)         # a threshold that stops (almost) nothing
    got, ranges = M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, slices, ids, 1e-6, projection, box_extension=0.025)
    assert got.dtype == np.int32 and got.shape == (Z,) + SHAPE and ranges.dtype == np.int64
    assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges)
    print("IoUs of the steps:", [(n, z, d, round(i, 4)) for n, z, d, i in log])
    # a threshold between the two smallest IoUs of the FIRST steps (which do not depend on the threshold): that object stops there
    first = sorted({i for n, z, d, i in log if z == slices[n] + d})
    assert len(first) >= 2, first
    thr = (first[0] + first[1]) / 2
    want, want_ranges = _manual(ctx, seeds, slices, ids, thr, projection, 0.025)
    full = np.stack([np.where(slices > 0, 0, slices), np.where(slices < Z - 1, Z - 1, slices)], axis=1)
    assert (want_ranges != full).any(), "the threshold stops no object before the end"
    assert (want_ranges != np.stack([slices, slices], axis=1)).any(), "the threshold stops every object at once"
    got, ranges = M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, slices, ids, thr, projection, box_extension=0.025)
    assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges)
    # chunks of two, labels left on the device, seeds given as a device tensor: the same volume
    dev, ranges2 = M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], torch.from_numpy(seeds).cuda(), slices, ids, thr, projection,
                                               box_extension=0.025, batch_size=2, return_device=True)
    assert dev.is_cuda and dev.dtype == torch.int32 and np.array_equal(ranges2, want_ranges)
    if not np.array_equal(dev.cpu().numpy(), want):                       # (equal only if the decoder is batch-invariant: reported, not asserted)
        print("batch_size=2 differs from batch_size=64 in", int((dev.cpu().numpy() != want).sum()), "pixels")


def test_one_object_equals_segment_mask_in_volume(ctx):
    from micro_sam_amd import multi_dimensional_segmentation as M
    p, emb = ctx["predictor"], ctx["emb"]
    for thr, ext in ((0.05, 0.0), (0.05, 0.25), (1.01, 0.0)):
        seg = np.zeros((Z,) + SHAPE, np.uint8)
        seg[1] = ctx["seeds"][0]
        want, want_range = M.segment_mask_in_volume(seg, p, emb, np.array(1), False, False, thr, "box", box_extension=ext)
        got, ranges = M.segment_objects_in_volume(p, emb, ctx["seeds"][:1], [1], [7], thr, "box", box_extension=ext)
        assert np.array_equal(got, want.astype(np.int32) * 7) and tuple(ranges[0]) == tuple(want_range), (thr, ext)
    assert tuple(ranges[0]) == (1, 1)


def test_seeds_in_the_first_and_the_last_slice_walk_one_way(ctx):
    from micro_sam_amd import multi_dimensional_segmentation as M
    seeds, slices, ids = ctx["seeds"][:2], np.array([0, Z - 1]), np.array([2, 3])
    want, want_ranges = _manual(ctx, seeds, slices, ids, 1e-6, "box")
    got, ranges = M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, slices, ids, 1e-6, "box")
    assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges)
    assert ranges[0, 0] == 0 and ranges[1, 1] == Z - 1
    assert np.array_equal(got[0] == 2, (seeds[0] == 1) & (got[0] != 3)) and np.array_equal(got[Z - 1] == 3, seeds[1] == 1)


def test_overlapping_objects_resolve_to_the_larger_id(ctx):
    from micro_sam_amd import multi_dimensional_segmentation as M
    seeds = np.stack([_disk((250, 260), 70), _disk((250, 300), 60)])
    slices, ids = np.array([1, 1]), np.array([4, 9])
    got, ranges = M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, slices, ids, 1.01, "box")
    assert np.array_equal(ranges, [[1, 1], [1, 1]]) and not got[0].any() and not got[2].any()
    both = (seeds[0] == 1) & (seeds[1] == 1)
    assert both.any() and (got[1][both] == 9).all() and (got[1][(seeds[0] == 1) & ~both] == 4).all() and (got[1][seeds[1] == 1] == 9).all()
    want, want_ranges = _manual(ctx, seeds, slices, ids, 1e-6, "mask")
    got, ranges = M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, slices, ids, 1e-6, "mask")
    assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges)
    with pytest.raises(ValueError, match="ascending"):
        M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, slices, [9, 4], 0.5, "box")
    with pytest.raises(ValueError, match="seed_slices"):
        M.segment_objects_in_volume(ctx["predictor"], ctx["emb"], seeds, [1, Z], ids, 0.5, "box")


@pytest.mark.parametrize("projection,thr", [("single_point", 0.05), ("points", 1.01)])
def test_point_projections_take_the_per_object_loop(ctx, projection, thr):
    from micro_sam_amd import multi_dimensional_segmentation as M
    p, emb = ctx["predictor"], ctx["emb"]
    seeds, slices, ids = ctx["seeds"][1:], np.array([2, 1]), np.array([9, 30])
    assert not M._can_propagate_on_device(p, emb, True) and M._can_propagate_on_device(p, emb, False)
    want = np.zeros((Z,) + SHAPE, np.int32)
    want_ranges = []
    for n in range(2):
        seg = np.zeros((Z,) + SHAPE, np.uint8)
        seg[slices[n]] = seeds[n]
        seg, rng = M.segment_mask_in_volume(seg, p, emb, np.array(slices[n]), False, False, thr, projection)
        want[seg == 1] = ids[n]
        want_ranges.append(rng)
    got, ranges = M.segment_objects_in_volume(p, emb, seeds, slices, ids, thr, projection)
    assert np.array_equal(got, want) and np.array_equal(ranges, np.array(want_ranges))


def _ellipsoids():
    gt = np.zeros((Z,) + SHAPE, np.int32)
    zz, yy, xx = np.mgrid[0:Z, 0:SHAPE[0], 0:SHAPE[1]]
    for label, (cz, cy, cx), (rz, ry, rx) in ((1, (1.5, 240, 250), (2.4, 90, 110)), (2, (2.0, 90, 400), (1.2, 50, 60)),
                                              (3, (0.0, 420, 70), (0.8, 12, 12))):
        gt[((zz - cz) / rz) ** 2 + ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0] = label
    return gt


def test_segment_slices_from_ground_truth_scores_its_volume(ctx):
    from micro_sam_amd import evaluation
    gt = _ellipsoids()
    kw = dict(predictor=ctx["predictor"], image_embeddings=ctx["emb"])
    results, seg = evaluation.segment_slices_from_ground_truth(ctx["volume"], gt, "vit_b", iou_threshold=0.3, projection="box",
                                                              return_segmentation=True, **kw)
    assert seg.shape == gt.shape and seg.dtype == gt.dtype and set(np.unique(seg)) <= {0, 1, 2, 3}
    msa, sa = evaluation.evaluation.mean_segmentation_accuracy(seg, gt, return_accuracies=True)
    assert results == {"mSA": msa, "SA50": sa[0], "SA75": sa[5]}
    # the small object is below min_size in its middle slice: neither segmented nor counted as a miss
    results_min, seg_min = evaluation.segment_slices_from_ground_truth(ctx["volume"], gt, "vit_b", iou_threshold=0.3, projection="box",
                                                                      return_segmentation=True, min_size=1000, **kw)
    assert 3 not in np.unique(seg_min)
    cut = np.where(gt == 3, 0, gt)
    assert results_min["mSA"] == evaluation.evaluation.mean_segmentation_accuracy(seg_min, cut)
    dice = evaluation.segment_slices_from_ground_truth(ctx["volume"], gt, "vit_b", iou_threshold=0.3, projection="box",
                                                      evaluation_metric="dice", **kw)
    inter = ((seg > 0) & (gt > 0)).sum()
    assert dice == {"Dice": 2.0 * inter / ((seg > 0).sum() + (gt > 0).sum() + 1e-7)}


def test_grid_search_on_the_device(ctx, tmp_path):
    import pandas as pd
    from micro_sam_amd import evaluation
    gt = _ellipsoids()
    grid = {"iou_threshold": [0.2, 0.6], "projection": ["mask", "box"], "box_extension": [0.0, 0.1]}
    best = evaluation.run_multi_dimensional_segmentation_grid_search(ctx["volume"], gt, "vit_b", None, None, str(tmp_path),
                                                                    grid_search_values=grid, predictor=ctx["predictor"],
                                                                    image_embeddings=ctx["emb"])
    rows = pd.read_csv(os.path.join(str(tmp_path), "all_grid_search_results.csv"))
    assert best == os.path.join(str(tmp_path), "grid_search_params_multi_dimensional_segmentation.csv") and len(rows) == 8
    top = pd.read_csv(best).iloc[0]
    assert top["mSA"] == pytest.approx(rows["mSA"].max())
    match = rows[(rows["iou_threshold"] == top["iou_threshold"]) & (rows["projection"] == top["projection"]) &
                 (rows["box_extension"] == top["box_extension"])]
    assert len(match) == 1 and match.iloc[0]["mSA"] == pytest.approx(rows["mSA"].max())
