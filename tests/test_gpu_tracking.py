"""tracking.track_objects_in_timeseries on the device.

The device path is compared, bit for bit, with a loop written here that visits the same frames with the same active sets but takes its
prompts, its motion and its gate from the HOST (``_compute_box_from_mask``, ``np.mean`` of ``np.where``, ``scipy.ndimage.shift``,
``util.compute_iou``; the mask prompts from ``ops.mask_logits`` after asserting that they agree with the host's outside the tie band),
decodes with one ``predict_torch`` call per frame and composes in numpy.  With one object and the box projection the result is pinned to
``track_mask_in_timeseries`` itself (a batch of one on both sides).  Whether N > 1 objects equal N per-object calls depends on the
decoder being batch-invariant; that is measured, not asserted here.

The scene, 6 frames of 480 x 500: A is annotated in frames 0 and 1, displaced by (+3, -5) - its motion at frame 2 is (3, -5) by
construction; B in frame 1 only; C in frames 0 and 3 (frames 1 and 2 are tracked without a gate); D is a small disk 4 pixels from the
upper border that moves towards it, so its moved mask is clipped; E has a "division" at its second annotation."""
import numpy as np
import pytest
import torch

import propagate_ref as R
import track_ref as T

pytestmark = pytest.mark.gpu
SHAPE = (480, 500)
FRAMES = 6


def _disk(center, radius, shape=SHAPE):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((yy - center[0]) ** 2 + (xx - center[1]) ** 2 < radius * radius).astype("uint8")


#        object, id, [(frame, centre, radius, state)]
SCENE = [("A", 4, [(0, (200, 260), 40, "track"), (1, (203, 255), 40, "track")]),
         ("B", 9, [(1, (100, 400), 41, "track")]),
         ("C", 30, [(0, (400, 80), 30, "track"), (3, (404, 86), 30, "track")]),
         ("D", 2, [(0, (12, 250), 9, "track"), (1, (9, 250), 9, "track")]),
         ("E", 17, [(0, (330, 330), 35, "track"), (2, (332, 333), 35, "division")])]


def _seeds(names="ABCDE"):
    seeds, frames, ids, states = [], [], [], []
    for name, i, notes in SCENE:
        if name in names:
            for t, c, r, state in notes:
                seeds.append(_disk(c, r)); frames.append(t); ids.append(i); states.append(state)
    return np.stack(seeds), np.array(frames), np.array(ids), states


@pytest.fixture(scope="module")
def ctx(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    series = np.stack([synthetic_tile(60 + t, SHAPE) for t in range(FRAMES)])
    emb = util.precompute_image_embeddings(predictor, series, ndim=3, verbose=False)
    return dict(predictor=predictor, emb=emb)


def test_the_scene_exercises_the_motion_and_the_clipping():
    """On the CPU side, from the annotations alone: A's motion at frame 2 is exactly (3, -5) and moves its bits; D's moved mask loses
    pixels at the border."""
    seeds, frames, ids, _ = _seeds()
    a0, a1 = seeds[0], seeds[1]
    motion = T.center(a1) - T.center(a0)
    assert motion.tolist() == [3.0, -5.0]
    moved = T.shift_ref(a1[None], motion[None])[0]
    assert not np.array_equal(moved, a1) and np.array_equal(moved, _disk((206, 250), 40))
    d0, d1 = seeds[5], seeds[6]
    assert ids[5] == ids[6] == 2 and np.flatnonzero(d0.any(axis=1))[0] == 4 and (T.center(d1) - T.center(d0)).tolist() == [-3.0, 0.0]
    assert 0 < T.shift_ref(d1[None], np.array([[-3.0, 0.0]]))[0].sum() < d1.sum()


def _manual(ctx, seeds, seed_frames, seed_ids, states, thr, projection, ext=0.0, alpha=0.5, stop=False, log=None):
    """The sweep of track_objects_in_timeseries with host prompts, host motion models, a host gate and numpy composition."""
    from micro_sam_amd import multi_dimensional_segmentation as M
    from micro_sam_amd import ops, util
    from micro_sam_amd.prompt_based_segmentation import _compute_box_from_mask
    p, emb = ctx["predictor"], ctx["emb"]
    use_box, use_mask, use_points, _ = M._validate_projection(projection)
    assert not use_points
    ids = np.unique(seed_ids)
    n_obj, (h, w) = len(ids), seeds.shape[1:]
    notes = [{int(t): m for m, t in enumerate(seed_frames) if seed_ids[m] == i} for i in ids]
    first, last = np.array([min(d) for d in notes]), np.array([max(d) for d in notes])
    stop = np.broadcast_to(np.asarray(stop), (n_obj,))
    vols = np.zeros((n_obj, FRAMES, h, w), np.uint8)
    for n, d in enumerate(notes):
        for t, m in d.items():
            vols[n, t] = seeds[m] == 1
    alive, motion, division = [True] * n_obj, [None] * n_obj, np.zeros(n_obj, bool)
    for t in range(int(first.min()) + 1, FRAMES):
        active = []
        for n in range(n_obj):
            if not alive[n] or first[n] >= t:
                continue
            if not vols[n, t - 1].any():
                alive[n] = False
                continue
            if t >= first[n] + 2:
                move = T.center(vols[n, t - 1]) - T.center(vols[n, t - 2])
                motion[n] = move if t == first[n] + 2 else alpha * motion[n] + (1 - alpha) * move
            active.append(n)
        tracked = [n for n in active if t not in notes[n]]
        for n in active:
            if t in notes[n] and states[notes[n][t]] == "division":
                division[n], alive[n] = True, False
        if tracked:
            util.set_precomputed(p, emb, i=t)
            prev = np.stack([vols[n, t - 1] if motion[n] is None else T.shift_ref(vols[n, t - 1][None], motion[n][None])[0] for n in tracked])
            nonempty = prev.reshape(len(prev), -1).any(axis=1)
            boxes = lg = None
            if use_box:
                host = np.stack([_compute_box_from_mask(m, box_extension=ext) if ok else np.zeros(4, int) for m, ok in zip(prev, nonempty)])
                boxes = torch.as_tensor(p.transform.apply_boxes(host, p.original_size), dtype=torch.float, device=p.device)
            if use_mask:
                lg = ops.mask_logits(ops.pack_bits(torch.from_numpy(prev).cuda()), h, w)
                values = R.resized64(prev)
                R.check_logits(lg.cpu().numpy(), values, f"frame {t}")
                R.check_logits(R.host_logits(prev), values, f"frame {t} (host)")         # so both agree outside the band
                lg = lg[:, None]
            masks, _, _ = p.predict_torch(None, None, boxes, lg, multimask_output=False)
            new = masks[:, 0].cpu().numpy()
            for k, n in enumerate(tracked):
                if not nonempty[k]:
                    alive[n] = False
                    continue
                if t > last[n] and thr is not None:
                    iou = util.compute_iou(prev[k], new[k])
                    if log is not None:
                        log.append((int(ids[n]), t, iou))
                    if iou < thr:
                        alive[n] = False
                        continue
                vols[n, t] = new[k]
        for n in active:
            if stop[n] and last[n] == t + 1:
                alive[n] = False
    labels = np.zeros((FRAMES, h, w), np.int32)
    centers = np.full((n_obj, FRAMES, 2), np.nan)
    ranges = np.zeros((n_obj, 2), np.int64)
    for n in range(n_obj):
        labels[vols[n] == 1] = ids[n]
        held = [t for t in range(FRAMES) if vols[n, t].any()]
        for t in held:
            centers[n, t] = T.center(vols[n, t])
        ranges[n] = (held[0], held[-1])
    return labels, ids, ranges, division, centers


def _same(got, want):
    assert got.labels.dtype == np.int32 and got.labels.shape == (FRAMES,) + SHAPE and got.ranges.dtype == np.int64
    assert np.array_equal(got.ids, want[1]) and np.array_equal(got.has_division, want[3])
    assert np.array_equal(got.ranges, want[2]), (got.ranges.tolist(), want[2].tolist())
    assert np.array_equal(got.centers, want[4], equal_nan=True)
    assert np.array_equal(got.labels, want[0])


@pytest.mark.parametrize("projection", ["mask", "box", {"use_box": False, "use_mask": True, "use_points": False}],
                         ids=["mask", "box", "dict-mask-only"])
def test_same_batches_with_host_prompts(ctx, projection):
    from micro_sam_amd import tracking
    seeds, frames, ids, states = _seeds()
    p, emb = ctx["predictor"], ctx["emb"]
    assert tracking._can_propagate_on_device(p, emb, False)
    log = []
    want = _manual(ctx, seeds, frames, ids, states, 1e-6, projection, 0.025, log=log)           # a threshold that stops (almost) nothing
    got = tracking.track_objects_in_timeseries(p, emb, seeds, frames, ids, 1e-6, projection, box_extension=0.025, seed_states=states)
    _same(got, want)
    print("gated IoUs:", [(i, t, round(v, 4)) for i, t, v in log])
    print("ranges:", got.ranges.tolist(), "divisions:", got.has_division.tolist())
    assert got.has_division.tolist() == [i == 17 for i in got.ids] and got.ids.tolist() == [2, 4, 9, 17, 30]
    assert not (got.labels[3:] == 17).any() and np.array_equal(got.centers[3, 2], [332.0, 333.0])      # E ends at its division, which stays
    # a threshold halfway between the two smallest gated IoUs of that run: one object provably stops there
    values = sorted({v for _, _, v in log})
    assert len(values) >= 2, values
    thr = (values[0] + values[1]) / 2
    want2 = _manual(ctx, seeds, frames, ids, states, thr, projection, 0.025)
    assert (want2[2] != want[2]).any(), "the threshold stops no object"
    got2 = tracking.track_objects_in_timeseries(p, emb, seeds, frames, ids, thr, projection, box_extension=0.025, seed_states=states)
    _same(got2, want2)
    # chunks of two, labels left on the device, seeds given as a device tensor, the seeds in another order: the same tracks
    order = np.array([6, 2, 0, 7, 4, 1, 5, 3, 8])
    dev = tracking.track_objects_in_timeseries(p, emb, torch.from_numpy(seeds[order]).cuda(), frames[order], ids[order], thr, projection,
                                               box_extension=0.025, seed_states=[states[m] for m in order], batch_size=2, return_device=True)
    assert dev.labels.is_cuda and dev.labels.dtype == torch.int32 and np.array_equal(dev.ids, want2[1])
    if not np.array_equal(dev.labels.cpu().numpy(), want2[0]):            # (equal only if the decoder is batch-invariant: reported, not asserted)
        print("batch_size=2 differs from batch_size=64 in", int((dev.labels.cpu().numpy() != want2[0]).sum()), "pixels")


def test_stop_upper_and_another_smoothing(ctx):
    from micro_sam_amd import tracking
    seeds, frames, ids, states = _seeds("ABC")
    stop = [False, False, True]                                       # C (id 30) ends in front of its annotation in frame 3
    want = _manual(ctx, seeds, frames, ids, states, 1e-6, "box", alpha=0.25, stop=stop)
    got = tracking.track_objects_in_timeseries(ctx["predictor"], ctx["emb"], seeds, frames, ids, 1e-6, "box", motion_smoothing=0.25,
                                               stop_upper=stop, seed_states=states)
    _same(got, want)
    assert got.ranges[2].tolist() == [0, 3] and not (got.labels[4:] == 30).any()


def test_one_object_equals_track_mask_in_timeseries(ctx):
    from micro_sam_amd import tracking
    p, emb = ctx["predictor"], ctx["emb"]
    seeds, frames, ids, states = _seeds("A")
    for thr, ext in ((0.05, 0.0), (0.05, 0.25), (1.01, 0.0), (None, 0.0)):
        seg = np.zeros((FRAMES,) + SHAPE, np.uint8)
        seg[frames] = seeds
        want, division = tracking.track_mask_in_timeseries(seg, p, emb, frames, False, thr, "box", box_extension=ext)
        got = tracking.track_objects_in_timeseries(p, emb, seeds, frames, [7, 7], thr, "box", box_extension=ext)
        assert np.array_equal(got.labels, want.astype(np.int32) * 7) and not division and not got.has_division[0], (thr, ext)
        held = [t for t in range(FRAMES) if want[t].any()]
        assert got.ranges.tolist() == [[held[0], held[-1]]]
        assert np.array_equal(got.centers[0, held], np.stack([T.center(want[t]) for t in held]))
    assert got.ranges[0, 0] == 0


def test_point_projections_take_the_per_object_loop(ctx):
    from micro_sam_amd import tracking
    p, emb = ctx["predictor"], ctx["emb"]
    seeds, frames, ids, states = _seeds("B")
    assert not tracking._can_propagate_on_device(p, emb, True)
    seg = np.zeros((FRAMES,) + SHAPE, np.uint8)
    seg[frames] = seeds
    want, _ = tracking.track_mask_in_timeseries(seg, p, emb, frames, False, 0.05, "single_point")
    got = tracking.track_objects_in_timeseries(p, emb, seeds, frames, ids, 0.05, "single_point")
    assert np.array_equal(got.labels, want.astype(np.int32) * 9) and got.ids.tolist() == [9]
