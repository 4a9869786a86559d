"""micro_sam_amd/tracking.py without a GPU: ``track_mask_in_timeseries`` with a stub predictor (tests/track_ref.StubPredictor: the
"decoder" answers a box prompt with the box moved and shrunk by a per-frame script) against the pure-Python walk of tests/track_ref.py -
the motion model taken at t0 + 2 and smoothed afterwards, the gate applied only past the last annotated frame, ``stop_upper``, a
division, the empty-mask stop in both its forms, the end of the series - and ``track_objects_in_timeseries`` on its host route (the
stub has no device decoder) against N such walks composed in ascending id order, with its argument errors."""
import numpy as np
import pytest

import track_ref as T

SHAPE = (40, 60)
FRAMES = 8


def _rect(y0, y1, x0, x1):
    m = np.zeros(SHAPE, np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _series(annotations):
    seg = np.zeros((FRAMES,) + SHAPE, np.uint8)
    for t, m in annotations.items():
        seg[t] = m
    return seg


def _both(annotations, script, stop_upper=False, threshold=None, states=None, alpha=0.5):
    """The package's walk and the reference walk on the same series: (result, has_division, decoder calls, log of the reference)."""
    from micro_sam_amd import tracking
    frames = np.array(sorted(annotations))
    log = []
    want, want_div = T.walk(_series(annotations), frames, stop_upper, threshold, script, alpha=alpha, states=states, log=log)
    predictor = T.StubPredictor(SHAPE, script)
    seg = _series(annotations)
    got, got_div = tracking.track_mask_in_timeseries(seg, predictor, T.stub_embeddings(FRAMES, SHAPE), frames, stop_upper, threshold, "box",
                                                     motion_smoothing=alpha, frame_states=states)
    assert got is seg and got_div == want_div and np.array_equal(got, want)
    assert predictor.calls == [(t, box) for t, _, _, box in log if box is not None]          # the same prompts in the same frames
    return got, got_div, predictor.calls, log


def test_motion_is_taken_at_the_third_frame_and_smoothed_afterwards():
    script = {t: (t, 2 * t, 0) for t in range(FRAMES)}               # the decoder moves the box further every frame: an accelerating object
    got, div, calls, log = _both({0: _rect(5, 11, 4, 12)}, script)
    motions = {t: m for t, _, m, _ in log}
    assert motions[1] is None and motions[2] == (1.0, 2.0)            # centre(1) - centre(0): the decoder's move at frame 1
    assert motions[3] == (0.5 * 1.0 + 0.5 * 3.0, 0.5 * 2.0 + 0.5 * 6.0)          # frame 2 moved by the motion (1, 2) plus the script's (2, 4)
    assert any(m is not None and (m[0] % 1 == 0.5 or m[1] % 1 == 0.5) for m in motions.values())      # a half-integer shift went through scipy
    assert not div and len(calls) == len([e for e in log if e[1] in ("tracked", "gated")]) >= 3
    other, _, _, log2 = _both({0: _rect(5, 11, 4, 12)}, script, alpha=0.25)
    assert {t: m for t, _, m, _ in log2}[3] == (0.25 * 1.0 + 0.75 * 3.0, 0.25 * 2.0 + 0.75 * 6.0)


def test_the_gate_applies_only_past_the_last_annotated_frame():
    script = {1: (0, 0, 2), 2: (0, 0, 0), 4: (0, 0, 0), 5: (0, 0, 2)}
    notes = {0: _rect(10, 30, 10, 40), 3: _rect(12, 28, 12, 38)}
    got, div, calls, log = _both(notes, script, threshold=0.9)
    assert [(t, what) for t, what, _, _ in log] == [(1, "tracked"), (2, "tracked"), (3, "annotated"), (4, "gated"), (5, "gate")]
    assert T.iou(got[0], got[1]) < 0.9                                # frame 1 would not have passed the gate
    assert got[4].any() and not got[5:].any() and np.array_equal(got[3], notes[3]) and not div
    # without a threshold the same series runs to its end
    got, _, _, log = _both(notes, script, threshold=None)
    assert log[-1][0] == FRAMES - 1 and got[FRAMES - 1].any()


def test_stop_upper_ends_in_front_of_the_last_annotated_frame():
    notes = {0: _rect(10, 30, 10, 40), 3: _rect(12, 28, 12, 38)}
    got, div, calls, log = _both(notes, {}, stop_upper=True, threshold=0.5)
    assert [t for t, _ in calls] == [1, 2] and log[-1][:2] == (3, "stop_upper")
    assert np.array_equal(got[3], notes[3]) and not got[4:].any() and not div
    # a single annotated frame: t never equals it again, the flag does nothing (as in the reference)
    got, _, calls, _ = _both({2: notes[0]}, {}, stop_upper=True, threshold=0.5)
    assert [t for t, _ in calls] == list(range(3, FRAMES)) and not got[:2].any()


def test_a_division_ends_the_walk():
    notes = {1: _rect(10, 30, 10, 40), 3: _rect(12, 28, 12, 38), 5: _rect(12, 28, 12, 38)}
    got, div, calls, log = _both(notes, {}, threshold=0.5, states={3: "division", 1: "track"})
    assert div and [t for t, _ in calls] == [2] and log[-1][:2] == (3, "division")
    assert np.array_equal(got[3], notes[3]) and not got[4].any() and np.array_equal(got[5], notes[5]) and not got[0].any()
    from micro_sam_amd import tracking
    with pytest.raises(ValueError, match="division"):
        tracking.track_mask_in_timeseries(_series(notes), T.StubPredictor(SHAPE, {}), T.stub_embeddings(FRAMES, SHAPE), [1, 3, 5], False, 0.5,
                                          "box", frame_states={3: "mitosis"})
    with pytest.raises(ValueError, match="ascending"):
        tracking.track_mask_in_timeseries(_series(notes), T.StubPredictor(SHAPE, {}), T.stub_embeddings(FRAMES, SHAPE), [3, 1], False, 0.5, "box")


def test_an_empty_mask_to_prompt_from_stops_the_object():
    # the decoder answers frame 2 with nothing: the empty mask is written (no gate in front of an annotation), frame 3 has no prompt
    notes = {0: _rect(10, 30, 10, 40), 6: _rect(12, 28, 12, 38)}
    got, div, calls, log = _both(notes, {2: None}, threshold=0.5)
    assert [t for t, _ in calls] == [1, 2] and log[-1][:2] == (3, "empty")
    assert got[1].any() and not got[2:6].any() and np.array_equal(got[6], notes[6]) and not div
    # an object that runs out of the image: the moved mask is empty before the decoder is asked
    fast = {t: (0, 18, 0) for t in range(FRAMES)}
    got, div, calls, log = _both({0: _rect(10, 20, 2, 12)}, fast)
    assert log[-1][1] == "shifted out" and log[-1][0] < FRAMES - 1 and not got[log[-1][0]:].any()
    # an empty annotation: nothing happens
    got, div, calls, log = _both({1: np.zeros(SHAPE, np.uint8)}, {})
    assert not calls and not got.any() and log == [(2, "empty", None, None)]


def test_the_end_of_the_series():
    got, div, calls, log = _both({5: _rect(10, 30, 10, 40)}, {})
    assert [t for t, _ in calls] == [6, 7] and got[7].any() and not got[:5].any()
    got, div, calls, log = _both({FRAMES - 1: _rect(10, 30, 10, 40)}, {})
    assert not calls and log == [] and got[FRAMES - 1].any() and not div


def test_the_mask_projection_prompts_with_logits_of_the_moved_mask():
    """The other prompt kind through segment_from_mask: box and mask ("mask" = both), on the walk's frames."""
    from micro_sam_amd import tracking
    script = {t: (1, 2, 0) for t in range(FRAMES)}
    notes = {0: _rect(5, 11, 4, 12)}
    want, _ = T.walk(_series(notes), np.array([0]), False, 0.3, script)
    got, _ = tracking.track_mask_in_timeseries(_series(notes), T.StubPredictor(SHAPE, script), T.stub_embeddings(FRAMES, SHAPE), np.array([0]),
                                               False, 0.3, "mask")
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------ all objects at once, host route

def _field():
    seeds = np.stack([_rect(5, 15, 5, 20), _rect(20, 34, 30, 50), _rect(8, 18, 10, 24), _rect(22, 36, 28, 48), _rect(2, 8, 40, 50),
                      _rect(24, 30, 4, 14)])
    seeds[4][3, 45] = 2                                                # a value that is not the object
    frames = np.array([0, 1, 3, 4, 2, 0])
    ids = np.array([7, 3, 7, 3, 12, 5])
    states = ["track", "track", "track", "division", "track", "track"]
    return seeds, frames, ids, states


def _compose(seeds, frames, ids, states, stop, threshold, script, alpha=0.5):
    uniq = np.unique(ids)
    labels = np.zeros((FRAMES,) + SHAPE, np.int32)
    division = np.zeros(len(uniq), bool)
    centers = np.full((len(uniq), FRAMES, 2), np.nan)
    ranges = np.zeros((len(uniq), 2), np.int64)
    for n, i in enumerate(uniq):
        mine = [m for m in np.argsort(frames) if ids[m] == i]
        seg = _series({int(frames[m]): seeds[m] == 1 for m in mine})
        seg, division[n] = T.walk(seg, frames[mine], stop[n], threshold, script, alpha=alpha, states={int(frames[m]): states[m] for m in mine})
        labels[seg == 1] = i
        held = [t for t in range(FRAMES) if seg[t].any()]
        for t in held:
            centers[n, t] = T.center(seg[t])
        ranges[n] = (held[0], held[-1])
    return labels, uniq, ranges, division, centers


@pytest.mark.parametrize("stop", [False, [False, False, True, False]], ids=["run-on", "stop-upper-of-7"])
def test_objects_on_the_host_route_are_n_walks_composed(stop):
    from micro_sam_amd import tracking
    seeds, frames, ids, states = _field()
    script = {t: (1, -1, 0) for t in range(FRAMES)}
    script[6] = (0, 0, 2)
    per_object = np.broadcast_to(np.asarray(stop), (4,))
    want = _compose(seeds, frames, ids, states, per_object, 0.6, script)
    predictor = T.StubPredictor(SHAPE, script)
    emb = T.stub_embeddings(FRAMES, SHAPE)
    assert not tracking._can_propagate_on_device(predictor, emb, False)
    got = tracking.track_objects_in_timeseries(predictor, emb, seeds, frames, ids, 0.6, "box", stop_upper=stop, seed_states=states)
    assert isinstance(got, tracking.TrackingResult) and got.labels.dtype == np.int32 and got.ids.dtype == np.int64
    assert got.ranges.dtype == np.int64 and got.has_division.dtype == bool and got.centers.dtype == np.float64
    assert np.array_equal(got.labels, want[0]) and np.array_equal(got.ids, want[1]) and np.array_equal(got.ranges, want[2])
    assert np.array_equal(got.has_division, want[3]) and np.array_equal(got.centers, want[4], equal_nan=True)
    assert got.has_division.tolist() == [True, False, False, False] and got.ids.tolist() == [3, 5, 7, 12]
    assert np.isnan(got.centers[3, :2]).all() and not np.isnan(got.centers[3, 2]).any()
    assert (got.labels[2][seeds[4] == 1] == 12).all() and got.labels[2][3, 45] != 12
    if stop is not False:
        assert got.ranges[2].tolist() == [0, 3] and not (got.labels[4:] == 7).any()


def test_argument_errors_of_track_objects():
    from micro_sam_amd import tracking
    seeds, frames, ids, states = _field()
    predictor, emb = T.StubPredictor(SHAPE, {}), T.stub_embeddings(FRAMES, SHAPE)

    def call(**kw):
        a = dict(seeds=seeds, seed_frames=frames, seed_ids=ids, iou_threshold=0.5, projection="box", seed_states=states)
        a.update(kw)
        return tracking.track_objects_in_timeseries(predictor, emb, **a)
    with pytest.raises(ValueError, match="twice"):
        call(seed_ids=np.array([7, 3, 7, 3, 12, 7]))                  # (7, frame 0) two times
    with pytest.raises(ValueError, match="positive"):
        call(seed_ids=np.array([7, 3, 7, 3, 0, 5]))
    with pytest.raises(ValueError, match="positive"):
        call(seed_ids=np.array([7, 3, 7, 3, 2 ** 31, 5]))
    with pytest.raises(ValueError, match="seed_frames"):
        call(seed_frames=np.array([0, 1, 3, 4, FRAMES, 0]))
    with pytest.raises(ValueError, match="seed_frames"):
        call(seed_frames=frames[:5])
    with pytest.raises(ValueError, match="division"):
        call(seed_states=["track"] * 5 + ["split"])
    with pytest.raises(ValueError, match="seed_states"):
        call(seed_states=["track"] * 5)
    with pytest.raises(ValueError, match="stop_upper"):
        call(stop_upper=[True, False])
    with pytest.raises(ValueError, match="seeds"):
        call(seeds=seeds[0])
    with pytest.raises(ValueError, match="projection"):
        call(projection="lines")
    empty = tracking.track_objects_in_timeseries(predictor, emb, seeds[:0], [], [], 0.5, "box")
    assert empty.labels.shape == (FRAMES,) + SHAPE and not empty.labels.any() and empty.ids.shape == (0,) and empty.centers.shape == (0, FRAMES, 2)
