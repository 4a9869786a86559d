"""micro_sam_amd.evaluation.inference on the device, on one 256 x 256 seeded image with about a dozen objects and the synthetic vit_b
model: box / point inference against ``batched_inference`` fed prompts built from the host restatement (tests/labelprops_ref.py) - the
prompt arrays equal, so the label images equal bit for bit -, the prompt cache, iterative prompting from a box and from a point (prompt
shapes per round, multimasking and logits rules, skipping, run-to-run identity under a seed), and scoring with ``run_evaluation``."""
import os
import pickle

import numpy as np
import pytest
import torch

import labelprops_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def predictor(vit_b_sd):
    from micro_sam_amd import util
    return util.get_sam_model("vit_b", device="cuda:0", state_dict=vit_b_sd)


@pytest.fixture(scope="module")
def data():
    gt = R.voronoi(256, 256, 15, 4)
    gt = np.unique(gt, return_inverse=True)[1].reshape(gt.shape).astype(np.int32)          # consecutive ids
    rng = np.random.default_rng(0)
    image = np.clip((gt * 53 % 160) + 40 + rng.normal(0, 6, gt.shape), 0, 255).astype(np.uint8)
    want = R.label_props(gt)
    assert 10 <= len(want["ids"]) <= 14 and (gt == 0).any()
    return image, gt, want


class Spy:
    """Records the keyword arguments of ``batched_inference`` as the evaluation module calls it."""

    def __init__(self, monkeypatch):
        from micro_sam_amd.evaluation import inference as I
        self.calls, real = [], I.batched_inference

        def spy(*args, **kw):
            self.calls.append(kw)
            return real(*args, **kw)
        monkeypatch.setattr(I, "batched_inference", spy)


def test_box_and_point_inference_equal_batched_inference_on_host_prompts(predictor, data):
    from micro_sam_amd.evaluation import inference as I
    from micro_sam_amd.inference import batched_inference
    image, gt, want = data
    boxes = want["bbox"][:, [1, 0, 3, 2]].astype(np.float32)
    labels, (p, pl, b) = I._run_inference_with_prompts_for_image(predictor, image, gt, use_points=False, use_boxes=True, n_positives=0,
                                                                 n_negatives=0, dilation=5, batch_size=8, cached_prompts=None, embedding_path=None)
    assert p is None and pl is None and b.dtype == np.float32 and np.array_equal(b, boxes)
    expected = batched_inference(predictor, image, 8, boxes=boxes, return_instance_segmentation=True)
    assert labels.dtype == expected.dtype and np.array_equal(labels, expected) and labels.max() > 0

    points = want["center"][:, None, ::-1].astype(np.float32)
    point_labels = np.ones((len(points), 1), np.float32)
    labels, (p, pl, b) = I._run_inference_with_prompts_for_image(predictor, image, gt.astype(np.uint32), use_points=True, use_boxes=False,
                                                                 n_positives=1, n_negatives=0, dilation=5, batch_size=8, cached_prompts=None,
                                                                 embedding_path=None)
    assert b is None and p.dtype == pl.dtype == np.float32 and np.array_equal(p, points) and np.array_equal(pl, point_labels)
    expected = batched_inference(predictor, image, 8, points=points, point_labels=point_labels, multimasking=True, return_instance_segmentation=True)
    assert np.array_equal(labels, expected)
    # cached prompts are used as given
    again, prompts = I._run_inference_with_prompts_for_image(predictor, image, None, use_points=True, use_boxes=False, n_positives=1, n_negatives=0,
                                                             dilation=5, batch_size=8, cached_prompts=(points, point_labels, None), embedding_path=None)
    assert np.array_equal(again, expected) and np.array_equal(prompts[0], points)


def test_prompt_cache_round_trip(tmp_path, data):
    from micro_sam_amd.evaluation import inference as I
    image, gt, want = data
    np.save(tmp_path / "cells.npy", gt)
    settings = [{"use_points": False, "use_boxes": True, "n_positives": 0, "n_negatives": 0},
                {"use_points": True, "use_boxes": False, "n_positives": 1, "n_negatives": 0},
                {"use_points": True, "use_boxes": False, "n_positives": 2, "n_negatives": 3, "dilation": 2}]
    np.random.seed(0)
    I.precompute_all_prompts([str(tmp_path / "cells.npy")], str(tmp_path / "prompts"), settings)
    assert sorted(os.listdir(tmp_path / "prompts")) == ["boxes.pkl", "points-p1-n0.pkl", "points-p2-n3.pkl"]
    stored_boxes = pickle.load(open(tmp_path / "prompts" / "boxes.pkl", "rb"))
    stored_points = pickle.load(open(tmp_path / "prompts" / "points-p1-n0.pkl", "rb"))
    assert list(stored_boxes) == list(stored_points) == ["cells.npy"]
    assert np.array_equal(stored_boxes["cells.npy"], want["bbox"][:, [1, 0, 3, 2]].astype(np.float32))
    assert np.array_equal(stored_points["cells.npy"][0], want["center"][:, None, ::-1].astype(np.float32))

    cache = I._get_prompt_caching(str(tmp_path / "prompts"), True, True, 1, 0)
    assert cache == (str(tmp_path / "prompts" / "points-p1-n0.pkl"), False, str(tmp_path / "prompts" / "points-p1-n0.pkl"),
                     str(tmp_path / "prompts" / "boxes.pkl"), False, str(tmp_path / "prompts" / "boxes.pkl"))
    (p, pl, b), cached_p, cached_b = I._load_prompts(cache[0], cache[1], cache[3], cache[4], "cells.npy")
    assert np.array_equal(p, stored_points["cells.npy"][0]) and np.array_equal(pl, stored_points["cells.npy"][1])
    assert np.array_equal(b, stored_boxes["cells.npy"]) and isinstance(cached_p, dict) and isinstance(cached_b, dict)
    assert I._load_prompts(None, False, None, False, "cells.npy") == (None, None, None)
    assert I._get_prompt_caching(None, True, True, 1, 0) == (None, False, None, None, False, None)

    # the sampled setting goes through PointAndBoxPromptGenerator: the centre first, positives inside, negatives outside the object
    pts, lab = pickle.load(open(tmp_path / "prompts" / "points-p2-n3.pkl", "rb"))["cells.npy"]
    n = len(want["ids"])
    assert pts.shape == (n, 5, 2) and lab.shape == (n, 5) and np.array_equal(pts[:, 0], want["center"][:, ::-1].astype(np.float32))
    xy = pts.astype(int)
    hit = gt[xy[..., 1], xy[..., 0]] == want["ids"][:, None]
    assert np.array_equal(hit, lab == 1) and (lab[:, :2] == 1).all()


def test_run_inference_with_prompts_writes_and_skips(tmp_path, predictor, data, monkeypatch):
    from micro_sam_amd.evaluation import inference as I
    from micro_sam_amd.evaluation.evaluation import run_evaluation
    from micro_sam_amd.inference import batched_inference
    image, gt, want = data
    spy = Spy(monkeypatch)
    args = dict(embedding_dir=str(tmp_path / "emb"), prediction_dir=str(tmp_path / "pred"), use_points=False, use_boxes=True, n_positives=0,
                n_negatives=0, prompt_save_dir=str(tmp_path / "prompts"), batch_size=8)
    os.makedirs(tmp_path / "emb")
    I.run_inference_with_prompts(predictor, [image], [gt], **args)
    assert len(spy.calls) == 1 and os.path.isdir(tmp_path / "emb" / "image_0.zarr")
    stored = pickle.load(open(tmp_path / "prompts" / "boxes.pkl", "rb"))
    boxes = want["bbox"][:, [1, 0, 3, 2]].astype(np.float32)
    assert np.array_equal(stored["image_0"], boxes)
    pred = np.load(tmp_path / "pred" / "image_0.npy")
    assert np.array_equal(pred, batched_inference(predictor, image, 8, boxes=boxes, return_instance_segmentation=True))
    I.run_inference_with_prompts(predictor, [image], [gt], **args)
    assert len(spy.calls) == 1                                                            # the image is done: skipped
    with pytest.raises(ValueError, match="at least one"):
        I.run_inference_with_prompts(predictor, [image], [gt], **dict(args, use_boxes=False))
    with pytest.raises(ValueError, match="same number"):
        I.run_inference_with_prompts(predictor, [image], [gt, gt], **args)
    # scoring the written prediction with the existing evaluation
    res = run_evaluation([gt], [str(tmp_path / "pred" / "image_0.npy")], save_path=str(tmp_path / "results" / "boxes.csv"), verbose=False)
    assert list(res.columns) == ["mSA", "SA50", "SA75", "Precision", "Recall", "F1 Score"] and len(res) == 1
    assert 0.0 <= float(res["mSA"][0]) <= 1.0 and os.path.exists(tmp_path / "results" / "boxes.csv")


def _folder(root):
    return {os.path.relpath(os.path.join(d, f), root): np.load(os.path.join(d, f)) for d, _, files in os.walk(root) for f in sorted(files)}


def test_iterative_prompting_from_a_box(tmp_path, predictor, data, monkeypatch):
    from micro_sam_amd.evaluation import inference as I
    from micro_sam_amd.evaluation.evaluation import run_evaluation_for_iterative_prompting
    image, gt, want = data
    n = len(want["ids"])
    spy = Spy(monkeypatch)
    torch.manual_seed(0)
    I.run_inference_with_iterative_prompting(predictor, [image], [gt], None, str(tmp_path / "it"), start_with_box_prompt=True, batch_size=8,
                                             n_iterations=3)
    assert sorted(os.listdir(tmp_path / "it")) == ["iteration00", "iteration01", "iteration02"]
    assert all(os.listdir(tmp_path / "it" / f"iteration{k:02}") == ["image_0.npy"] for k in range(3))
    assert len(spy.calls) == 3
    boxes = want["bbox"][:, [1, 0, 3, 2]].astype(np.float32)
    for k, kw in enumerate(spy.calls):
        assert np.array_equal(kw["boxes"], boxes) and kw["multimasking"] is False and kw["logits_masks"] is None
        if k == 0:
            assert kw["points"] is None and kw["point_labels"] is None
        else:
            assert kw["points"].shape == (n, 2 * k, 2) and kw["point_labels"].shape == (n, 2 * k)
            assert np.array_equal(kw["point_labels"], np.tile([1, 0], (n, k)))
            x, y = kw["points"][..., 0].astype(int), kw["points"][..., 1].astype(int)
            assert (x >= 0).all() and (x < 256).all() and (y >= 0).all() and (y < 256).all()
            assert (gt[y[:, 0::2], x[:, 0::2]] == want["ids"][:, None]).all()             # positive points lie in their object
            assert (gt[y[:, 1::2], x[:, 1::2]] != want["ids"][:, None]).all()             # negative points outside it
    for k in range(3):
        seg = np.load(tmp_path / "it" / f"iteration{k:02}" / "image_0.npy")
        assert seg.shape == gt.shape and seg.dtype == np.uint32 and seg.max() > 0
    I.run_inference_with_iterative_prompting(predictor, [image], [gt], None, str(tmp_path / "it"), start_with_box_prompt=True, batch_size=8,
                                             n_iterations=3)
    assert len(spy.calls) == 3                                                            # finished images are skipped
    res = run_evaluation_for_iterative_prompting([gt], str(tmp_path / "it"), str(tmp_path / "exp"), start_with_box_prompt=True)
    assert len(res) == 3 and list(res.columns) == ["mSA", "SA50", "SA75", "Precision", "Recall", "F1 Score"]
    assert os.path.exists(tmp_path / "exp" / "results" / "iterative_prompting_without_mask" / "iterative_prompts_start_box.csv")


def test_iterative_prompting_from_a_point_with_masks_is_repeatable(tmp_path, predictor, data, monkeypatch):
    from micro_sam_amd.evaluation import inference as I
    image, gt, want = data
    n = len(want["ids"])
    spy = Spy(monkeypatch)
    for run in ("a", "b"):
        torch.manual_seed(5)
        I.run_inference_with_iterative_prompting(predictor, [image], [gt], None, str(tmp_path / run), start_with_box_prompt=False, batch_size=8,
                                                 n_iterations=3, use_masks=True)
    assert len(spy.calls) == 6
    centre = want["center"][:, None, ::-1].astype(np.float32)
    for k, kw in enumerate(spy.calls[:3]):
        assert kw["boxes"] is None and kw["multimasking"] is (k == 0)                     # multimasking for the single point only
        assert kw["points"].shape == (n, 1 + 2 * k, 2) and np.array_equal(kw["points"][:, :1], centre)
        assert kw["point_labels"].shape == (n, 1 + 2 * k)
        if k == 0:
            assert kw["logits_masks"] is None
        else:
            assert kw["logits_masks"].is_cuda and tuple(kw["logits_masks"].shape) == (n, 1, 256, 256)
    a, b = _folder(tmp_path / "a"), _folder(tmp_path / "b")
    assert sorted(a) == sorted(b) == [os.path.join(f"iteration{k:02}", "image_0.npy") for k in range(3)]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for x, y in zip(spy.calls[:3], spy.calls[3:]):
        assert np.array_equal(x["points"], y["points"])
