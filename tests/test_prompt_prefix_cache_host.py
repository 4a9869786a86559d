"""The mask generator's cache of uploaded point grids and their prompt-prefix blocks (micro_sam_amd/_prompt_prefix.py,
AutomaticMaskGenerator._process_batch), without a device: keying, eviction at 8 entries (oldest first), the drop when the decoder's
prepared constants are another object, and the modes that keep no block.  The decode is a stub."""
import numpy as np
import pytest
import torch

from micro_sam_amd._prompt_prefix import MAX_ENTRIES, PromptPrefixCache


def _grid(n, scale=1.0):
    return (np.stack(np.meshgrid(np.arange(n), np.arange(n)), -1).reshape(-1, 2) + 0.5) * scale


def test_cache_keying_and_eviction():
    assert MAX_ENTRIES == 8
    cache, made, owner = PromptPrefixCache(), [], object()

    def make(pts):
        made.append(pts.copy())
        return ("entry", len(made))

    a = cache.get(("k", 0), _grid(4), owner, make)
    assert cache.get(("k", 0), _grid(4), owner, make) is a and len(made) == 1          # found again
    b = cache.get(("k", 0), _grid(4, 2.0), owner, make)                                 # same key, other points: made anew, replaces
    assert b is not a and len(made) == 2 and len(cache) == 1
    assert cache.get(("k", 0), _grid(4), owner, make) is not a and len(made) == 3
    for i in range(1, MAX_ENTRIES):
        cache.get(("k", i), _grid(4, 1.0 + i), owner, make)
    assert len(cache) == MAX_ENTRIES and len(made) == 3 + MAX_ENTRIES - 1
    n = len(made)
    cache.get(("k", 1), _grid(4, 2.0), owner, make)
    assert len(made) == n                                                               # all 8 still there
    cache.get(("k", 99), _grid(5), owner, make)                                         # the ninth drops the oldest: ("k", 0)
    assert len(cache) == MAX_ENTRIES and len(made) == n + 1
    cache.get(("k", 1), _grid(4, 2.0), owner, make)
    assert len(made) == n + 1                                                           # the second oldest stayed
    cache.get(("k", 0), _grid(4), owner, make)
    assert len(made) == n + 2 and len(cache) == MAX_ENTRIES                             # ("k", 0) was gone; now ("k", 1) is


def test_cache_is_dropped_when_the_owner_is_another_object():
    cache, made = PromptPrefixCache(), []
    make = lambda pts: made.append(1) or object()                                       # noqa: E731
    own1, own2 = ["params", "keep", "consts"], ["params", "keep", "consts"]             # equal, but two objects
    assert own1 == own2 and own1 is not own2
    for i in range(3):
        cache.get(i, _grid(3), own1, make)
    assert len(cache) == 3 and len(made) == 3
    cache.get(0, _grid(3), own2, make)
    assert len(cache) == 1 and len(made) == 4                                           # identity, not equality, decides
    cache.get(0, _grid(3), own2, make)
    assert len(made) == 4


class _StubTransform:
    def apply_coords(self, pts, im_size):
        return np.asarray(pts, dtype=np.float64) * 2.0


class _StubModel:
    def __init__(self):
        self.reference_formulation = False
        self.prepared = ("params", [], "consts")
        self.made = []

    def _prepare_decoder(self):
        return self.prepared

    def make_prompt_prefix(self, pts, lbl, boxes=None):
        assert pts.shape[1:] == (1, 2) and lbl.shape[1:] == (1,) and boxes is None
        self.made.append(pts.clone())
        return ("prefix", len(self.made), self.prepared)


class _StubPredictor:
    def __init__(self):
        self.model, self.transform, self.device = _StubModel(), _StubTransform(), torch.device("cpu")
        self.calls = []

    def predict_masks_device(self, point_coords, point_labels, boxes=None, multimask_output=True, stability_score_offset=1.0,
                             prompt_prefix=None):
        self.calls.append((point_coords, point_labels, prompt_prefix))
        return "iou", "post"


@pytest.fixture
def amg(monkeypatch):
    from micro_sam_amd import _lib
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator
    gen = AutomaticMaskGenerator(_StubPredictor(), points_per_side=4)
    monkeypatch.setattr(gen, "_to_mask_data_device", lambda iou, post, crop_box, original_size, points=None: (iou, post))
    knob = {"prompt_prefix": 1}
    monkeypatch.setattr(_lib, "tune_get", lambda key: knob[key])
    return gen, knob


def test_process_batch_keeps_one_block_per_grid_and_size(amg):
    gen, knob = amg
    pred, model = gen._predictor, gen._predictor.model
    pts = gen.point_grids[0] * np.array([[1024, 1024]])
    for _ in range(3):                                                                  # three tiles of one size: one block
        gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert len(model.made) == 1 and len(gen._prompt_cache) == 1
    assert all(c[0] is None and c[1] is None and c[2] == ("prefix", 1, model.prepared) for c in pred.calls)
    assert torch.equal(model.made[0][:, 0], torch.as_tensor(pts * 2.0, dtype=torch.float))
    gen._process_batch(pts[:8], (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))        # another chunk of the grid
    half = gen.point_grids[0] * np.array([[512, 768]])
    gen._process_batch(half, (768, 512), [0, 0, 512, 768], (768, 512))                 # another crop size
    assert len(model.made) == 3 and len(gen._prompt_cache) == 3
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert len(model.made) == 3 and pred.calls[-1][2] == ("prefix", 1, model.prepared)
    # rebuilt constants (new weights, set_split_token_mlp, a PEFT merge): every block goes
    model.prepared = ("params", [], "consts")
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert len(model.made) == 4 and len(gen._prompt_cache) == 1 and pred.calls[-1][2][2] is model.prepared
    # at most 8 entries
    for k in range(12):
        gen._process_batch(pts[: 3 + k], (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert len(gen._prompt_cache) == 8


def test_process_batch_without_blocks(amg):
    """The knob at 0 and the precision modes off the kernel path decode from the cached point tensors, with no block."""
    gen, knob = amg
    pred, model = gen._predictor, gen._predictor.model
    pts = gen.point_grids[0] * np.array([[1024, 1024]])
    knob["prompt_prefix"] = 0
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert not model.made and pred.calls[-1][2] is None and pred.calls[-1][0].shape == (16, 1, 2)
    assert pred.calls[-1][0].data_ptr() == pred.calls[-2][0].data_ptr()                 # the uploaded points are kept all the same
    knob["prompt_prefix"] = 1
    model.reference_formulation = True
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert not model.made and pred.calls[-1][2] is None
    model.reference_formulation = False
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    assert len(model.made) == 1 and pred.calls[-1][2] is not None


def test_lane_clone_has_a_cache_of_its_own(amg):
    gen, _ = amg
    pts = gen.point_grids[0] * np.array([[1024, 1024]])
    gen._process_batch(pts, (1024, 1024), [0, 0, 1024, 1024], (1024, 1024))
    clone = gen._lane_clone(_StubPredictor())
    assert clone._prompt_cache is not gen._prompt_cache and len(clone._prompt_cache) == 0
