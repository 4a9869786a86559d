"""csrc/labelprops.hip on the device: ``ops.edt_squared`` and ``ops.label_props`` integer for integer against tests/labelprops_ref.py on the
label images of tests/test_host_labelprops.py plus one 512 x 512 Voronoi image, run-to-run identity, the boundary of the two wrappers,
and ``util.get_centers_and_bounding_boxes`` / ``util.segmentation_to_one_hot`` (the latter against the reference's formula, written out
below)."""
import functools

import numpy as np
import pytest
import torch

import labelprops_ref as R

pytestmark = pytest.mark.gpu
CASES, MASKS = R.cases(), R.edt_masks()


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _voronoi512():
    seg = R.voronoi(512, 512, 350, 5)
    return seg, R.label_props(seg)


def _same(props, want, centers=True):
    assert props.ids.dtype == torch.int32 and props.area.dtype == torch.int32 and props.bbox.dtype == torch.int32
    assert props.coord_sum.dtype == torch.int64
    n = len(want["ids"])
    assert np.array_equal(props.ids.cpu().numpy(), want["ids"])
    assert np.array_equal(props.area.cpu().numpy(), want["area"])
    assert tuple(props.bbox.shape) == (n, 4) and np.array_equal(props.bbox.cpu().numpy(), want["bbox"])
    assert tuple(props.coord_sum.shape) == (n, 2) and np.array_equal(props.coord_sum.cpu().numpy(), want["coord_sum"])
    if centers:
        assert props.center.dtype == torch.int32 and tuple(props.center.shape) == (n, 2)
        assert np.array_equal(props.center.cpu().numpy(), want["center"])
    else:
        assert props.center is None


@pytest.mark.parametrize("name", sorted(MASKS))
def test_edt_squared_is_exact(name):
    from micro_sam_amd import ops
    mask = MASKS[name]
    want = R.edt_squared(mask)
    for m in (_dev(mask, np.uint8), _dev(mask, np.uint8).bool(), _dev(mask.astype(np.int32) * 77)):
        got = ops.edt_squared(m)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


def test_edt_squared_of_boundaries_512():
    from micro_sam_amd import ops
    seg, _ = _voronoi512()
    mask = (R.inner_boundaries(seg) == 0)[1:-1, 1:-1]
    assert np.array_equal(ops.edt_squared(_dev(mask, np.uint8)).cpu().numpy(), R.edt_squared(mask))


@pytest.mark.parametrize("name", sorted(CASES))
def test_label_props_equal_the_restatement(name):
    from micro_sam_amd import ops
    seg, ids = CASES[name]
    want = R.label_props(seg, ids)
    _same(ops.label_props(_dev(seg), None if ids is None else _dev(ids)), want)
    _same(ops.label_props(_dev(seg), None if ids is None else _dev(ids), centers=False), want, centers=False)


def test_label_props_voronoi_512_twice():
    from micro_sam_amd import ops
    seg, want = _voronoi512()
    assert 280 <= len(want["ids"]) <= 320 and (seg == 0).mean() > 0.1
    d = _dev(seg)
    first, second = ops.label_props(d), ops.label_props(d)
    _same(first, want)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_no_object_means_no_launch():
    from micro_sam_amd import ops
    from ops_boundary_table import recording
    with recording(real_gpu=True) as rec:
        props = ops.label_props(torch.zeros((5, 7), dtype=torch.int32, device="cuda"))
        empty = ops.label_props(torch.ones((5, 7), dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert not rec.calls
    for p in (props, empty):
        assert [tuple(t.shape) for t in p] == [(0,), (0,), (0, 4), (0, 2), (0, 2)]


def test_wrappers_refuse_what_the_kernels_cannot_read():
    from micro_sam_amd import ops
    from ops_boundary_table import recording
    lab = torch.ones((6, 8), dtype=torch.int32, device="cuda")
    ids = torch.ones(1, dtype=torch.int32, device="cuda")
    with recording(real_gpu=True) as rec:
        for bad in (lab.long(), lab[:, ::2], lab[None], lab.cpu(), lab.float()):
            with pytest.raises((ValueError, TypeError), match="labels"):
                ops.label_props(bad, ids)
        for bad in (ids.long(), torch.ones(4, dtype=torch.int32, device="cuda")[::2], ids[None], ids.cpu()):
            with pytest.raises((ValueError, TypeError), match="ids"):
                ops.label_props(lab, bad)
        for bad in (lab.long(), lab[:, ::2], lab[None], lab.cpu().to(torch.uint8), lab.float()):
            with pytest.raises((ValueError, TypeError), match="mask"):
                ops.edt_squared(bad)
    assert not rec.calls
    with pytest.raises(ValueError, match="msam_label_props"):                         # refused by the library: unsorted ids
        ops.label_props(lab, torch.tensor([3, 1], dtype=torch.int32, device="cuda"))


def test_get_centers_and_bounding_boxes_round_trip():
    from micro_sam_amd import util
    for name in ("c", "ring", "big_ids", "130x257"):
        seg, _ = CASES[name]
        want = R.label_props(seg)
        for given in (seg, seg.astype(np.uint32), seg.astype(np.int64), _dev(seg), torch.from_numpy(seg)):
            centers, boxes = util.get_centers_and_bounding_boxes(given)
            assert list(centers) == list(boxes) == want["ids"].tolist() and all(type(k) is int for k in centers)
            assert all(type(c) is tuple and len(c) == 2 and all(type(v) is int for v in c) for c in centers.values())
            assert all(type(b) is tuple and len(b) == 4 and all(type(v) is int for v in b) for b in boxes.values())
            assert [list(c) for c in centers.values()] == want["center"].tolist()
            assert [list(b) for b in boxes.values()] == want["bbox"].tolist()
        centroids, boxes_p = util.get_centers_and_bounding_boxes(seg, mode="p")
        assert boxes_p == boxes and all(type(v) is float for c in centroids.values() for v in c)
        assert np.array_equal(np.array(list(centroids.values())), want["centroid"])       # float64 bits: sum / area is exact
    seg, _ = CASES["c"]
    (cy, cx), = util.get_centers_and_bounding_boxes(seg)[0].values()
    (py, px), = util.get_centers_and_bounding_boxes(seg, mode="p")[0].values()
    assert seg[cy, cx] != 0 and seg[int(round(py)), int(round(px))] == 0                  # "v" inside, "p" outside
    assert util.get_centers_and_bounding_boxes(np.zeros((4, 4), np.int32)) == ({}, {})
    with pytest.raises(ValueError, match="2-d"):
        util.get_centers_and_bounding_boxes(np.zeros((2, 4, 4), np.int32))
    with pytest.raises(ValueError, match="2-d"):
        util.get_centers_and_bounding_boxes(torch.zeros(8, dtype=torch.int32))


def _one_hot_reference(segmentation, segmentation_ids=None):
    """micro_sam/util.py:1356-1395 with ``relabel_sequential`` written out."""
    masks = segmentation.copy()
    if segmentation_ids is None:
        n_ids = int(segmentation.max())
    else:
        if len(segmentation_ids) == 0 or 0 in segmentation_ids:
            raise RuntimeError("No foreground objects were found.")
        segmentation_ids = np.sort(segmentation_ids)
        masks[~np.isin(masks, segmentation_ids)] = 0
        present = np.unique(masks)
        present = present[present != 0]
        masks = np.where(masks != 0, np.searchsorted(present, masks) + 1, 0)           # relabel_sequential
        n_ids = len(segmentation_ids)
    masks = torch.from_numpy(masks.astype(np.int64))
    one_hot_shape = (n_ids + 1,) + masks.shape
    return torch.zeros(one_hot_shape).scatter_(0, masks.unsqueeze(0), 1)[1:].unsqueeze(1)


def test_segmentation_to_one_hot_equals_the_reference_formula():
    from micro_sam_amd import util
    seg = CASES["33x65"][0].astype(np.int64)
    present = np.unique(seg)[1:]
    for ids in (None, present[[1, 3, 4]], present[[4, 1, 3]], list(present[[4, 1]]) + [400], present):
        want = _one_hot_reference(seg, None if ids is None else np.asarray(ids))
        got = util.segmentation_to_one_hot(seg, ids)
        assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and torch.equal(got, want)
        on_dev = util.segmentation_to_one_hot(torch.from_numpy(seg).cuda(), ids)
        assert on_dev.is_cuda and on_dev.dtype == torch.float32 and torch.equal(on_dev.cpu(), want)
    assert util.segmentation_to_one_hot(seg).shape[0] == int(seg.max())
    for ids in ([], [0, 1], np.array([2, 0])):
        with pytest.raises(RuntimeError, match="No foreground objects were found."):
            util.segmentation_to_one_hot(seg, ids)
        with pytest.raises(RuntimeError, match="No foreground objects were found."):
            util.segmentation_to_one_hot(torch.from_numpy(seg).cuda(), ids)
