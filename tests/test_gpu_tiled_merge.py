"""Cross-tile mask NMS and label merge on the device (csrc/tilemerge.hip behind ops.tiled_mask_overlaps / ops.paint_tiled and
util.apply_nms on tile-local records whose masks are CUDA tensors): the kernel checks of tests/test_tiled_merge_host.py through the
tensor wrappers, and util.apply_nms bit for bit - ids included - against the oracle and against the host path on the same records as
numpy.  One timing record (host path against device path, no assertion on time) is printed and written as tiled_merge.json to the
directory MSAM_TIMING_DIR names (the test's temporary directory without it)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import tiled_merge_cases as T
from oracle import amg_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """Per seed: the records, checked to be a real cross-tile input, and their table with the words on the device."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = {}
    for seed in T.SEEDS:
        recs = T.tiled_records(seed)
        T.check_preconditions(recs, A)
        words, off, geom = T.table(recs)
        out[seed] = dict(recs=recs, words=torch.from_numpy(words.view(np.int32)).cuda(), off=off, geom=geom)
    return out


def _cuda(recs):
    return [dict(r, segmentation=torch.from_numpy(r["segmentation"]).cuda()) for r in recs]


def _numpy(recs):
    return [dict(r) for r in recs]


@pytest.mark.parametrize("seed", T.SEEDS)
def test_overlaps_of_all_candidate_pairs_are_the_numpy_counts(cases, seed):
    from micro_sam_amd import ops
    c = cases[seed]
    pairs = T.candidate_pairs(c["recs"])
    want = np.array([T.overlap(c["recs"][i], c["recs"][j]) for i, j in pairs.tolist()], np.int32)
    got = ops.tiled_mask_overlaps(c["words"], c["off"], c["geom"], pairs)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.tiled_mask_overlaps(c["words"], c["off"], c["geom"], np.ascontiguousarray(pairs[:, ::-1])).cpu().numpy(), want)
    assert ops.tiled_mask_overlaps(c["words"], c["off"], c["geom"], np.zeros((0, 2), np.int32)).shape == (0,)


def test_overlap_hand_cases_of_ragged_tiles():
    """Tiles of different shapes in one table: the coinciding squares (81), a 1 x 1 window, an empty window, the last row of a 150-high
    tile against a tile 17 rows lower."""
    from micro_sam_amd import ops
    a = np.zeros((40, 40), bool); a[5:15, 5:15] = True
    b = np.zeros((40, 40), bool); b[25:35, 15:25] = True
    c = np.zeros((70, 50), bool); c[10:20, 10:20] = True
    d = np.zeros((33, 90), bool); d[3:9, 4:30] = True
    e = np.zeros((70, 50), bool); e[12:30, 19:40] = True
    g = np.zeros((150, 200), bool); g[80:150, 30:90] = True
    h = np.zeros((150, 200), bool); h[40:149, 20:70] = True
    recs = [T.record(a, (20, 100)), T.record(b, (0, 90)), T.record(c, (0, 0)), T.record(d, (15, 14)), T.record(e, (0, 0)),
            T.record(g, (0, 0)), T.record(h, (17, 25))]
    pairs = np.array([(0, 1), (2, 3), (2, 4), (5, 6), (5, 5)], np.int32)
    want = [T.overlap(recs[i], recs[j]) for i, j in pairs.tolist()]
    assert want[:3] == [81, 1, 0] and want[3] > 1000
    words, off, geom = T.table(recs)
    got = ops.tiled_mask_overlaps(torch.from_numpy(words.view(np.int32)).cuda(), off, geom, pairs)
    assert got.cpu().tolist() == want


@pytest.mark.parametrize("seed", T.SEEDS)
def test_paint_is_the_exclusive_merge_of_the_host(cases, seed):
    from micro_sam_amd import ops, util
    c = cases[seed]
    recs = [dict(r, area=int(r["segmentation"].sum())) for r in c["recs"]]
    order = np.array(sorted(range(len(recs)), key=lambda i: recs[i]["area"], reverse=True), np.int32)
    shape = A.infer_tiled_shape(recs)
    got = ops.paint_tiled(c["words"], c["off"], c["geom"], order, *shape).cpu().numpy()
    assert np.array_equal(got, T.paint(recs, order.tolist(), shape))
    host = util.mask_data_to_segmentation(_numpy(recs), shape=shape, label_masks=False)
    assert T.same_partition(got, host.astype(np.int64)) and len(np.unique(got)) > 30
    back = ops.paint_tiled(c["words"], c["off"], c["geom"], np.ascontiguousarray(order[::-1]), *shape).cpu().numpy()
    assert np.array_equal(back, T.paint(recs, order[::-1].tolist(), shape)) and not T.same_partition(got, back)     # first painter wins
    assert not ops.paint_tiled(c["words"], c["off"], c["geom"], np.zeros(0, np.int32), *shape).any()


def test_wrappers_refuse_tables_the_kernels_could_not_trust(cases):
    from micro_sam_amd import ops
    c = cases[0]
    pairs, order = np.zeros((1, 2), np.int32), np.zeros(1, np.int32)

    def geom_with(col, value):
        g = c["geom"].copy()
        g[3, col] = value
        return g
    for col, value in ((2, -1), (4, 250), (3, -2), (5, 170), (0, 0)):                 # bx < 0, bx + bw > tw, by < 0, by + bh > 32 wpc, wpc < 1
        with pytest.raises(ValueError, match="geom"):
            ops.tiled_mask_overlaps(c["words"], c["off"], geom_with(col, value), pairs)
    off = c["off"].copy()
    off[-1] += 1
    with pytest.raises(ValueError, match="word_offset"):
        ops.tiled_mask_overlaps(c["words"], off, c["geom"], pairs)
    with pytest.raises(ValueError, match="pairs"):
        ops.tiled_mask_overlaps(c["words"], c["off"], c["geom"], np.array([[0, 60]], np.int32))
    with pytest.raises(ValueError, match="order"):
        ops.paint_tiled(c["words"], c["off"], c["geom"], np.array([60], np.int32), 260, 420)
    with pytest.raises(ValueError, match="geom"):
        ops.paint_tiled(c["words"], c["off"], c["geom"], order, 100, 420)             # windows leave the image
    with pytest.raises(ValueError, match="words"):
        ops.tiled_mask_overlaps(c["words"].cpu(), c["off"], c["geom"], pairs)


@pytest.mark.parametrize("iomin", [False, True])
@pytest.mark.parametrize("seed", T.SEEDS)
def test_apply_nms_on_cuda_records_is_the_oracle_and_the_host_path(cases, seed, iomin):
    from micro_sam_amd import util
    recs = cases[seed]["recs"]
    for kw in T.KWARGS:
        got = util.apply_nms(_cuda(recs), intersection_over_min=iomin, **kw)
        ref = A.apply_nms(_numpy(recs), intersection_over_min=iomin, **kw)
        assert got.shape == ref.shape == (260, 420) and got.dtype == np.uint32
        assert np.array_equal(got, ref) and got.max() > 0
        assert np.array_equal(got, util.apply_nms(_numpy(recs), intersection_over_min=iomin, **kw))


def test_apply_nms_box_nms_explicit_shape_and_nothing_left(cases):
    from micro_sam_amd import util
    recs = cases[1]["recs"]
    got = util.apply_nms(_cuda(recs), min_size=10, perform_box_nms=True, nms_thresh=0.5)
    assert np.array_equal(got, util.apply_nms(_numpy(recs), min_size=10, perform_box_nms=True, nms_thresh=0.5)) and got.max() > 0
    assert np.array_equal(got, A.apply_nms(_numpy(recs), min_size=10, perform_box_nms=True, nms_thresh=0.5))
    got = util.apply_nms(_cuda(recs), min_size=0, shape=(310, 430))
    assert got.shape == (310, 430) and np.array_equal(got, A.apply_nms(_numpy(recs), min_size=0, shape=(310, 430)))
    assert np.array_equal(got, util.apply_nms(_numpy(recs), min_size=0, shape=(310, 430)))
    gone = util.apply_nms(_cuda(recs), min_size=10 ** 6)
    assert gone.shape == (260, 420) and gone.dtype == np.uint32 and not gone.any()


def test_cuda_records_take_the_device_path(cases, monkeypatch):
    from micro_sam_amd import util
    recs = cases[2]["recs"]
    want = util.apply_nms(_numpy(recs), min_size=30, nms_thresh=0.5)

    def host_only(*a, **k):
        raise AssertionError("the host path ran")
    monkeypatch.setattr(util, "_tiled_overlap_scores", host_only)
    monkeypatch.setattr(util, "mask_data_to_segmentation", host_only)
    assert np.array_equal(util.apply_nms(_cuda(recs), min_size=30, nms_thresh=0.5), want)
    with pytest.raises(AssertionError, match="host path"):                             # numpy records still go there
        util.apply_nms(_numpy(recs), min_size=30, nms_thresh=0.5)


def test_shared_seg_ids_of_different_tiles_merge_as_on_the_host(cases):
    """inference._merge_tiled_records: every record paints its own seg_id, and the ids restart in every tile - touching pieces of equal
    id are one component, exactly as util.mask_data_to_segmentation paints them on the host."""
    from micro_sam_amd import inference, util
    recs = [dict(r, area=int(r["segmentation"].sum()), seg_id=1 + k % 7) for k, r in enumerate(cases[3]["recs"])]
    want = util.mask_data_to_segmentation(_numpy(recs), shape=(300, 420), min_object_size=0)
    distinct = util.mask_data_to_segmentation([{k: v for k, v in r.items() if k != "seg_id"} for r in recs], shape=(300, 420))
    assert not np.array_equal(want, distinct)                                           # the shared ids matter on this input
    assert np.array_equal(inference._merge_tiled_records(_cuda(recs), (300, 420)), want)


def _wsi_records(g, n_per_tile=50):
    """About 200 records of the 2 x 2 tiles of 512 with halo 64 of a 1152 x 1152 image (outer blocks of 640 x 640), synthetic masks."""
    recs = []
    yy, xx = np.mgrid[0:640, 0:640]
    for oy, ox in [(0, 0), (0, 512), (512, 0), (512, 512)]:
        for _ in range(n_per_tile):
            cy, cx, r = g.integers(10, 630), g.integers(10, 630), g.integers(10, 60)
            m = (yy - cy) ** 2 + ((xx - cx) * g.uniform(0.6, 1.4)) ** 2 < r * r
            recs.append(dict(T.record(m, (oy, ox)), predicted_iou=float(g.uniform(0.5, 1.0)), stability_score=float(g.uniform(0.5, 1.0))))
    return recs


def test_timing_record_of_host_and_device_merge(tmp_path):
    """Seconds of util.apply_nms on ~200 tile-local records of a 1152 x 1152 image: numpy records (the host path) and CUDA records (the
    device path, after one warm-up).  Recorded, not asserted; the results are compared."""
    from micro_sam_amd import util
    recs = _wsi_records(np.random.default_rng(11))
    dev = _cuda(recs)
    kw = dict(min_size=25, nms_thresh=0.5, shape=(1152, 1152))
    t0 = time.perf_counter()
    host = util.apply_nms(_numpy(recs), **kw)
    t_host = time.perf_counter() - t0
    # CUDA records without the device path: one pageable copy per mask, then the host path
    t0 = time.perf_counter()
    util.apply_nms([dict(r, segmentation=r["segmentation"].cpu().numpy()) for r in dev], **kw)
    t_host_from_device = time.perf_counter() - t0
    util.apply_nms(dev, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = util.apply_nms(dev, **kw)
    t_dev = time.perf_counter() - t0
    assert np.array_equal(got, host) and got.max() > 20
    rec = {"records": len(recs), "image": [1152, 1152], "tile": [640, 640], "host_seconds": t_host,
           "host_seconds_with_mask_download": t_host_from_device, "device_seconds": t_dev, "mask_bytes_not_downloaded_per_record": 640 * 640}
    print("\ntiled merge, host path vs device path:", json.dumps(rec))
    out = os.environ.get("MSAM_TIMING_DIR") or str(tmp_path)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "tiled_merge.json"), "w") as fh:
        json.dump(rec, fh)
