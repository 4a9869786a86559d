"""msam_tiled_mask_overlaps / msam_paint_tiled (csrc/tilemerge.hip) compiled for the host (tests/hip_host_shim.build_library) and driven
through the C ABI as tests/test_host_library.py drives the rest: the kernels' indexing - word rows that straddle a 32-row group of the
window, tiles of different shapes, tail bits, the bounds guards - against numpy slicing, bit for bit.  The GPU suite runs the same
comparisons on the device (tests/test_gpu_tiled_merge.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import tiled_merge_cases as T
from hip_host_shim import build_library
from oracle import amg_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_lib")), ROOT)
    lib.msam_last_error.restype = C.c_char_p
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _overlaps(lib, recs, pairs):
    words, off, geom = T.table(recs)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    inter = np.full(len(pairs), -7, np.int32)
    rc = lib.msam_tiled_mask_overlaps(_p(words), _p(off), _p(geom), len(recs), _p(pairs), len(pairs), _p(inter), None)
    assert rc == 0, lib.msam_last_error()
    return inter


def _paint(lib, recs, order, shape):
    words, off, geom = T.table(recs)
    order = np.ascontiguousarray(order, np.int32)
    label = np.full(shape, -7, np.int32)
    rc = lib.msam_paint_tiled(_p(words), _p(off), _p(geom), _p(order), len(order), shape[0], shape[1], _p(label), None)
    assert rc == 0, lib.msam_last_error()
    return label


@pytest.mark.parametrize("seed", T.SEEDS)
def test_overlaps_of_all_candidate_pairs_are_the_numpy_counts(lib, seed):
    recs = T.tiled_records(seed)
    T.check_preconditions(recs, A)
    pairs = T.candidate_pairs(recs)
    want = np.array([T.overlap(recs[i], recs[j]) for i, j in pairs.tolist()], np.int32)
    assert np.array_equal(_overlaps(lib, recs, pairs), want)
    assert np.array_equal(_overlaps(lib, recs, pairs[:, ::-1]), want)                  # symmetric
    # the oracle's dense matrix is these counts over the IoU denominator
    ref = A.tiled_mask_overlap_matrix([r["segmentation"] for r in recs], [r["bbox"] for r in recs], [r["global_bbox"] for r in recs], False)
    area = np.array([r["segmentation"].sum() for r in recs], np.float64)
    for (i, j), n in zip(pairs.tolist(), want.tolist()):
        assert abs(float(ref[i, j]) - n / (area[i] + area[j] - n)) < 1e-6


def test_overlap_hand_cases(lib):
    a = np.zeros((40, 40), bool); a[5:15, 5:15] = True
    b = np.zeros((40, 40), bool); b[25:35, 15:25] = True
    recs = [T.record(a, (20, 100)), T.record(b, (0, 90))]                    # two 10 x 10 squares of different tiles that coincide
    assert recs[0]["global_bbox"] == recs[1]["global_bbox"] == [105, 25, 9, 9]
    assert _overlaps(lib, recs, [(0, 1)]).tolist() == [81]
    # a 1 x 1 window: the boxes share one column and one row
    c = np.zeros((70, 50), bool); c[10:20, 10:20] = True
    d = np.zeros((33, 90), bool); d[3:9, 4:30] = True
    recs = [T.record(c, (0, 0)), T.record(d, (15, 14))]                      # c: x 10..19, y 10..19; d: x 18..44, y 18..24
    assert T.window(*recs) == (18, 19, 18, 19)
    assert _overlaps(lib, recs, [(0, 1)]).tolist() == [T.overlap(*recs)] == [1]
    # an empty window (the boxes touch: x1 == x0), a pair in one tile, a record with itself
    e = np.zeros((70, 50), bool); e[12:30, 19:40] = True
    f = np.zeros((70, 50), bool); f[0:25, 0:25] = True
    recs = [T.record(c, (0, 0)), T.record(e, (0, 0)), T.record(f, (0, 0))]
    assert T.window(recs[0], recs[1])[:2] == (19, 19)
    got = _overlaps(lib, recs, [(0, 1), (0, 2), (1, 2), (2, 2)])
    assert got.tolist() == [0, 81, T.overlap(recs[1], recs[2]), 24 * 24] and got[2] > 0
    # an object that touches the last row of a 150-high tile (word row 4 holds 22 rows) against one of a tile 17 rows lower
    g = np.zeros((150, 200), bool); g[80:150, 30:90] = True
    h = np.zeros((150, 200), bool); h[40:149, 20:70] = True
    recs = [T.record(g, (0, 0)), T.record(h, (17, 25))]
    assert _overlaps(lib, recs, [(0, 1)]).tolist() == [T.overlap(*recs)] and T.overlap(*recs) > 1000
    # pair indices outside the table give 0
    assert _overlaps(lib, recs, [(0, 2), (-1, 1)]).tolist() == [0, 0]


@pytest.mark.parametrize("seed", T.SEEDS)
def test_paint_is_the_exclusive_merge_of_the_host(lib, seed):
    from micro_sam_amd import util
    recs = T.tiled_records(seed)
    for r in recs:
        r["area"] = int(r["segmentation"].sum())
    order = sorted(range(len(recs)), key=lambda i: recs[i]["area"], reverse=True)
    shape = A.infer_tiled_shape(recs)
    got = _paint(lib, recs, order, shape)
    assert np.array_equal(got, T.paint(recs, order, shape))
    host = util.mask_data_to_segmentation([dict(r) for r in recs], shape=shape, label_masks=False)
    assert T.same_partition(got, host.astype(np.int64)) and len(np.unique(got)) > 30
    # another order paints another image: the first painter wins
    assert np.array_equal(_paint(lib, recs, order[::-1], shape), T.paint(recs, order[::-1], shape))
    assert not T.same_partition(got, _paint(lib, recs, order[::-1], shape))
    # painted image + numpy labelling = the host's label image
    ref = util.mask_data_to_segmentation([dict(r) for r in recs], shape=shape)
    assert np.array_equal(util._label_equal_value_components(got.astype(np.uint32)), ref)


def test_first_painter_wins(lib):
    a = np.zeros((40, 60), bool); a[4:30, 5:50] = True
    b = np.zeros((50, 40), bool); b[10:40, 2:30] = True
    recs = [T.record(a, (3, 7)), T.record(b, (0, 30))]                       # image: a = y 7..32, x 12..56; b = y 10..39, x 32..59
    first_a, first_b = _paint(lib, recs, [0, 1], (64, 70)), _paint(lib, recs, [1, 0], (64, 70))
    assert np.array_equal(first_a, T.paint(recs, [0, 1], (64, 70))) and np.array_equal(first_b, T.paint(recs, [1, 0], (64, 70)))
    assert first_a[15, 40] == 2 and first_b[15, 40] == 2 and first_a[15, 20] == 2 and first_b[15, 20] == 1
    assert (first_a == 2).sum() == 25 * 44 and (first_b == 2).sum() == 29 * 27          # bw / bh = max - min: last row / column unpainted
    assert not _paint(lib, recs, [], (64, 70)).any()                         # nothing to paint: the image is zeroed


def test_malformed_tables_do_not_leave_their_buffers(lib):
    """The guards of the kernels: a window that leaves the image paints its inside part only, a bbox that leaves its tile reads zeros."""
    a = np.ones((40, 60), bool)
    words, off, geom = T.table([T.record(a, (0, 0))])
    geom[0, 2:8] = [50, 30, 40, 40, 40, 25]                                  # bbox x 50..89, y 30..69 of a 40 x 60 tile; image 32 x 48
    label = np.full((36, 48), -7, np.int32)                                  # (spare rows: must stay untouched)
    order = np.zeros(1, np.int32)
    assert lib.msam_paint_tiled(_p(words), _p(off), _p(geom), _p(order), 1, 32, 48, _p(label), None) == 0
    want = np.zeros((32, 48), np.int32)
    want[25:32, 40:48] = 1                  # rows 30..39, columns 50..59 of the tile exist: image rows 25..34, columns 40..49, clipped
    assert np.array_equal(label[:32], want) and (label[32:] == -7).all()
    pairs = np.zeros((1, 2), np.int32)
    inter = np.full(1, -7, np.int32)
    assert lib.msam_tiled_mask_overlaps(_p(words), _p(off), _p(geom), 1, _p(pairs), 1, _p(inter), None) == 0
    assert inter[0] == 100


def test_null_and_negative_arguments_are_refused(lib):
    words, off, geom = T.table([T.record(np.ones((8, 8), bool), (0, 0))])
    pairs, inter, order, label = np.zeros((1, 2), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((8, 8), np.int32)
    good = [_p(words), _p(off), _p(geom), 1, _p(pairs), 1, _p(inter), None]
    assert lib.msam_tiled_mask_overlaps(*good) == 0
    for k in (0, 1, 2, 4, 6):
        assert lib.msam_tiled_mask_overlaps(*[None if i == k else v for i, v in enumerate(good)]) == 1
        assert b"msam_tiled_mask_overlaps" in lib.msam_last_error()
    assert lib.msam_tiled_mask_overlaps(*[-1 if i == 3 else v for i, v in enumerate(good)]) == 1
    assert lib.msam_tiled_mask_overlaps(*[-1 if i == 5 else v for i, v in enumerate(good)]) == 1
    good = [_p(words), _p(off), _p(geom), _p(order), 1, 8, 8, _p(label), None]
    assert lib.msam_paint_tiled(*good) == 0
    for k in (0, 1, 2, 3, 7):
        assert lib.msam_paint_tiled(*[None if i == k else v for i, v in enumerate(good)]) == 1
        assert b"msam_paint_tiled" in lib.msam_last_error()
    for k, bad in ((4, -1), (5, 0), (6, -3)):
        assert lib.msam_paint_tiled(*[bad if i == k else v for i, v in enumerate(good)]) == 1


# ------------------------------------------------------------------------------------------------------------- the product's device path

@pytest.fixture(scope="module")
def on_host(tmp_path_factory):
    """The product's Python layer on the host-compiled library (tests/host_product.py): CPU tensors stand in for device tensors."""
    from host_product import product_on_host
    with product_on_host(str(tmp_path_factory.mktemp("host_product"))):
        yield


def _tensors(recs):
    import torch
    return [dict(r, segmentation=torch.from_numpy(r["segmentation"])) for r in recs]


@pytest.mark.parametrize("iomin", [False, True])
@pytest.mark.parametrize("seed", T.SEEDS)
def test_device_path_of_apply_nms_is_the_oracle(on_host, seed, iomin):
    """util._apply_nms_tiled_device (what util.apply_nms runs for CUDA records) from packing to the relabelled image: bit for bit
    the oracle's apply_nms, ids included."""
    from micro_sam_amd import util
    recs = T.tiled_records(seed)
    for kw in T.KWARGS:
        args = dict(dict(shape=A.infer_tiled_shape(recs), perform_box_nms=False, nms_thresh=0.9, max_size=None), **kw)
        got = util._apply_nms_tiled_device(_tensors(recs), intersection_over_min=iomin, **args)
        assert got.dtype == np.uint32 and got.max() > 0
        assert np.array_equal(got, A.apply_nms([dict(r) for r in recs], intersection_over_min=iomin, **kw))


def test_device_path_box_nms_explicit_shape_nothing_left_and_refusals(on_host):
    from micro_sam_amd import util
    recs = T.tiled_records(1)
    args = dict(min_size=10, perform_box_nms=True, nms_thresh=0.5, max_size=None, intersection_over_min=False)
    assert np.array_equal(util._apply_nms_tiled_device(_tensors(recs), shape=(260, 420), **args),
                          A.apply_nms([dict(r) for r in recs], min_size=10, perform_box_nms=True, nms_thresh=0.5))
    args = dict(min_size=0, perform_box_nms=False, nms_thresh=0.9, max_size=None, intersection_over_min=False)
    assert np.array_equal(util._apply_nms_tiled_device(_tensors(recs), shape=(310, 430), **args),
                          A.apply_nms([dict(r) for r in recs], min_size=0, shape=(310, 430)))
    gone = util._apply_nms_tiled_device(_tensors(recs), shape=(260, 420), **dict(args, min_size=10 ** 6))
    assert gone.shape == (260, 420) and not gone.any()
    # a window that leaves the shape, a bbox that leaves its tile: the host path has to answer
    assert util._apply_nms_tiled_device(_tensors(recs), shape=(200, 420), **args) is None
    bad = _tensors(recs)
    bad[5] = dict(bad[5], bbox=[190, 3, 20, 5])
    assert util._apply_nms_tiled_device(bad, shape=(260, 420), **args) is None


def test_device_merge_paints_shared_seg_ids_as_the_host_does(on_host):
    """Records of different tiles may carry the same seg_id (inference.batched_tiled_inference numbers them per tile): touching pieces
    of equal id are one component on the host, and on the device."""
    from micro_sam_amd import util
    recs = [dict(r, area=int(r["segmentation"].sum()), seg_id=1 + k % 7) for k, r in enumerate(T.tiled_records(3))]
    want = util.mask_data_to_segmentation([dict(r) for r in recs], shape=(300, 420), min_object_size=0)
    distinct = util.mask_data_to_segmentation([{k: v for k, v in r.items() if k != "seg_id"} for r in recs], shape=(300, 420))
    assert not np.array_equal(want, distinct)
    order = sorted(range(len(recs)), key=lambda i: recs[i]["area"], reverse=True)
    got = util._merge_tiled_device(util._TiledTable(_tensors(recs)), order, (300, 420), 0, seg_ids=[recs[i]["seg_id"] for i in order])
    assert np.array_equal(got, want)
