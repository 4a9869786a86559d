"""micro_sam_amd.object_classification on the CPU: the resize tables against scipy.ndimage.zoom, and the product's Python layer driving the
host-compiled library (tests/host_product.py) against the restatement of the reference (tests/object_features_ref.py) on small cases."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import object_features_ref as REF
from host_product import product_on_host
from micro_sam_amd import object_classification as OC
from micro_sam_amd.tiling import Blocking, TileArray, TiledFeatures


@pytest.mark.parametrize("R", [256, 200, 100, 65, 64])
def test_resize_tables_bit_equal_to_zoom(R):
    w_ref = ndi.zoom(np.eye(64), (R / 64, 1), order=1, mode="mirror", grid_mode=True)
    i0, i1, w = OC.bilinear_table(64, R)
    m = np.zeros((R, 64))
    m[np.arange(R), i0] += 1 - w
    m[np.arange(R), i1] += w
    assert np.array_equal(m, w_ref)
    x = np.arange(64, dtype=np.float64)
    assert np.array_equal((1 - w) * x[i0] + w * x[i1], ndi.zoom(x, R / 64, order=1, mode="mirror", grid_mode=True))
    for s in range(1, 4097):
        r = min(R, s)
        z = ndi.zoom(np.arange(s, dtype=np.float64), r / s, order=0, mode="mirror", grid_mode=True)
        assert np.array_equal(z, OC.nearest_table(s, r)), (s, r)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    with product_on_host(str(tmp_path_factory.mktemp("host_objfeat"))):
        yield


def _emb(rng, n=1):
    return rng.standard_normal((n, 1, 256, 64, 64)).astype(np.float32)


def _check(got, ref, emb_max):
    (ids, f), (rids, rf) = got, ref
    assert ids.dtype == np.int64 and np.array_equal(ids, rids)
    assert f.dtype == rf.dtype and f.shape == rf.shape
    assert np.array_equal(f[:, 0], rf[:, 0])
    assert np.abs(f[:, 1:].astype(np.float64) - rf[:, 1:]).max(initial=0) <= 1e-6 * emb_max


def _blocky(rng, shape, n_ids, block=6):
    small = rng.integers(0, n_ids + 1, tuple(-(-s // block) for s in shape))
    return np.kron(small, np.ones((block,) * len(shape), dtype=np.int64))[tuple(slice(0, s) for s in shape)].astype(np.uint32)


@pytest.mark.parametrize("shape,resize", [((96, 96), (256, 256)), ((90, 70), (256, 256)), ((200, 120), (100, 128)), ((40, 50), (256, 256)),
                                          ((120, 120), (48, 100))])
def test_2d_matches_reference(host, shape, resize):
    rng = np.random.default_rng(sum(shape))
    emb = _emb(rng)[0]
    seg = _blocky(rng, shape, 9)
    side = max(shape)
    gone = [min(set(range(side)) - set(OC.nearest_table(side, min(r, side)).tolist()), default=0) for r in resize]
    seg[min(gone[0], shape[0] - 1), min(gone[1], shape[1] - 1)] = 77      # a one-pixel object: vanishes when the label grid shrinks
    emb_d = {"features": emb, "input_size": (1024, 1024), "original_size": shape}
    got = OC.compute_object_features(emb_d, seg, resize, verbose=False)
    ref = REF.compute_object_features(emb, seg, resize_embedding_shape=resize)
    _check(got, ref, np.abs(emb).max())
    assert got[1].dtype == np.float64
    if max(shape) > min(resize):
        assert 77 not in got[0]


def _tiled(rng, shape, tile, halo, n_slices=None):
    tiling = Blocking([0, 0], shape, tile)
    feats = TiledFeatures(shape, tile, halo)
    blocks = []
    for t in range(tiling.number_of_blocks):
        ob = tiling.get_block_with_halo(t, list(halo)).outer_block
        data = torch.from_numpy(_emb(rng, n_slices or 1) if n_slices else _emb(rng)[0])
        feats[t] = TileArray(data, (0, 0), (0, 0))
        blocks.append((t, (ob.begin[0], ob.begin[1], ob.end[0], ob.end[1])))
    return feats, blocks


def test_tiled_2d_with_halo_and_vanishing_object(host):
    rng = np.random.default_rng(3)
    shape, tile, halo = (150, 130), (80, 80), (16, 16)
    feats, blocks = _tiled(rng, shape, tile, halo)
    seg = _blocky(rng, shape, 12, 9)
    # a one-pixel object only the corner tile's outer block (rows / columns 64..) sees, at a row and column its 86 -> 64 label grid skips:
    # an all-zero row of the result
    skipped = sorted(set(range(86)) - set(OC.nearest_table(86, 64).tolist()))
    y = x = 64 + [k for k in skipped if 96 - 64 <= k < 130 - 64][0]
    seg[y, x] = 4000
    got = OC.compute_object_features({"features": feats, "input_size": None, "original_size": None}, seg, (64, 64), verbose=False)
    ref = REF.compute_object_features(feats, seg, is_tiled=True, tile_blocks=blocks, resize_embedding_shape=(64, 64))
    _check(got, ref, 5.5)
    assert got[1].dtype == np.float32 and 4000 in got[0] and not got[1][list(got[0]).index(4000)].any()


def test_3d_and_3d_tiled(host):
    rng = np.random.default_rng(4)
    emb = _emb(rng, 3)
    seg = _blocky(rng, (3, 70, 80), 8, 7)
    got = OC.compute_object_features({"features": torch.from_numpy(emb), "input_size": (1024, 1024), "original_size": (70, 80)}, seg,
                                     (96, 96), verbose=False)
    _check(got, REF.compute_object_features(emb, seg, resize_embedding_shape=(96, 96)), np.abs(emb).max())
    feats, blocks = _tiled(rng, (100, 90), (64, 64), (8, 8), n_slices=2)
    seg = _blocky(rng, (2, 100, 90), 10, 8)
    got = OC.compute_object_features({"features": feats, "input_size": None, "original_size": None}, seg, (72, 72), verbose=False)
    _check(got, REF.compute_object_features(feats, seg, is_tiled=True, tile_blocks=blocks, resize_embedding_shape=(72, 72)), 5.5)


@pytest.mark.parametrize("dtype,base", [(np.uint32, 0), (np.int64, 3 << 31), (np.int64, 1 << 40)])
def test_id_dtypes_and_large_ids(host, dtype, base):
    rng = np.random.default_rng(5)
    emb = _emb(rng)[0]
    seg = _blocky(rng, (80, 80), 6).astype(np.int64)
    seg = np.where(seg > 0, seg + base, 0).astype(dtype)
    d = {"features": emb, "input_size": (1024, 1024), "original_size": (80, 80)}
    got = OC.compute_object_features(d, seg, (128, 128), verbose=False)
    _check(got, REF.compute_object_features(emb, seg.astype(np.int64), resize_embedding_shape=(128, 128)), np.abs(emb).max())
    pred = np.arange(len(got[0]), dtype=np.int64) % 3 + 1
    proj = OC.project_prediction_to_segmentation(seg, pred, got[0])
    assert proj.shape == seg.shape and np.array_equal(proj, REF.project_prediction_to_segmentation(seg, pred, got[0]))


def test_empty_segmentation(host):
    rng = np.random.default_rng(6)
    d = {"features": _emb(rng)[0], "input_size": (1024, 1024), "original_size": (64, 64)}
    ids, f = OC.compute_object_features(d, np.zeros((64, 64), np.uint32), verbose=False)
    assert ids.shape == (0,) and ids.dtype == np.int64 and f.shape == (0, 257) and f.dtype == np.float64
    proj = OC.project_prediction_to_segmentation(np.zeros((5, 6, 7), np.uint16), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert proj.shape == (5, 6, 7) and not proj.any()


def test_argument_errors(host):
    rng = np.random.default_rng(7)
    d = {"features": _emb(rng)[0], "input_size": (1024, 1024), "original_size": (64, 64)}
    with pytest.raises(TypeError):
        OC.compute_object_features(d, np.ones((64, 64), np.float32), verbose=False)
    with pytest.raises(ValueError):
        OC.compute_object_features(d, -np.ones((64, 64), np.int32), verbose=False)
    with pytest.raises(ValueError):
        OC.compute_object_features(d, np.ones((64,), np.int32), verbose=False)
    with pytest.raises(TypeError):
        OC.project_prediction_to_segmentation(np.ones((4, 4), np.int32), np.array(["a"]), np.array([1]))
    from micro_sam_amd import ops
    labels, ids = torch.zeros(16, dtype=torch.int64), torch.ones(1, dtype=torch.int64)
    desc = np.zeros((1, ops.OBJFEAT_DESC), np.int64)
    desc[0] = (0, 4, 4, 4, 0, 64, 4, 4, 0, 0, 0, 64)
    itab, ftab = np.zeros(24, np.int32), np.zeros(8, np.float32)
    sums, area = torch.zeros((1, 256), dtype=torch.float64), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="embedding"):          # the embedding buffer is smaller than the unit's 64 x 64 x 256
        ops.objfeat_accumulate_batch(labels, ids, torch.zeros(256), desc, itab, ftab, sums, area)
    desc[0, ops.OF_LAB_H] = 5
    with pytest.raises(ValueError, match="labels"):
        ops.objfeat_accumulate_batch(labels, ids, torch.zeros(64 * 64 * 256), desc, itab, ftab, sums, area)
