"""micro_sam_amd.object_classification on the device against the restatement of the reference (tests/object_features_ref.py), on real
embeddings of the synthetic vit_b model: 2-D, tiled, 3-D, 3-D tiled, a zarr-cached tiled container, device inputs, run-to-run identity,
the projection and run_prediction_with_object_classifier."""
import numpy as np
import pytest
import torch

import object_features_ref as REF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def predictor():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_state_dict
    return util.get_sam_model("vit_b", device="cuda:0", state_dict=synthetic_state_dict("vit_b", 0))


def _data(seed, shape):
    from micro_sam_amd.synthetic import synthetic_tile_with_labels
    return synthetic_tile_with_labels(seed, shape)


def _host(x):
    return x.detach().float().cpu().numpy() if torch.is_tensor(x) else np.asarray(x[:] if not isinstance(x, np.ndarray) else x)


def _blocks(feats):
    from micro_sam_amd.tiling import Blocking
    tiling = Blocking([0, 0], feats.attrs["shape"], feats.attrs["tile_shape"])
    out = []
    for t in range(tiling.number_of_blocks):
        ob = tiling.get_block_with_halo(t, list(feats.attrs["halo"])).outer_block
        out.append((t, (ob.begin[0], ob.begin[1], ob.end[0], ob.end[1])))
    return out


class _HostTiles(dict):
    def __init__(self, feats):
        super().__init__({str(k): _host(feats[k].data if hasattr(feats[k], "data") else feats[k]) for k in feats.keys()})


def _check(got, ref, emb_max):
    (ids, f), (rids, rf) = got, ref
    assert ids.dtype == np.int64 and np.array_equal(ids, rids)
    assert f.dtype == rf.dtype and f.shape == rf.shape
    assert np.array_equal(f[:, 0], rf[:, 0])
    assert np.abs(f[:, 1:].astype(np.float64) - rf[:, 1:]).max(initial=0) <= 1e-6 * emb_max


@pytest.mark.parametrize("shape", [(1024, 1024), (700, 1100)])
def test_2d_matches_reference(predictor, shape):
    from micro_sam_amd import object_classification as OC
    from micro_sam_amd import util
    image, labels = _data(1, shape)
    emb = util.precompute_image_embeddings(predictor, image, verbose=False)
    got = OC.compute_object_features(emb, labels, verbose=False)
    feats = _host(emb["features"])
    _check(got, REF.compute_object_features(feats, labels), np.abs(feats).max())
    assert got[1].dtype == np.float64 and len(got[0]) > 5
    # device-tensor embeddings and segmentation: the same result, bit for bit; two calls are bit-identical
    emb_dev = util.precompute_image_embeddings(predictor, image, verbose=False, keep_on_device=True)
    again = OC.compute_object_features(emb_dev, torch.from_numpy(labels).cuda(), verbose=False)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    assert np.array_equal(OC.compute_object_features(emb, labels, verbose=False)[1], got[1])


def test_tiled_2d_and_zarr_cache(predictor, tmp_path):
    from micro_sam_amd import object_classification as OC
    from micro_sam_amd import util
    image, labels = _data(2, (1100, 900))
    emb = util.precompute_image_embeddings(predictor, image, tile_shape=(512, 512), halo=(64, 64), verbose=False)
    feats = emb["features"]
    got = OC.compute_object_features(emb, labels, verbose=False)
    host = _HostTiles(feats)
    ref = REF.compute_object_features(host, labels, is_tiled=True, tile_blocks=_blocks(feats))
    _check(got, ref, max(np.abs(v).max() for v in host.values()))
    assert got[1].dtype == np.float32
    path = str(tmp_path / "emb.zarr")
    util.precompute_image_embeddings(predictor, image, save_path=path, tile_shape=(512, 512), halo=(64, 64), verbose=False)
    cached = util.precompute_image_embeddings(predictor, image, save_path=path, tile_shape=(512, 512), halo=(64, 64), verbose=False,
                                              lazy_loading=True)
    got_z = OC.compute_object_features(cached, labels, verbose=False)
    assert np.array_equal(got_z[0], got[0])
    assert np.abs(got_z[1][:, 1:].astype(np.float64) - ref[1][:, 1:]).max() <= 1e-6 * max(np.abs(v).max() for v in host.values())


def test_3d_and_3d_tiled_and_projection(predictor):
    from micro_sam_amd import object_classification as OC
    from micro_sam_amd import util
    pairs = [_data(10 + z, (512, 640)) for z in range(4)]
    volume = np.stack([p[0] for p in pairs])
    labels = np.stack([p[1] for p in pairs]).astype(np.uint32)
    emb = util.precompute_image_embeddings(predictor, volume, verbose=False, batch_size=2)
    got = OC.compute_object_features(emb, labels, verbose=False)
    feats = _host(emb["features"])
    _check(got, REF.compute_object_features(feats, labels), np.abs(feats).max())
    pred = (np.arange(len(got[0])) % 4).astype(np.int64)
    proj = OC.project_prediction_to_segmentation(labels, pred, got[0])
    assert proj.dtype == pred.dtype and np.array_equal(proj, REF.project_prediction_to_segmentation(labels, pred, got[0]))
    proj_dev = OC.project_prediction_to_segmentation(torch.from_numpy(labels.astype(np.int32)).cuda(), pred, got[0])
    assert proj_dev.is_cuda and np.array_equal(proj_dev.cpu().numpy(), proj)

    vol_t, lab_t = volume[:3, :, :600], labels[:3, :, :600]
    emb_t = util.precompute_image_embeddings(predictor, vol_t, tile_shape=(384, 384), halo=(32, 32), verbose=False)
    got_t = OC.compute_object_features(emb_t, lab_t, verbose=False)
    host = _HostTiles(emb_t["features"])
    ref_t = REF.compute_object_features(host, lab_t, is_tiled=True, tile_blocks=_blocks(emb_t["features"]))
    _check(got_t, ref_t, max(np.abs(v).max() for v in host.values()))


def test_run_prediction_with_object_classifier(predictor, tmp_path):
    pytest.importorskip("sklearn")
    import joblib
    from sklearn.ensemble import RandomForestClassifier
    from micro_sam_amd import object_classification as OC
    from micro_sam_amd import util
    image, labels = _data(5, (512, 512))
    emb = util.precompute_image_embeddings(predictor, image, verbose=False)
    ids, feats = OC.compute_object_features(emb, labels, verbose=False)
    rf = RandomForestClassifier(n_estimators=8, random_state=0).fit(feats, (ids % 3) + 1)
    path = str(tmp_path / "rf.joblib")
    joblib.dump(rf, path)
    out = OC.run_prediction_with_object_classifier([image], [labels], predictor, path)
    assert len(out) == 1
    assert np.array_equal(out[0], REF.project_prediction_to_segmentation(labels, rf.predict(feats), ids))
