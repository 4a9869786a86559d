"""csrc/merge3d.hip on the device, everything for exact equality with the host functions of micro_sam_amd.multi_dimensional_segmentation
on the same arrays: ops.close_gaps_z against _preprocess_closing on the volumes of tests/merge3d_cases.py (the labelling flag 0 in every
case, two calls bit for bit), ops.label_z_ranges and ops.apply_label_lut against numpy, merge_instance_segmentation_3d and
automatic_3d_segmentation device route against host route, and automatic_segmentation.automatic_instance_segmentation end to end."""
import numpy as np
import pytest
import torch

import merge3d_cases as MC

pytestmark = pytest.mark.gpu

CASES = {name: (vol, gap) for name, vol, gap in MC.cases()}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def model(dev, vit_b_sd):
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=vit_b_sd)
    vol = np.stack([synthetic_tile(s, (512, 512)) for s in (11, 12, 13, 14)])
    return predictor, vol


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_close_gaps_equals_the_host_function(dev, name):
    from micro_sam_amd import ops
    vol, gap = CASES[name]
    ref, offset = MC.host_close(vol, gap)
    t = torch.as_tensor(vol, device=dev)
    out, result = ops.close_gaps_z(t, gap)
    out2, result2 = ops.close_gaps_z(t, gap, id_limit=int(vol.max()) + 1)
    got, res = out.cpu().numpy(), result.tolist()
    print(f"{name}: result {res}, host offset {offset}, differing voxels {int((got != ref).sum())}")
    assert res == [offset, 0, 0, 0]
    assert np.array_equal(got, ref)
    assert torch.equal(out, out2) and torch.equal(result, result2)            # two calls agree bit for bit
    assert torch.equal(t, torch.as_tensor(vol, device=dev))                   # the input is left alone


def test_close_gaps_flags_and_workspace(dev):
    from micro_sam_amd import _lib, ops
    vol = CASES["bridged"][0].copy()
    vol[1, 0, 0] = -3
    _, result = ops.close_gaps_z(torch.as_tensor(vol, device=dev), 1)
    assert result.tolist()[1:] == [1, 0, 0]
    vol, gap = CASES["painting_order"]
    t = torch.as_tensor(vol, device=dev)
    need = int(_lib.load().msam_close_gaps_workspace_bytes(*vol.shape, gap, int(vol.max()) + 1))
    ws = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=dev)      # a caller's workspace: nothing past its end is touched
    out, result = ops.close_gaps_z(t, gap, workspace=ws[:need])
    assert np.array_equal(out.cpu().numpy(), MC.host_close(vol, gap)[0]) and bool((ws[need:] == 0xAB).all())
    with pytest.raises(ValueError, match="workspace"):
        ops.close_gaps_z(t, gap, workspace=ws[:need - 4])
    empty, result = ops.close_gaps_z(torch.zeros((0, 4, 4), dtype=torch.int32, device=dev), 1)
    assert empty.shape == (0, 4, 4) and result.tolist() == [1, 0, 0, 0]


def test_label_z_ranges(dev):
    from micro_sam_amd import ops
    vol = CASES["repeating_ids"][0].copy()
    vol[0, 0, 0] = vol[3, 23, 29] = 33                       # slices 0 and Z - 1 only
    zr, flag = ops.label_z_ranges(torch.as_tensor(vol, device=dev), 45)
    got = zr.cpu().numpy()
    assert flag.item() == 0 and np.array_equal(got, MC.z_ranges_ref(vol, 45))
    assert got[33].tolist() == [0, 3] and got[0].tolist() == [4, -1] and got[44].tolist() == [4, -1]
    zr, flag = ops.label_z_ranges(torch.as_tensor(vol, device=dev), 34)
    assert flag.item() == 1 and np.array_equal(zr.cpu().numpy(), MC.z_ranges_ref(vol, 34))
    wide = CASES["wide_gap1"][0]
    zr, flag = ops.label_z_ranges(torch.as_tensor(wide, device=dev), int(wide.max()) + 3)
    assert flag.item() == 0 and np.array_equal(zr.cpu().numpy(), MC.z_ranges_ref(wide, int(wide.max()) + 3))


def test_apply_label_lut(dev):
    from micro_sam_amd import ops
    rng = np.random.default_rng(0)
    vol = rng.integers(0, 50, (3, 37, 129)).astype(np.int32)
    lut = rng.integers(0, 1000, 50).astype(np.int32)
    t, l = torch.as_tensor(vol, device=dev), torch.as_tensor(lut, device=dev)
    out, flag = ops.apply_label_lut(t, l)
    assert flag.item() == 0 and np.array_equal(out.cpu().numpy(), lut[vol])
    out, flag = ops.apply_label_lut(t, l[:40].contiguous())
    assert flag.item() == 1 and np.array_equal(out.cpu().numpy(), np.where(vol < 40, lut[np.minimum(vol, 39)], 0))
    same, flag = ops.apply_label_lut(t, l, out=t)                             # in place
    assert same is t and flag.item() == 0 and np.array_equal(t.cpu().numpy(), lut[vol])


def _merge_both(vol, **kw):
    from micro_sam_amd import multi_dimensional_segmentation as M
    host = M.merge_instance_segmentation_3d(vol.copy(), **kw)
    got = M.merge_instance_segmentation_3d(torch.as_tensor(vol.astype(np.int32)).cuda(), **kw)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.int32
    return host, got.cpu().numpy()


def test_merge_instance_segmentation_3d_device_equals_host(dev):
    from test_merge_3d_host import _blobs, _stack      # tests/ is on sys.path (pytest prepend import mode)
    seg = _blobs(0, 256)
    host, got = _merge_both(_stack(seg, 5))
    assert np.array_equal(got, host) and len(np.unique(host)) > 10
    host, got = _merge_both(_stack(_blobs(1), 5, blank=(2,)), gap_closing=1)
    assert np.array_equal(got, host)
    for z in range(1, 5):
        assert np.array_equal(np.unique(got[0]), np.unique(got[z]))            # the closed gap: every object runs through
    from scipy import ndimage
    vol = _stack(seg, 4)
    y, x = np.argwhere(ndimage.binary_erosion(seg == 0, iterations=5))[0]      # room for a one-slice object in the background
    lone = int(vol.max()) + 1
    vol[1, y - 2:y + 3, x - 2:x + 3] = lone
    host, got = _merge_both(vol, min_z_extent=2)
    plain, plain_dev = _merge_both(vol)
    assert np.array_equal(got, host) and np.array_equal(plain_dev, plain)
    assert (plain[1][vol[1] == lone] != 0).all() and (host[1][vol[1] == lone] == 0).all()      # min_z_extent = 2 drops it
    host, got = _merge_both(vol, gap_closing=1, min_z_extent=3)
    assert np.array_equal(got, host)
    for name in ("painting_order", "blobs", "wide_gap2", "single_slice"):
        v, gap = CASES[name]
        host, got = _merge_both(v, gap_closing=gap, min_z_extent=2)
        assert np.array_equal(got, host), name


def test_ids_in_two_slices_are_refused_as_on_the_host(dev):
    from micro_sam_amd import multi_dimensional_segmentation as M
    vol, gap = CASES["reset"]                                # the offset falls back to 1: the closed volume repeats ids
    with pytest.raises(ValueError, match="unique across slices") as host_err:
        M.merge_instance_segmentation_3d(vol.copy(), gap_closing=gap)
    with pytest.raises(ValueError, match="unique across slices") as dev_err:
        M.merge_instance_segmentation_3d(torch.as_tensor(vol, device=dev), gap_closing=gap)
    assert str(dev_err.value) == str(host_err.value)
    rep = CASES["repeating_ids"][0]
    with pytest.raises(ValueError, match="unique across slices"):
        M.merge_instance_segmentation_3d(torch.as_tensor(rep, device=dev))
    host, got = _merge_both(CASES["empty_slices"][0], gap_closing=1)          # empty first and interior slices: no error, equal
    assert np.array_equal(got, host)


def test_automatic_3d_segmentation_device_merge_equals_host_merge(model):
    from micro_sam_amd import multi_dimensional_segmentation as M
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator
    predictor, vol = model
    kw = dict(gap_closing=1, min_z_extent=2, batch_size=2, pred_iou_thresh=0.5, stability_score_thresh=0.5)
    host = M.automatic_3d_segmentation(vol, predictor, AutomaticMaskGenerator(predictor, points_per_side=6), device_merge=False, **kw)
    got = M.automatic_3d_segmentation(vol, predictor, AutomaticMaskGenerator(predictor, points_per_side=6), device_merge=True, **kw)
    auto = M.automatic_3d_segmentation(vol, predictor, AutomaticMaskGenerator(predictor, points_per_side=6), **kw)
    loop = M.automatic_3d_segmentation(vol, predictor, AutomaticMaskGenerator(predictor, points_per_side=6), device_merge=True,
                                       decode_lanes=0, **kw)                    # labels uploaded after the reference's loop
    assert got.dtype == np.uint32 and got.shape == vol.shape and int(host.max()) > 0
    assert np.array_equal(got, host) and np.array_equal(auto, host) and np.array_equal(loop, host)


def test_automatic_instance_segmentation(model, tmp_path, capsys):
    from micro_sam_amd import multi_dimensional_segmentation as M
    from micro_sam_amd import util
    from micro_sam_amd.automatic_segmentation import automatic_instance_segmentation
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator
    predictor, vol = model
    gen_kw = dict(pred_iou_thresh=0.5, stability_score_thresh=0.5)
    amg = AutomaticMaskGenerator(predictor, points_per_side=6)
    out2 = tmp_path / "seg2d.png"                                               # the suffix is forced to .tif
    seg = automatic_instance_segmentation(predictor, amg, vol[0], output_path=out2, verbose=False, **gen_kw)
    by_hand = AutomaticMaskGenerator(predictor, points_per_side=6)
    by_hand.initialize(vol[0], image_embeddings=util.precompute_image_embeddings(predictor, vol[0], ndim=2, verbose=False), verbose=False)
    assert np.array_equal(seg, by_hand.generate(**gen_kw)) and int(seg.max()) > 0
    assert (tmp_path / "seg2d.tif").exists() and not out2.exists()
    assert np.array_equal(util.load_image_data(tmp_path / "seg2d.tif"), seg)
    assert automatic_instance_segmentation(predictor, amg, vol[0], output_path=out2, verbose=False, **gen_kw) is None
    assert "already stored" in capsys.readouterr().out
    kw3 = dict(gap_closing=1, min_z_extent=2, batch_size=2, **gen_kw)
    seg3, emb = automatic_instance_segmentation(predictor, AutomaticMaskGenerator(predictor, points_per_side=6), vol,
                                                output_path=tmp_path / "seg3d.tif", verbose=False, return_embeddings=True, **kw3)
    ref3 = M.automatic_3d_segmentation(vol, predictor, AutomaticMaskGenerator(predictor, points_per_side=6), **kw3)
    assert np.array_equal(seg3, ref3) and emb["features"].shape[0] == vol.shape[0]
    assert np.array_equal(util.load_image_data(tmp_path / "seg3d.tif"), seg3)
