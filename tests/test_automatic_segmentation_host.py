"""micro_sam_amd.automatic_segmentation (reference micro_sam/automatic_segmentation.py), the parts that need no GPU: the suffix helper,
the output file (written once, read back by util.load_image_data with equal values, never overwritten), the shape checks and refusals
with the reference's messages, and the mode resolution of get_predictor_and_segmenter.  tests/test_gpu_merge3d.py runs the driver end
to end on the device."""
import os

import numpy as np
import pytest

from micro_sam_amd import automatic_segmentation as AS
from micro_sam_amd import util


class _Untouchable:
    """A predictor / segmenter that nothing may reach."""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name}")


@pytest.fixture()
def nothing_loads(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("work was started")
    monkeypatch.setattr(util, "load_image_data", refuse)
    monkeypatch.setattr(util, "precompute_image_embeddings", refuse)
    monkeypatch.setattr(AS, "automatic_3d_segmentation", refuse)


def test_suffix_helper(tmp_path):
    assert AS._add_suffix_to_output_path(tmp_path / "seg.tif", "_automatic") == str((tmp_path / "seg_automatic.tif").resolve())
    assert AS._add_suffix_to_output_path(str(tmp_path / "seg"), "_automatic") == str((tmp_path / "seg_automatic.tif").resolve())
    assert AS._add_suffix_to_output_path(tmp_path / "a.b.png", "_x") == str((tmp_path / "a.b_x.png").resolve())
    assert AS._add_suffix_to_output_path("rel/seg.tiff", "") == os.path.join(os.getcwd(), "rel", "seg.tiff")


def test_an_existing_output_is_not_overwritten(tmp_path, capsys, nothing_loads):
    (tmp_path / "seg.tif").write_bytes(b"kept")
    for given in ("seg.tif", "seg.png", "seg"):                       # the suffix is forced before the look-up
        assert AS.automatic_instance_segmentation(_Untouchable(), _Untouchable(), "no_such_input.tif", output_path=tmp_path / given) is None
        assert f"The segmentation results are already stored at '{tmp_path / 'seg.tif'}'." in capsys.readouterr().out
    assert (tmp_path / "seg.tif").read_bytes() == b"kept"


def test_shape_checks(monkeypatch):
    monkeypatch.setattr(util, "precompute_image_embeddings", lambda **kw: pytest.fail("embeddings of a refused input"))
    monkeypatch.setattr(AS, "automatic_3d_segmentation", lambda **kw: pytest.fail("segmentation of a refused input"))
    with pytest.raises(ValueError, match=r"does not match the shape expectation of 2d inputs: \(2, 3, 8, 8\)"):
        AS.automatic_instance_segmentation(_Untouchable(), _Untouchable(), np.zeros((2, 3, 8, 8), np.uint8), ndim=2)
    with pytest.raises(ValueError, match=r"does not match the shape expectation of 3d inputs: \(8, 8\)"):
        AS.automatic_instance_segmentation(_Untouchable(), _Untouchable(), np.zeros((8, 8), np.uint8), ndim=3)
    with pytest.raises(ValueError, match="3d inputs"):
        AS.automatic_instance_segmentation(_Untouchable(), _Untouchable(), np.zeros((2, 2, 2, 8, 8), np.uint8))
    with pytest.raises(NotImplementedError):                         # a mask with a volume
        AS.automatic_instance_segmentation(_Untouchable(), _Untouchable(), np.zeros((3, 8, 8), np.uint8), mask_path=np.ones((3, 8, 8), bool))


def test_annotate_raises_before_anything_is_loaded(tmp_path, nothing_loads):
    with pytest.raises(NotImplementedError, match="napari"):
        AS.automatic_instance_segmentation(_Untouchable(), _Untouchable(), "no_such_input.tif", output_path=tmp_path / "seg.tif", annotate=True)
    assert not os.listdir(tmp_path)


def test_the_driver_hands_over_what_the_reference_hands_over(tmp_path, monkeypatch):
    """Inputs and masks from files, ndim from the data, the 3-d branch's keywords, the stored result."""
    vol = (np.arange(3 * 8 * 9).reshape(3, 8, 9) % 251).astype(np.uint8)
    np.save(tmp_path / "vol.npy", vol)
    seen = {}

    def fake_3d(**kw):
        seen.update(kw)
        return np.full(kw["volume"].shape, 7, np.uint32), {"features": "emb"}
    monkeypatch.setattr(AS, "automatic_3d_segmentation", fake_3d)
    seg, emb = AS.automatic_instance_segmentation("P", "S", str(tmp_path / "vol.npy"), output_path=tmp_path / "out.xyz", embedding_path="E",
                                                  tile_shape=(4, 4), halo=(1, 1), verbose=False, return_embeddings=True, batch_size=5,
                                                  gap_closing=1, min_z_extent=2, pred_iou_thresh=0.7)
    assert np.array_equal(seen.pop("volume"), vol)
    assert seen == dict(predictor="P", segmentor="S", embedding_path="E", tile_shape=(4, 4), halo=(1, 1), verbose=False,
                        return_embeddings=True, batch_size=5, gap_closing=1, min_z_extent=2, pred_iou_thresh=0.7)
    assert emb == {"features": "emb"} and (seg == 7).all()
    assert np.array_equal(util.load_image_data(tmp_path / "out.tif"), seg)

    class Segmenter:
        def initialize(self, **kw):
            self.init = kw

        def generate(self, **kw):
            self.gen = kw
            return np.ones((8, 9), np.uint32)
    s = Segmenter()
    mask = vol[0] > 100
    np.save(tmp_path / "mask.npy", mask)
    monkeypatch.setattr(util, "precompute_image_embeddings", lambda **kw: dict(kw, made=True))
    out = AS.automatic_instance_segmentation("P", s, vol[0], mask_path=str(tmp_path / "mask.npy"), verbose=False, tile_shape=(4, 4),
                                             halo=(1, 1), batch_size=3, foo=1)
    e = s.init.pop("image_embeddings")
    assert e["made"] and e["predictor"] == "P" and e["ndim"] == 2 and e["tile_shape"] == (4, 4) and e["batch_size"] == 3
    assert np.array_equal(e["mask"], mask) and np.array_equal(s.init.pop("mask"), mask) and np.array_equal(s.init.pop("image"), vol[0])
    assert s.init == dict(verbose=False) and s.gen == dict(foo=1) and (out == 1).all()      # (no decoder: tiling stays out of generate)


@pytest.mark.parametrize("shape", [(7, 9), (3, 7, 9), (1, 5, 5)])
def test_writer_round_trip(tmp_path, shape):
    rng = np.random.default_rng(1)
    seg = rng.integers(0, 2 ** 31 - 1, shape).astype(np.uint32)
    seg.reshape(-1)[:3] = [0, 2 ** 31 - 1, 70000]
    AS._write_segmentation(tmp_path / "seg.tif", seg)
    back = util.load_image_data(tmp_path / "seg.tif")
    assert np.array_equal(np.asarray(back).reshape(shape), seg)
    assert os.path.getsize(tmp_path / "seg.tif") > 0 and os.listdir(tmp_path) == ["seg.tif"]


def test_writer_compresses_and_refuses_what_it_cannot_store(tmp_path):
    seg = np.zeros((4, 64, 64), np.uint32)
    seg[:, 10:20, 10:20] = 3
    AS._write_segmentation(tmp_path / "seg.tif", seg)
    assert os.path.getsize(tmp_path / "seg.tif") < seg.nbytes // 4
    try:
        import imageio.v3  # noqa: F401
    except ImportError:                                              # the Pillow writer: 32-bit signed pages
        big = np.array([[0, 2 ** 31]], dtype=np.uint32)
        with pytest.raises(ValueError, match=r"2\^31 - 1"):
            AS._write_segmentation(tmp_path / "big.tif", big)
        assert not (tmp_path / "big.tif").exists()
    with pytest.raises(ValueError, match="2d or 3d integer"):
        AS._write_segmentation(tmp_path / "f.tif", np.zeros((4, 4), np.float32))


def test_mode_resolution(monkeypatch):
    made = []

    class Predictor:
        class model:
            image_encoder = "encoder"
    monkeypatch.setattr(AS, "get_decoder", lambda image_encoder, decoder_state, device: ("decoder", image_encoder, decoder_state, device))
    monkeypatch.setattr(AS, "get_instance_segmentation_generator", lambda **kw: made.append(kw) or "segmenter")
    p = Predictor()
    with_decoder, without = {"model_state": {}, "decoder_state": {"w": 1}}, {"model_state": {}}
    for mode in (None, "auto"):
        assert AS.get_predictor_and_segmenter("vit_b", predictor=p, state=with_decoder, segmentation_mode=mode, is_tiled=True, foo=2) == (p, "segmenter")
        assert made.pop() == dict(predictor=p, is_tiled=True, decoder=("decoder", "encoder", {"w": 1}, None), segmentation_mode="ais", foo=2)
        AS.get_predictor_and_segmenter("vit_b", predictor=p, state=without, segmentation_mode=mode)
        assert made.pop() == dict(predictor=p, is_tiled=False, decoder=None, segmentation_mode="amg")
    AS.get_predictor_and_segmenter("vit_b", predictor=p, state=with_decoder, segmentation_mode="AMG")
    assert made.pop()["decoder"] is None
    AS.get_predictor_and_segmenter("vit_b", predictor=p, state=with_decoder, segmentation_mode="apg")
    assert made.pop()["segmentation_mode"] == "apg"
    with pytest.raises(RuntimeError, match="You have passed 'segmentation_mode=apg', but your model does not contain a decoder."):
        AS.get_predictor_and_segmenter("vit_b", predictor=p, state=without, segmentation_mode="apg")
    with pytest.raises(AssertionError):
        AS.get_predictor_and_segmenter("vit_b", predictor=p)
    # without a predictor the model is loaded with its state
    monkeypatch.setattr(util, "get_device", lambda device=None: "the-device")
    monkeypatch.setattr(util, "get_sam_model", lambda **kw: (p, dict(with_decoder, kw=kw)))
    AS.get_predictor_and_segmenter("vit_l", checkpoint="ckpt.pt")
    got = made.pop()
    assert got["segmentation_mode"] == "ais" and got["decoder"][3] == "the-device"
