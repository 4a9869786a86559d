"""ops.pack_bits / mask_iou_counts / mask_box_prompts / mask_logits / paint_max (csrc/propagate.hip) on the device: the cases of
tests/test_host_propagate.py through the tensor wrappers.  Counts, keep flags, nonempty flags and painted labels exactly, boxes bit for
bit against the host chain, the mask prompts against torch's CPU operator in fp64 outside the tie band (tests/propagate_ref.py);
garbage in the tail bits of the last word row wherever H is no multiple of 32."""
import numpy as np
import pytest
import torch

import propagate_ref as R

pytestmark = pytest.mark.gpu
NAMES = sorted(R.CASES)


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cache = {}

    def get(name):
        if name not in cache:
            m = R.masks(name)
            bits = R.with_garbage_tail(R.pack(m), m.shape[1])
            cache[name] = dict(masks=m, bits=torch.from_numpy(bits.view(np.int32)).cuda())
        return cache[name]
    return get


def _dev_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).cuda()


@pytest.mark.parametrize("name", NAMES)
def test_pack_bits(data, name):
    from micro_sam_amd import ops
    m = data(name)["masks"]
    got = ops.pack_bits(torch.from_numpy(m).cuda())
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), R.pack(m))
    assert torch.equal(ops.pack_bits(torch.from_numpy(m == 1).cuda()), got)              # bool input
    assert torch.equal(ops.unpack_bits(got, m.shape[1]), torch.from_numpy(m == 1).cuda())


@pytest.mark.parametrize("name", NAMES)
def test_iou_counts_and_keep(data, name):
    from micro_sam_amd import ops
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    other = R.partners(m, name)
    b = _dev_bits(R.with_garbage_tail(R.pack(other), h, seed=11))
    for thr in (0.0, 0.3, 0.5, 0.9, 1.0, 1.01):
        counts, keep = ops.mask_iou_counts(d["bits"], b, h, w, thr)
        want_counts, want_keep = R.iou(m, other, thr)
        assert np.array_equal(counts.cpu().numpy(), want_counts)
        assert np.array_equal(keep.cpu().numpy(), want_keep), thr
    again = ops.mask_iou_counts(d["bits"], b, h, w, 0.5)
    assert torch.equal(again[0], ops.mask_iou_counts(d["bits"], b, h, w, 0.5)[0])


def test_keep_is_not_less_than_at_an_attained_iou():
    """overlap 1, union 2: IoU = 1 / (2 + 1e-7); a threshold of exactly that value keeps the object, the next double above does not."""
    from micro_sam_amd import ops
    h, w = 40, 70
    a = np.zeros((2, h, w), np.uint8); b = np.zeros((2, h, w), np.uint8)
    a[0, 39, 69] = a[0, 0, 0] = 1
    b[0, 39, 69] = 1
    attained = 1.0 / (2.0 + 1e-7)
    ab, bb = _dev_bits(R.pack(a)), _dev_bits(R.pack(b))
    for thr, want in ((attained, [1, 0]), (np.nextafter(attained, 1.0), [0, 0]), (np.nextafter(attained, 0.0), [1, 0]), (0.5, [0, 0]),
                      (0.0, [1, 1]), (float("nan"), [1, 1])):
        counts, keep = ops.mask_iou_counts(ab, bb, h, w, thr)
        assert counts.cpu().tolist() == [[1, 2], [0, 0]] and keep.cpu().tolist() == want, thr


@pytest.mark.parametrize("name", NAMES)
def test_box_prompts_bit_for_bit(data, name):
    from micro_sam_amd import ops
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    for ext in R.BOX_EXTENSIONS:
        nonempty, boxes = ops.mask_box_prompts(d["bits"], h, w, R.input_size((h, w)), ext)
        want_nonempty, want = R.boxes(m, ext)
        assert np.array_equal(nonempty.cpu().numpy(), want_nonempty)
        assert np.array_equal(boxes.cpu().numpy().view(np.uint32), want.view(np.uint32)), ext


@pytest.mark.parametrize("name", NAMES)
def test_mask_logits(data, name):
    from micro_sam_amd import ops
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    values = R.resized64(m)
    fraction = R.tie_band(values).reshape(p, -1).mean(axis=1).max()
    print(f"{name}: largest tie band of a mask {fraction:.2e} of its pixels")
    assert fraction <= R.TIE_BAND_MAX_FRACTION                                            # from the fp64 operator alone
    got = ops.mask_logits(d["bits"], h, w)
    R.check_logits(got.cpu().numpy(), values, name)
    assert torch.equal(got, ops.mask_logits(d["bits"], h, w))


@pytest.mark.parametrize("name", NAMES)
def test_paint_max(data, name):
    from micro_sam_amd import ops
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(np.arange(1, 5000), size=p, replace=False)).astype(np.int32)
    keep = (rng.random(p) < 0.7).astype(np.uint8)
    start = np.where(rng.random((h, w)) < 0.05, 2500, 0).astype(np.int32)
    for k in (keep, None):
        label = torch.from_numpy(start).cuda()
        out = ops.paint_max(d["bits"], torch.from_numpy(ids).cuda(), label, None if k is None else torch.from_numpy(k).cuda())
        assert out is label and np.array_equal(label.cpu().numpy(), R.paint(start, m, ids, k))


def test_wrappers_refuse_what_the_kernels_take_on_trust(data):
    from micro_sam_amd import ops
    d = data("96x160_p14")
    bits = d["bits"]
    ids = torch.arange(1, 15, dtype=torch.int32).cuda()
    label = torch.zeros((96, 160), dtype=torch.int32).cuda()
    with pytest.raises(TypeError, match="bits"):
        ops.mask_logits(bits.float(), 96, 160)
    with pytest.raises(ValueError, match="bits"):
        ops.mask_logits(bits, 128, 160)                                                   # four word rows expected
    with pytest.raises(ValueError, match="bits"):
        ops.mask_logits(bits.cpu(), 96, 160)
    with pytest.raises(ValueError, match="b must"):
        ops.mask_iou_counts(bits, bits[:5], 96, 160, 0.5)
    with pytest.raises(ValueError, match="box_extension"):
        ops.mask_box_prompts(bits, 96, 160, (614, 1024), -1.0)
    with pytest.raises(TypeError, match="ids"):
        ops.paint_max(bits, ids.long(), label)
    with pytest.raises(ValueError, match="keep"):
        ops.paint_max(bits, ids, label, torch.ones(5, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="label"):
        ops.paint_max(bits, ids, label.t())
    with pytest.raises(TypeError, match="masks"):
        ops.pack_bits(torch.zeros((2, 8, 8), dtype=torch.int32).cuda())
    assert ops.mask_logits(bits[:0], 96, 160).shape == (0, 256, 256)
