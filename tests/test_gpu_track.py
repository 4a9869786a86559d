"""ops.mask_moments / ops.mask_shift (csrc/track.hip) on the device: the cases of tests/test_host_track.py through the tensor wrappers,
with the same references (tests/track_ref.py) - the moments exactly against numpy, the shift bit for bit against scipy.ndimage.shift,
garbage in the tail bits of every input wherever H is no multiple of 32, zero tail bits of every output."""
import numpy as np
import pytest
import torch

import track_ref as T

pytestmark = pytest.mark.gpu
IDS = [f"{h}x{w}" for h, w in T.SHAPES]


def _dev(a, dtype=np.int32):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


@pytest.mark.parametrize("shape", T.SHAPES, ids=IDS)
def test_moments_are_exact(shape):
    from micro_sam_amd import ops
    h, w = shape
    m = T.masks(shape, T.CHUNK)
    want = T.moments(m)
    bits = _dev(T.with_garbage_tail(T.pack(m), h))
    got = ops.mask_moments(bits, h, w)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.mask_moments(bits, h, w), got)             # integer atomics: the same bits again
    assert np.array_equal(ops.mask_moments(bits[1:2], h, w).cpu().numpy(), want[1:2])
    rows = got.cpu().numpy()
    for i in np.flatnonzero(want[:, 0] > 0)[:8]:
        assert np.array_equal(T.center_from_moments(rows[i]).view(np.uint64), T.center(m[i]).view(np.uint64))


def test_moments_of_a_full_2049_mask_need_64_bits():
    from micro_sam_amd import ops
    h = w = 2049
    bits = _dev(np.full((1, 65, w), 0xFFFFFFFF, np.uint32))           # the tail bits of the last word row set as well: garbage
    want = [[h * w, w * (h * (h - 1) // 2), h * (w * (w - 1) // 2)]]
    assert want[0][1] > 2 ** 32 and ops.mask_moments(bits, h, w).cpu().tolist() == want


@pytest.mark.parametrize("shape", T.SHAPES, ids=IDS)
def test_shift_equals_scipy_bit_for_bit(shape):
    from micro_sam_amd import ops
    h, w = shape
    if h > 1:
        pairs = T.shift_pairs(shape)
        assert any(T.offset_varies(h, sy) for sy, _ in pairs) and any(T.offset_varies(w, sx) for _, sx in pairs)
    for m, shifts in T.shift_batches(shape):
        bits = _dev(T.with_garbage_tail(T.pack(m), h))
        before = bits.clone()
        out = ops.mask_shift(bits, h, w, _dev(shifts, np.float64))
        assert out.dtype == torch.int32 and out.shape == bits.shape and torch.equal(bits, before)
        got = out.cpu().numpy().view(np.uint32)
        assert T.tail_is_zero(got, h)
        want = T.shift_ref(m, shifts)
        bad = [i for i in range(len(m)) if not np.array_equal(T.unpack(got[i:i + 1], h)[0], want[i])]
        assert not bad, [(i, shifts[i].tolist()) for i in bad[:5]]


def test_wrappers_refuse_what_the_kernels_take_on_trust():
    from micro_sam_amd import ops
    h, w = 33, 65
    bits = _dev(T.pack(T.masks((h, w), 4)))
    shifts = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError, match="shifts"):
        ops.mask_shift(bits, h, w, shifts.float())
    with pytest.raises(ValueError, match="shifts"):
        ops.mask_shift(bits, h, w, shifts[:3])
    with pytest.raises(ValueError, match="shifts"):
        ops.mask_shift(bits, h, w, shifts.cpu())
    with pytest.raises(ValueError, match="bits"):
        ops.mask_moments(bits, 32, w)                                 # one word row expected
    with pytest.raises(TypeError, match="bits"):
        ops.mask_moments(bits.long(), h, w)
    assert ops.mask_shift(bits[:0], h, w, shifts[:0]).shape == (0, 2, w) and ops.mask_moments(bits[:0], h, w).shape == (0, 3)
