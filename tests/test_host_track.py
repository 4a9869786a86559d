"""msam_mask_moments / msam_mask_shift (csrc/track.hip) compiled for the host (tests/hip_host_shim.build_library) and driven through the
C ABI: the moments exactly against numpy, the shift bit for bit against scipy.ndimage.shift (tests/track_ref.py), garbage in the tail
bits of every input, zero tail bits of every output, guard words around every buffer the library writes, and the refusals - each with a
non-zero return, a message that names the entry point, and the outputs untouched.  tests/test_gpu_track.py runs the same cases on the
device."""
import ctypes as C
import os

import numpy as np
import pytest

import track_ref as T
from hip_host_shim import build_library
from test_host_propagate import GUARD, Buf, err, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_track")), ROOT, files=["track.hip"])
    lib.emu_last_error.restype = C.c_char_p
    lib.msam_mask_moments.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    lib.msam_mask_shift.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    return lib


def _moments(lib, bits, p, h, w):
    out = Buf(2 * 3 * p, np.uint32)                                    # int64 [p, 3] between guard words
    assert lib.msam_mask_moments(ptr(bits), p, h, w, out.ptr, None) == 0, err(lib)
    assert out.intact()
    return out.a[GUARD:GUARD + 6 * p].view(np.int64).reshape(p, 3)


@pytest.mark.parametrize("shape", T.SHAPES, ids=[f"{h}x{w}" for h, w in T.SHAPES])
def test_moments_are_exact(lib, shape):
    h, w = shape
    m = T.masks(shape, T.CHUNK)
    assert not m[0].any() and m[1].all() and m[2].sum() == 1 and m[2, h - 1, w - 1] == 1
    want = T.moments(m)
    clean = T.pack(m)
    for bits in (clean, T.with_garbage_tail(clean, h)):
        assert np.array_equal(_moments(lib, bits, len(m), h, w), want)
    assert np.array_equal(_moments(lib, np.ascontiguousarray(clean[1:2]), 1, h, w), want[1:2])          # a call of one object
    for i in np.flatnonzero(want[:, 0] > 0)[:8]:                       # the host's division is np.mean of the index arrays, bit for bit
        assert np.array_equal(T.center_from_moments(want[i]).view(np.uint64), T.center(m[i]).view(np.uint64))


def test_moments_of_a_full_2049_mask_need_64_bits(lib):
    h = w = 2049
    bits = np.full((1, 65, w), 0xFFFFFFFF, np.uint32)                  # the tail bits of the last word row set as well: garbage
    n = h * w
    want = np.array([[n, w * (h * (h - 1) // 2), h * (w * (w - 1) // 2)]], np.int64)
    assert want[0, 1] > 2 ** 32
    assert np.array_equal(_moments(lib, bits, 1, h, w), want)


def test_the_cases_hold_a_shift_whose_offset_is_not_constant():
    """Without one the per-index evaluation is untested: a single integer offset per object would pass."""
    for shape in T.SHAPES[1:]:
        pairs = T.shift_pairs(shape)
        assert any(T.offset_varies(shape[0], sy) for sy, _ in pairs) and any(T.offset_varies(shape[1], sx) for _, sx in pairs), shape
    assert T.offset_varies(300, np.nextafter(0.5, 1.0)) and not T.offset_varies(300, 0.5) and not T.offset_varies(300, 3.25)


def test_the_rule_is_scipy():
    """``T.source`` - the rule as csrc/track.hip states it - against scipy on a ramp, so that the assertion above speaks about scipy."""
    from scipy import ndimage
    for n in (1, 2, 33, 300):
        ramp = np.arange(1, n + 1, dtype=np.float64)
        for s in T.axis_shifts(n):
            got = ndimage.shift(ramp, s, order=0, prefilter=False)
            src = T.source(n, s)
            assert np.array_equal(got, np.where(src >= 0, ramp[np.maximum(src, 0)], 0.0)), (n, s)


@pytest.mark.parametrize("shape", T.SHAPES, ids=[f"{h}x{w}" for h, w in T.SHAPES])
def test_shift_equals_scipy_bit_for_bit(lib, shape):
    h, w = shape
    for m, shifts in T.shift_batches(shape):
        p = len(m)
        bits = T.with_garbage_tail(T.pack(m), h)
        out = Buf(bits.size, np.uint32)
        assert lib.msam_mask_shift(ptr(bits), p, h, w, ptr(shifts), out.ptr, None) == 0, err(lib)
        assert out.intact()
        got = out.body.reshape(bits.shape)
        assert T.tail_is_zero(got, h)
        want = T.shift_ref(m, shifts)
        bad = [i for i in range(p) if not np.array_equal(T.unpack(got[i:i + 1], h)[0], want[i])]
        assert not bad, [(i, shifts[i].tolist()) for i in bad[:5]]
        odd = ~np.isfinite(shifts).all(axis=1)
        assert not want[odd].any()                                     # NaN and the infinities: an empty mask


def test_refusals_leave_the_outputs_untouched(lib):
    h, w, p = 40, 70, 3
    bits = T.pack(np.ones((p, h, w), np.uint8))
    shifts = np.zeros((p, 2), np.float64)
    shapes = (dict(P=0), dict(P=-1), dict(P=65536), dict(H=0), dict(W=0), dict(H=-5), dict(H=32768), dict(W=32768))
    calls = {
        "msam_mask_moments": (lambda a: lib.msam_mask_moments(a["bits"], a["P"], a["H"], a["W"], a["out"], None),
                              (dict(bits=None), dict(out=None))),
        "msam_mask_shift": (lambda a: lib.msam_mask_shift(a["bits"], a["P"], a["H"], a["W"], a["shifts"], a["bits_out"], None),
                            (dict(bits=None), dict(shifts=None), dict(bits_out=None))),
    }
    for entry, (call, faults) in calls.items():
        for kw in faults + shapes:
            o = dict(out=Buf(6 * p, np.uint32), bits_out=Buf(bits.size, np.uint32))
            a = dict(bits=ptr(bits), shifts=ptr(shifts), P=p, H=h, W=w, out=o["out"].ptr, bits_out=o["bits_out"].ptr)
            a.update(kw)
            assert call(a) != 0 and entry in err(lib), (entry, kw, err(lib))
            assert all(b.untouched() for b in o.values()), (entry, kw)
    inplace = Buf(bits.size, np.uint32, init=bits)                     # bits_out == bits_in
    assert lib.msam_mask_shift(inplace.ptr, p, h, w, ptr(shifts), inplace.ptr, None) != 0 and "msam_mask_shift" in err(lib)
    assert inplace.untouched()
