"""csrc/merge3d.hip compiled for the host (tests/hip_host_shim.build_library) and driven through the C ABI: msam_close_gaps integer for
integer against ``multi_dimensional_segmentation._preprocess_closing`` on the volumes of tests/merge3d_cases.py, msam_label_z_ranges and
msam_apply_label_lut against numpy, guard words around every buffer the library writes, and the refusals.  tests/test_gpu_merge3d.py
runs the same cases on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from hip_host_shim import build_library
import merge3d_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 64, -1234567


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_merge3d")), ROOT, files=["merge3d.hip"])
    lib.msam_close_gaps_workspace_bytes.restype = C.c_int64
    lib.emu_last_error.restype = C.c_char_p
    return lib


class Guarded:
    """An int32 buffer between guard words."""

    def __init__(self, n):
        self.raw = np.full(n + 2 * GUARD, FILL, np.int32)
        self.body = self.raw[GUARD:GUARD + n]

    @property
    def ptr(self):
        return C.c_void_p(self.body.ctypes.data)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == FILL).all() and (self.raw[GUARD + len(self.body):] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def close_gaps(lib, labels, gap, id_limit=None):
    labels = np.ascontiguousarray(labels, np.int32)
    Z, H, W = labels.shape
    id_limit = int(labels.max()) + 1 if id_limit is None else id_limit
    nbytes = lib.msam_close_gaps_workspace_bytes(Z, H, W, gap, id_limit)
    assert nbytes > 0 and nbytes % 4 == 0
    out, result, ws = Guarded(labels.size), Guarded(4), Guarded(nbytes // 4)
    rc = lib.msam_close_gaps(_ptr(labels), Z, H, W, gap, id_limit, out.ptr, result.ptr, ws.ptr, C.c_int64(nbytes), None)
    assert rc == 0, lib.emu_last_error().decode()
    assert out.guards_intact() and result.guards_intact() and ws.guards_intact()
    return out.body.reshape(labels.shape).copy(), result.body.copy()


CASES = {name: (vol, gap) for name, vol, gap in MC.cases()}


def test_the_case_list_is_complete():
    assert list(CASES) == MC.CASE_NAMES


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_close_gaps_equals_the_host_function(lib, name):
    vol, gap = CASES[name]
    ref, offset = MC.host_close(vol, gap)
    got, result = close_gaps(lib, vol, gap)
    assert result.tolist() == [offset, 0, 0, 0]
    assert np.array_equal(got, ref), (name, np.argwhere(got != ref)[:5], got[got != ref][:5], ref[got != ref][:5])
    again, result2 = close_gaps(lib, vol, gap, id_limit=int(vol.max()) + 77)      # a looser id limit: the same volume
    assert np.array_equal(again, got) and result2.tolist() == result.tolist()


def test_the_cases_exercise_what_they_are_meant_to():
    """The yardstick itself shows the properties the cases are built for."""
    from micro_sam_amd.multi_dimensional_segmentation import _check_ids_unique_per_slice, _preprocess_closing
    from scipy import ndimage
    wide, _ = CASES["wide_gap1"]
    first = {int(v): int(np.flatnonzero(wide[1].reshape(-1) == v)[0]) for v in np.unique(wide[1]) if v}
    a, b = sorted(first, key=first.get)[:2]
    assert first[a] % 600 >= 512 and first[b] % 600 < 512                       # raster order: the component beyond column 512 comes first
    vol, _ = CASES["painting_order"]
    out = _preprocess_closing(vol, 1)
    assert len(np.unique(out[2][vol[2] == 22])) == 1 and len(np.unique(out[2][vol[2] == 24])) == 1
    assert out[2][vol[2] == 22][0] != out[2][vol[2] == 23][0]
    assert (out[2][10:31, 5:41][vol[2][10:31, 5:41] == 0] == 0).all()           # the merging component itself is not painted
    n4 = ndimage.label(CASES["diagonal"][0][1] > 0)[1]
    n8 = ndimage.label(CASES["diagonal"][0][1] > 0, structure=np.ones((3, 3)))[1]
    assert (n4, n8) == (3, 1)
    vol, _ = CASES["bridged"]
    out = _preprocess_closing(vol, 1)
    assert (out[1][4:9, 3:8] > 0).all() and (vol[1][4:9, 3:8] == 0).all()
    vol, gap = CASES["reset"]
    out = _preprocess_closing(vol, gap)
    assert out[2].min() == 0 and set(np.unique(out[2])) & set(np.unique(out[0])) - {0}
    with pytest.raises(ValueError):
        _check_ids_unique_per_slice(out)


def test_a_label_outside_the_range_is_reported(lib):
    vol = CASES["bridged"][0].copy()
    vol[1, 0, 0] = -3
    _, result = close_gaps(lib, vol, 1)
    assert result[1] == 1 and result[2] == 0
    vol[1, 0, 0] = 50
    _, result = close_gaps(lib, vol, 1, id_limit=10)
    assert result[1] == 2


def test_refusals_leave_everything_untouched(lib):
    vol = np.ascontiguousarray(CASES["bridged"][0])
    Z, H, W = vol.shape
    nbytes = lib.msam_close_gaps_workspace_bytes(Z, H, W, 1, 5)
    out, result, ws = Guarded(vol.size), Guarded(4), Guarded(nbytes // 4)
    base = dict(labels=_ptr(vol), Z=Z, H=H, W=W, gap=1, lim=5, out=out.ptr, result=result.ptr, ws=ws.ptr, nbytes=nbytes)
    for kw in (dict(labels=None), dict(out=None), dict(result=None), dict(ws=None), dict(Z=0), dict(H=0), dict(W=-1), dict(gap=0),
               dict(lim=0), dict(nbytes=nbytes - 4), dict(out=_ptr(vol)), dict(ws=C.c_void_p(ws.body.ctypes.data + 2))):
        a = dict(base)
        a.update(kw)
        rc = lib.msam_close_gaps(a["labels"], a["Z"], a["H"], a["W"], a["gap"], a["lim"], a["out"], a["result"], a["ws"],
                                 C.c_int64(a["nbytes"]), None)
        assert rc != 0 and "msam_close_gaps" in lib.emu_last_error().decode(), kw
        assert out.untouched() and result.untouched() and ws.untouched(), kw
    assert lib.msam_close_gaps_workspace_bytes(0, 4, 4, 1, 5) == 0 and lib.msam_close_gaps_workspace_bytes(2, 4, 4, 0, 5) == 0
    assert lib.msam_close_gaps_workspace_bytes(2, 4, 4, 1, 0) == 0 and lib.msam_close_gaps_workspace_bytes(2, 65536, 65536, 1, 5) == 0
    zr, flag = Guarded(10), Guarded(1)
    for args in ((None, Z, H, W, 5, zr.ptr, flag.ptr), (_ptr(vol), 0, H, W, 5, zr.ptr, flag.ptr), (_ptr(vol), Z, H, W, 0, zr.ptr, flag.ptr),
                 (_ptr(vol), Z, H, W, 5, None, flag.ptr), (_ptr(vol), Z, H, W, 5, zr.ptr, None)):
        assert lib.msam_label_z_ranges(*args, None) != 0 and "msam_label_z_ranges" in lib.emu_last_error().decode()
        assert zr.untouched() and flag.untouched()
    lut = np.arange(5, dtype=np.int32)
    for args in ((None, C.c_int64(vol.size), _ptr(lut), 5, out.ptr, flag.ptr), (_ptr(vol), C.c_int64(0), _ptr(lut), 5, out.ptr, flag.ptr),
                 (_ptr(vol), C.c_int64(vol.size), None, 5, out.ptr, flag.ptr), (_ptr(vol), C.c_int64(vol.size), _ptr(lut), 0, out.ptr, flag.ptr),
                 (_ptr(vol), C.c_int64(vol.size), _ptr(lut), 5, None, flag.ptr), (_ptr(vol), C.c_int64(vol.size), _ptr(lut), 5, out.ptr, None)):
        assert lib.msam_apply_label_lut(*args, None) != 0 and "msam_apply_label_lut" in lib.emu_last_error().decode()
        assert out.untouched() and flag.untouched()


def test_label_z_ranges(lib):
    vol = CASES["repeating_ids"][0].copy()
    vol[0, 0, 0] = vol[3, 23, 29] = 33                       # slices 0 and Z - 1 only
    Z, H, W = vol.shape
    n_ids = 45                                                # ids 41..44 and most below never occur
    zr, flag = Guarded(2 * n_ids), Guarded(1)
    assert lib.msam_label_z_ranges(_ptr(vol), Z, H, W, n_ids, zr.ptr, flag.ptr, None) == 0, lib.emu_last_error().decode()
    assert zr.guards_intact() and flag.guards_intact() and flag.body[0] == 0
    got = zr.body.reshape(n_ids, 2)
    assert np.array_equal(got, MC.z_ranges_ref(vol, n_ids))
    assert got[33].tolist() == [0, 3] and got[40].tolist() == [0, 3] and got[0].tolist() == [Z, -1] and got[44].tolist() == [Z, -1]
    assert lib.msam_label_z_ranges(_ptr(vol), Z, H, W, 34, zr.ptr, flag.ptr, None) == 0           # id 40 is out of range now
    assert flag.body[0] == 1 and np.array_equal(zr.body[:68].reshape(34, 2), MC.z_ranges_ref(vol, 34))


def test_apply_label_lut(lib):
    rng = np.random.default_rng(0)
    vol = rng.integers(0, 50, (3, 17, 19)).astype(np.int32)
    lut = rng.integers(0, 1000, 50).astype(np.int32)
    out, flag = Guarded(vol.size), Guarded(1)
    assert lib.msam_apply_label_lut(_ptr(vol), C.c_int64(vol.size), _ptr(lut), 50, out.ptr, flag.ptr, None) == 0
    assert out.guards_intact() and flag.body[0] == 0 and np.array_equal(out.body.reshape(vol.shape), lut[vol])
    assert lib.msam_apply_label_lut(_ptr(vol), C.c_int64(vol.size), _ptr(lut), 40, out.ptr, flag.ptr, None) == 0
    assert flag.body[0] == 1 and np.array_equal(out.body.reshape(vol.shape), np.where(vol < 40, lut[np.minimum(vol, 39)], 0))
    bad = vol.copy()
    bad[1, 2, 3] = -1
    assert lib.msam_apply_label_lut(_ptr(bad), C.c_int64(vol.size), _ptr(lut), 50, out.ptr, flag.ptr, None) == 0
    assert flag.body[0] == 1 and out.body.reshape(vol.shape)[1, 2, 3] == 0
    inplace = vol.copy()                                      # in place
    assert lib.msam_apply_label_lut(_ptr(inplace), C.c_int64(vol.size), _ptr(lut), 50, _ptr(inplace), flag.ptr, None) == 0
    assert flag.body[0] == 0 and np.array_equal(inplace, lut[vol])
