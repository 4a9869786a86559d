"""msam_edt_squared / msam_label_props (csrc/labelprops.hip) compiled for the host (tests/hip_host_shim.build_library) and driven through
the C ABI: every output integer for integer against tests/labelprops_ref.py, guard words around every buffer the library writes, and
the refusals - each with a non-zero return, a message that names the entry point, and the outputs untouched.
tests/test_gpu_labelprops.py runs the same label images on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import labelprops_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
GUARD, FILL = 64, -1234567
CASES, MASKS = R.cases(), R.edt_masks()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_labelprops")), ROOT, files=["labelprops.hip"])
    lib.msam_edt_squared_workspace_bytes.restype = C.c_int64
    lib.msam_label_props_workspace_bytes.restype = C.c_int64
    lib.emu_last_error.restype = C.c_char_p
    return lib


class Buf:
    """An int32 / int64 buffer with guard words on both sides."""

    def __init__(self, n, dtype=np.int32):
        self.a = np.full(n + 2 * GUARD, FILL, dtype)
        self.n = n

    @property
    def ptr(self):
        return vp(self.a.ctypes.data + GUARD * self.a.itemsize)

    @property
    def body(self):
        return self.a[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.a[:GUARD] == FILL).all() and (self.a[GUARD + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.a == FILL).all())


def run_edt(lib, mask, ws_bytes=None):
    mask = np.ascontiguousarray(mask)
    h, w = mask.shape
    need = int(lib.msam_edt_squared_workspace_bytes(h, w))
    assert need == 4 * h * w + 12 * ((h + 31) // 32) * w
    out, ws = Buf(h * w), Buf(need // 4)
    rc = lib.msam_edt_squared(mask.ctypes.data_as(vp), int(mask.dtype == np.int32), h, w, out.ptr, ws.ptr,
                              C.c_int64(need if ws_bytes is None else ws_bytes), None)
    assert out.intact() and ws.intact()
    return rc, out.body.reshape(h, w).astype(np.int64), out


def run_props(lib, seg, ids, centers=True):
    seg = np.ascontiguousarray(seg, np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    h, w = seg.shape
    n = len(ids)
    need = int(lib.msam_label_props_workspace_bytes(h, w, n))
    assert need == 12 * h * w + 8 * n + 16 + 12 * ((h + 31) // 32) * w
    bufs = {"area": Buf(n), "bbox": Buf(4 * n), "coord_sum": Buf(2 * n, np.int64), "center": Buf(2 * n), "ws": Buf(need // 4)}
    rc = lib.msam_label_props(seg.ctypes.data_as(vp), h, w, ids.ctypes.data_as(vp), n, bufs["area"].ptr, bufs["bbox"].ptr,
                              bufs["coord_sum"].ptr, bufs["center"].ptr if centers else None, bufs["ws"].ptr, C.c_int64(need), None)
    assert all(b.intact() for b in bufs.values())
    return rc, bufs


def same_props(bufs, want, centers=True):
    n = len(want["ids"])
    assert np.array_equal(bufs["area"].body, want["area"])
    assert np.array_equal(bufs["bbox"].body.reshape(n, 4), want["bbox"])
    assert np.array_equal(bufs["coord_sum"].body.reshape(n, 2), want["coord_sum"])
    if centers:
        assert np.array_equal(bufs["center"].body.reshape(n, 2), want["center"])
    else:
        assert bufs["center"].untouched()


@pytest.mark.parametrize("name", sorted(MASKS))
def test_edt_squared_is_exact(lib, name):
    mask = MASKS[name]
    want = R.edt_squared(mask)
    if max(mask.shape) <= 48:
        assert np.array_equal(want, R.edt_squared_brute(mask))
    for m in (mask, mask.astype(np.int32) * 77):
        rc, got, _ = run_edt(lib, m)
        assert rc == 0, lib.emu_last_error().decode()
        assert np.array_equal(got, want)


def test_edt_of_a_mask_without_zero_is_int32_max(lib):
    rc, got, _ = run_edt(lib, MASKS["no_zero"])
    assert rc == 0 and (got == 2 ** 31 - 1).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_label_props_equal_the_restatement(lib, name):
    seg, ids = CASES[name]
    want = R.label_props(seg, ids)
    rc, bufs = run_props(lib, seg, want["ids"])
    assert rc == 0, lib.emu_last_error().decode()
    same_props(bufs, want)


def test_the_restatement_agrees_with_the_brute_force_distance():
    """The reference's float arg-max and an integer arg-max over the brute-force squared distances name the same pixels."""
    for name in ("ring", "c", "bar", "single_pixels", "big_ids"):
        seg, _ = CASES[name]
        if max(seg.shape) > 46:
            seg = seg[:46, :46]
        want = R.label_props(seg)
        d2 = R.edt_squared_brute(R.inner_boundaries(seg) == 0)[1:-1, 1:-1]
        for k, i in enumerate(want["ids"]):
            score = np.where(seg == i, d2, -1).reshape(-1)
            assert tuple(want["center"][k]) == divmod(int(score.argmax()), seg.shape[1])


def test_shapes_of_the_concave_objects():
    """"v" lies inside the object, the centroid outside; in the bars the first pixel in raster order wins the tie."""
    for name in ("ring", "c"):
        seg, _ = CASES[name]
        want = R.label_props(seg)
        cy, cx = want["center"][0]
        assert seg[cy, cx] != 0
        py, px = np.rint(want["centroid"][0]).astype(int)
        assert seg[py, px] == 0
    want = R.label_props(CASES["bar"][0])
    assert want["center"].tolist() == [[3, 4], [7, 1]]


def test_without_centres_no_distance_is_computed(lib):
    seg, _ = CASES["33x65"]
    want = R.label_props(seg)
    rc, bufs = run_props(lib, seg, want["ids"], centers=False)
    assert rc == 0
    same_props(bufs, want, centers=False)


def test_two_runs_are_identical(lib):
    seg, _ = CASES["130x257"]
    ids = R.label_props(seg)["ids"]
    a, b = run_props(lib, seg, ids)[1], run_props(lib, seg, ids)[1]
    assert all(np.array_equal(a[k].body, b[k].body) for k in ("area", "bbox", "coord_sum", "center"))


def test_refusals_leave_the_outputs_untouched(lib):
    seg = np.ascontiguousarray(CASES["33x65"][0], np.int32)
    ids = np.array([1, 2, 5], np.int32)
    h, w = seg.shape
    need = int(lib.msam_label_props_workspace_bytes(h, w, 3))
    base = dict(labels=seg.ctypes.data_as(vp), H=h, W=w, ids=ids.ctypes.data_as(vp), N=3, ws_bytes=need)
    unsorted, dup, zero = np.array([2, 1, 5], np.int32), np.array([1, 2, 2], np.int32), np.array([0, 1, 2], np.int32)
    for kw in (dict(labels=None), dict(ids=None), dict(area=None), dict(bbox=None), dict(coord_sum=None), dict(ws=None),
               dict(H=0), dict(W=0), dict(H=-3), dict(H=32768), dict(W=32768), dict(N=0), dict(ws_bytes=need - 1),
               dict(ids=unsorted.ctypes.data_as(vp)), dict(ids=dup.ctypes.data_as(vp)), dict(ids=zero.ctypes.data_as(vp))):
        bufs = {"area": Buf(3), "bbox": Buf(12), "coord_sum": Buf(6, np.int64), "center": Buf(6), "ws": Buf(need // 4)}
        a = dict(base, **{k: b.ptr for k, b in bufs.items()})
        a.update(kw)
        rc = lib.msam_label_props(a["labels"], a["H"], a["W"], a["ids"], a["N"], a["area"], a["bbox"], a["coord_sum"], a["center"], a["ws"],
                                  C.c_int64(a["ws_bytes"]), None)
        msg = lib.emu_last_error().decode()
        assert rc != 0 and "msam_label_props" in msg, kw
        assert all(bufs[k].untouched() for k in ("area", "bbox", "coord_sum", "center")), kw
    assert lib.msam_label_props_workspace_bytes(0, 5, 1) == 0 and lib.msam_label_props_workspace_bytes(5, 32768, 1) == 0
    assert lib.msam_label_props_workspace_bytes(5, 5, 0) == 0

    mask = np.ones((6, 7), np.uint8)
    need = int(lib.msam_edt_squared_workspace_bytes(6, 7))
    base = dict(mask=mask.ctypes.data_as(vp), kind=0, H=6, W=7, ws_bytes=need)
    for kw in (dict(mask=None), dict(out=None), dict(ws=None), dict(H=0), dict(W=-1), dict(H=32768), dict(W=40000), dict(kind=2),
               dict(ws_bytes=need - 1)):
        out, ws = Buf(42), Buf(need // 4)
        a = dict(base, out=out.ptr, ws=ws.ptr)
        a.update(kw)
        rc = lib.msam_edt_squared(a["mask"], a["kind"], a["H"], a["W"], a["out"], a["ws"], C.c_int64(a["ws_bytes"]), None)
        assert rc != 0 and "msam_edt_squared" in lib.emu_last_error().decode(), kw
        assert out.untouched() and ws.untouched(), kw
    assert lib.msam_edt_squared_workspace_bytes(0, 7) == 0 and lib.msam_edt_squared_workspace_bytes(32768, 7) == 0
