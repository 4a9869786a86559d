"""msam_mask_pack / msam_mask_iou_counts / msam_mask_box_prompts / msam_mask_logits / msam_paint_max (csrc/propagate.hip) compiled for the
host (tests/hip_host_shim.build_library) and driven through the C ABI: every integer output exactly and the boxes bit for bit against
tests/propagate_ref.py, the mask prompts against torch's CPU operator in fp64 outside a tie band of 1e-5 around 0.5, guard words around
every buffer the library writes, and the refusals - each with a non-zero return, a message that names the entry point, and the outputs
untouched.  tests/test_gpu_propagate.py runs the same cases on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import propagate_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
GUARD = 64
HOST_CASES = ["300x200_p70", "96x160_p14", "257x255_p1", "256x256_p3", "512x512_p3", "768x1024_p3"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_propagate")), ROOT, files=["propagate.hip"])
    lib.emu_last_error.restype = C.c_char_p
    lib.msam_mask_pack.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    lib.msam_mask_iou_counts.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, vp, vp, vp]
    lib.msam_mask_box_prompts.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, vp, vp, vp]
    lib.msam_mask_logits.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    lib.msam_paint_max.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    return lib


@pytest.fixture(scope="module")
def data():
    """Per case: the masks, their packed form with garbage in the tail bits, and the fp64 resize - computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            m = R.masks(name)
            cache[name] = dict(masks=m, bits=R.with_garbage_tail(R.pack(m), m.shape[1]), values=None)
        return cache[name]
    return get


class Buf:
    """An output buffer with guard words on both sides, filled with a pattern no result equals."""

    def __init__(self, n, dtype, init=None):
        self.dtype = np.dtype(dtype)
        self.fill = {1: 0xA5, 4: 0x5A5A5A5A}[self.dtype.itemsize]
        raw = np.uint8 if self.dtype.itemsize == 1 else np.uint32
        self.a = np.full(n + 2 * GUARD, self.fill, raw)
        self.n = n
        if init is not None:
            self.a[GUARD:GUARD + n] = np.ascontiguousarray(init).reshape(-1).view(raw)
        self.before = self.a.copy()

    @property
    def ptr(self):
        return vp(self.a.ctypes.data + GUARD * self.a.itemsize)

    @property
    def body(self):
        return self.a[GUARD:GUARD + self.n].view(self.dtype)

    def intact(self):
        return bool((self.a[:GUARD] == self.fill).all() and (self.a[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.a == self.before).all())


def ptr(a):
    return a.ctypes.data_as(vp)


def err(lib):
    return lib.emu_last_error().decode()


@pytest.mark.parametrize("name", HOST_CASES)
def test_pack_sets_the_pixels_that_equal_one(lib, data, name):
    m = data(name)["masks"]
    p, h, w = m.shape
    out = Buf(p * ((h + 31) // 32) * w, np.uint32)
    assert lib.msam_mask_pack(ptr(m), p, h, w, out.ptr, None) == 0, err(lib)
    assert out.intact()
    assert np.array_equal(out.body.reshape(p, -1, w), R.pack(m))                 # tail bits zero


@pytest.mark.parametrize("name", HOST_CASES)
def test_iou_counts_and_keep_flags_are_exact(lib, data, name):
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    other = R.partners(m, name)
    b_bits = R.with_garbage_tail(R.pack(other), h, seed=11)
    for thr in (0.0, 0.3, 0.5, 0.9, 1.0, 1.01):
        counts, keep = Buf(2 * p, np.int32), Buf(p, np.uint8)
        assert lib.msam_mask_iou_counts(ptr(d["bits"]), ptr(b_bits), p, h, w, thr, counts.ptr, keep.ptr, None) == 0, err(lib)
        assert counts.intact() and keep.intact()
        want_counts, want_keep = R.iou(m, other, thr)
        assert np.array_equal(counts.body.reshape(p, 2), want_counts)
        assert np.array_equal(keep.body, want_keep), thr


def test_keep_is_not_less_than_at_an_attained_iou(lib):
    """overlap 1, union 2: the IoU is 1 / (2 + 1e-7).  A threshold of exactly that value keeps the object (``<``, not ``<=``); 0.5, which
    lies just above it, does not; two empty masks have IoU 0 and are kept only by a threshold <= 0."""
    h, w = 40, 70
    a = np.zeros((2, h, w), np.uint8); b = np.zeros((2, h, w), np.uint8)
    a[0, 39, 69] = a[0, 0, 0] = 1
    b[0, 39, 69] = 1
    attained = 1.0 / (2.0 + 1e-7)
    for thr, want in ((attained, [1, 0]), (np.nextafter(attained, 1.0), [0, 0]), (np.nextafter(attained, 0.0), [1, 0]), (0.5, [0, 0]),
                      (0.0, [1, 1]), (-1.0, [1, 1]), (float("nan"), [1, 1])):
        counts, keep = Buf(4, np.int32), Buf(2, np.uint8)
        assert lib.msam_mask_iou_counts(ptr(R.pack(a)), ptr(R.pack(b)), 2, h, w, thr, counts.ptr, keep.ptr, None) == 0
        assert counts.body.tolist() == [1, 2, 0, 0] and keep.body.tolist() == want, thr
        assert R.iou(a, b, thr)[1].tolist() == want


@pytest.mark.parametrize("name", HOST_CASES)
def test_boxes_equal_the_host_chain_bit_for_bit(lib, data, name):
    # (the host build is compiled with -ffp-contract=off throughout, so this test cannot notice a lost "#pragma clang fp contract(off)"
    #  in pr_box_finish_kernel; tests/test_gpu_propagate.py::test_box_prompts_bit_for_bit pins it on the device build)
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    ih, iw = R.input_size((h, w))
    for ext in R.BOX_EXTENSIONS:
        boxes, nonempty = Buf(4 * p, np.float32), Buf(p, np.uint8)
        assert lib.msam_mask_box_prompts(ptr(d["bits"]), p, h, w, ext, ih, iw, boxes.ptr, nonempty.ptr, None) == 0, err(lib)
        assert boxes.intact() and nonempty.intact()
        want_nonempty, want = R.boxes(m, ext)
        assert np.array_equal(nonempty.body, want_nonempty)
        assert np.array_equal(boxes.body.view(np.uint32).reshape(p, 4), want.view(np.uint32)), ext


def test_half_pixel_extension_rounds_half_to_even(lib):
    """A side of 20 pixels at 0.025 extends by exactly 0.5: 6.5 -> 6, 27.5 -> 28 (image frame; 1024 / 160 = 6.4 to the input frame)."""
    m = R.masks("96x160_p14")[10:11]
    nonempty, want = R.boxes(m, 0.025)
    assert (want / np.float32(6.4)).round().tolist() == [[6.0, 64.0, 28.0, 86.0]]
    boxes, flag = Buf(4, np.float32), Buf(1, np.uint8)
    assert lib.msam_mask_box_prompts(ptr(R.pack(m)), 1, 96, 160, 0.025, 614, 1024, boxes.ptr, flag.ptr, None) == 0
    assert np.array_equal(boxes.body.reshape(1, 4), want) and flag.body.tolist() == [1]


@pytest.mark.parametrize("name", HOST_CASES)
def test_logits_equal_the_fp64_operator_outside_the_tie_band(lib, data, name):
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    values = R.resized64(m)
    band = R.tie_band(values)
    assert band.reshape(p, -1).mean(axis=1).max() <= R.TIE_BAND_MAX_FRACTION          # from the fp64 operator alone
    out = Buf(p * 256 * 256, np.float32)
    assert lib.msam_mask_logits(ptr(d["bits"]), p, h, w, out.ptr, None) == 0, err(lib)
    assert out.intact()
    R.check_logits(out.body.reshape(p, 256, 256), values, name)
    R.check_logits(R.host_logits(m), values, name + " (host fp32)")               # the package's own host function obeys the same rule


@pytest.mark.parametrize("name", HOST_CASES)
def test_paint_max_composes_like_ascending_assignment(lib, data, name):
    d = data(name)
    m = d["masks"]
    p, h, w = m.shape
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(np.arange(1, 5000), size=p, replace=False)).astype(np.int32)
    keep = (rng.random(p) < 0.7).astype(np.uint8)
    start = np.where(rng.random((h, w)) < 0.05, 2500, 0).astype(np.int32)
    for k in (keep, None):
        label = Buf(h * w, np.int32, init=start)
        assert lib.msam_paint_max(ptr(d["bits"]), ptr(ids), None if k is None else ptr(k), p, h, w, label.ptr, None) == 0, err(lib)
        assert label.intact()
        assert np.array_equal(label.body.reshape(h, w), R.paint(start, m, ids, k))


def test_two_runs_are_identical(lib, data):
    d = data("300x200_p70")
    p, h, w = d["masks"].shape
    runs = []
    for _ in range(2):
        counts, keep, logits = Buf(2 * p, np.int32), Buf(p, np.uint8), Buf(p * 65536, np.float32)
        assert lib.msam_mask_iou_counts(ptr(d["bits"]), ptr(np.roll(d["bits"], 3, axis=2).copy()), p, h, w, 0.5, counts.ptr, keep.ptr, None) == 0
        assert lib.msam_mask_logits(ptr(d["bits"]), p, h, w, logits.ptr, None) == 0
        runs.append((counts.body.copy(), keep.body.copy(), logits.body.view(np.uint32).copy()))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def test_refusals_leave_the_outputs_untouched(lib):
    h, w, p = 40, 70, 3
    m = np.ones((p, h, w), np.uint8)
    bits = R.pack(m)
    ids = np.array([1, 2, 3], np.int32)
    shapes = (dict(P=0), dict(P=-1), dict(P=65536), dict(H=0), dict(W=0), dict(H=-5), dict(H=32768), dict(W=32768))

    def outputs():
        return dict(bits=Buf(p * 2 * w, np.uint32), counts=Buf(2 * p, np.int32), keep=Buf(p, np.uint8), boxes=Buf(4 * p, np.float32),
                    nonempty=Buf(p, np.uint8), logits=Buf(p * 65536, np.float32), label=Buf(h * w, np.int32, init=np.zeros(h * w, np.int32)))

    calls = {
        "msam_mask_pack": (lambda a, o: lib.msam_mask_pack(a["masks"], a["P"], a["H"], a["W"], a["bits_out"], None),
                           (dict(masks=None), dict(bits_out=None))),
        "msam_mask_iou_counts": (lambda a, o: lib.msam_mask_iou_counts(a["a"], a["b"], a["P"], a["H"], a["W"], 0.5, a["counts"], a["keep"], None),
                                 (dict(a=None), dict(b=None), dict(counts=None), dict(keep=None))),
        "msam_mask_box_prompts": (lambda a, o: lib.msam_mask_box_prompts(a["a"], a["P"], a["H"], a["W"], a["ext"], a["ih"], a["iw"], a["boxes"],
                                                                         a["nonempty"], None),
                                  (dict(a=None), dict(boxes=None), dict(nonempty=None), dict(ext=-0.1), dict(ext=float("nan")),
                                   dict(ext=float("inf")), dict(ih=0), dict(iw=-3))),
        "msam_mask_logits": (lambda a, o: lib.msam_mask_logits(a["a"], a["P"], a["H"], a["W"], a["logits"], None),
                             (dict(a=None), dict(logits=None), dict(H=1, W=32767))),
        "msam_paint_max": (lambda a, o: lib.msam_paint_max(a["a"], a["ids"], a["keep_in"], a["P"], a["H"], a["W"], a["label"], None),
                           (dict(a=None), dict(ids=None), dict(label=None))),
    }
    for entry, (call, faults) in calls.items():
        for kw in faults + shapes:
            o = outputs()
            a = dict(masks=ptr(m), a=ptr(bits), b=ptr(bits), ids=ptr(ids), keep_in=None, P=p, H=h, W=w, ext=0.0, ih=585, iw=1024,
                     bits_out=o["bits"].ptr, counts=o["counts"].ptr, keep=o["keep"].ptr, boxes=o["boxes"].ptr, nonempty=o["nonempty"].ptr,
                     logits=o["logits"].ptr, label=o["label"].ptr)
            a.update(kw)
            rc = call(a, o)
            assert rc != 0 and entry in err(lib), (entry, kw, err(lib))
            assert all(b.untouched() for b in o.values()), (entry, kw)
