"""msam_seed_centers (csrc/labelprops.hip, with the component labelling of csrc/segment.hip) compiled for the host
(tests/hip_host_shim.build_library) and driven through the C ABI: N, the flag and the centres integer for integer against the host
function ``instance_segmentation._get_centers`` on the components of ``util._label_equal_value_components``, guard words around every
buffer the library writes, and the refusals.  tests/test_gpu_prompt_seeds.py runs these and larger images on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, f64 = C.c_void_p, C.c_double
GUARD, FILL = 64, -1234567


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_prompt_seeds")), ROOT, files=["labelprops.hip", "segment.hip"])
    lib.msam_seed_centers_workspace_bytes.restype = C.c_int64
    lib.emu_last_error.restype = C.c_char_p
    return lib


class Buf:
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


def run(lib, maps, thresholds=(0.5, 0.5, 0.5), border=1, cap=None, **bad):
    f, c, b = (np.ascontiguousarray(m, np.float32) for m in maps)
    h, w = f.shape
    cap = (h * w + 1) // 2 if cap is None else cap
    need = int(lib.msam_seed_centers_workspace_bytes(h, w, cap))
    assert need == 16 * cap + 13 * h * w + 12 * ((h + 31) // 32) * w + 4 * ((h * w + 4095) // 4096)
    centers, result, ws = Buf(2 * cap), Buf(4), Buf((need + 7) // 8, np.int64)
    a = dict(f=f.ctypes.data_as(vp), c=c.ctypes.data_as(vp), b=b.ctypes.data_as(vp), H=h, W=w, ft=thresholds[0], ct=thresholds[1],
             bt=thresholds[2], border=border, centers=centers.ptr, cap=cap, result=result.ptr, ws=ws.ptr, ws_bytes=need)
    a.update(bad)
    rc = lib.msam_seed_centers(a["f"], a["c"], a["b"], a["H"], a["W"], f64(a["ft"]), f64(a["ct"]), f64(a["bt"]), a["border"], a["centers"],
                               a["cap"], a["result"], a["ws"], C.c_int64(a["ws_bytes"]), None)
    assert centers.intact() and result.intact() and ws.intact()
    return rc, centers, result


def maps_of(seed):
    seed = np.asarray(seed, bool)
    return seed.astype("float32"), (1.0 - seed).astype("float32"), (1.0 - seed).astype("float32")


def field_maps(seed, shape):
    from scipy.ndimage import uniform_filter
    g = np.random.default_rng(seed)

    def field():
        f = np.kron(g.random((shape[0] // 8 + 2, shape[1] // 8 + 2)), np.ones((8, 8)))[:shape[0], :shape[1]]
        return uniform_filter(f, 7).astype("float32")
    return field(), field(), field()


def ties():
    s = np.zeros((40, 50), bool)
    s[39, 47:50] = True
    s[37:40, 49] = True
    s[10:20, 10:20] = True
    return s


def diagonal():
    s = np.zeros((30, 30), bool)
    for k in range(5, 12):
        s[k, 30 - k] = True
    return s


def seam():
    """a rectangle across row 512: the blockwise transform differs from the global one (the centre lies on the seam row)"""
    s = np.zeros((560, 120), bool)
    s[480:550, 10:111] = True
    return s


CASES = {"ties": (maps_of(ties()), (0.5, 0.5, 0.5)), "diagonal": (maps_of(diagonal()), (0.5, 0.5, 0.5)), "seam": (maps_of(seam()), (0.5, 0.5, 0.5)),
         "field 96x70": (field_maps(1, (96, 70)), (0.45, 0.55, 0.55)), "field 130x128": (field_maps(2, (130, 128)), (0.45, 0.55, 0.55)),
         "1x1": (maps_of(np.ones((1, 1), bool)), (0.5, 0.5, 0.5)), "1x37": (maps_of(np.arange(37)[None] % 5 != 2), (0.5, 0.5, 0.5)),
         "41x1": (maps_of(np.arange(41)[:, None] % 7 != 3), (0.5, 0.5, 0.5))}


def expected(maps, thresholds, border):
    from micro_sam_amd import instance_segmentation as IS
    from micro_sam_amd import util
    f, c, b = maps
    ft, ct, bt = (np.float32(t) for t in thresholds)
    seeds = (c < ct) & (b < bt) & ~(f < ft)
    return IS._get_centers(util._label_equal_value_components(seeds.astype("uint32")), avoid_image_border=bool(border)).reshape(-1, 2)


@pytest.mark.parametrize("border", [1, 0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_centres_equal_the_host_function(lib, name, border):
    maps, thr = CASES[name]
    thr = tuple(float(np.float32(t)) for t in thr)
    rc, centers, result = run(lib, maps, thr, border)
    assert rc == 0, lib.emu_last_error().decode()
    n, flag, incomplete, last = result.body.tolist()
    seed_everywhere = bool((maps[1] < 0.5).all())
    if not border and seed_everywhere:                      # no zero pixel at all: undefined, and said so
        assert (n, flag, incomplete, last) == (1, 1, 0, 0)
        return
    want = expected(maps, thr, border)
    assert (n, flag, incomplete, last) == (len(want), 0, 0, 0)
    assert np.array_equal(centers.body[:2 * n].reshape(n, 2), want)
    assert (centers.body[2 * n:] == FILL).all()             # nothing beyond the N rows is written
    if name == "seam" and border:
        assert want.tolist() == [[512, 47]]                 # (a global transform: [[514, 44]])


def test_known_answers(lib):
    for seed, want in ((ties(), [[14, 14], [37, 47]]), (diagonal(), [[k, 30 - k] for k in range(5, 12)])):
        rc, centers, result = run(lib, maps_of(seed))
        assert rc == 0 and result.body[0] == len(want) and centers.body[:2 * len(want)].reshape(-1, 2).tolist() == want


def test_two_runs_are_identical_and_a_small_capacity_is_respected(lib):
    maps, thr = CASES["field 130x128"]
    a, b = run(lib, maps, thr)[1], run(lib, maps, thr)[1]
    assert np.array_equal(a.body, b.body)
    rc, centers, result = run(lib, maps, thr, cap=2)
    assert rc == 0 and result.body[0] > 2 and np.array_equal(centers.body, a.body[:4])


def test_refusals_leave_the_outputs_untouched(lib):
    maps = maps_of(ties())
    need = int(lib.msam_seed_centers_workspace_bytes(40, 50, 1000))
    nan = float("nan")
    for kw in (dict(f=None), dict(c=None), dict(b=None), dict(centers=None), dict(result=None), dict(ws=None), dict(H=0), dict(W=-1),
               dict(H=32768), dict(W=40000), dict(cap=0), dict(ft=nan), dict(ct=nan), dict(bt=nan), dict(border=2), dict(ws_bytes=need - 1)):
        f, c, b = (np.ascontiguousarray(m) for m in maps)
        centers, result, ws = Buf(2000), Buf(4), Buf((need + 7) // 8, np.int64)
        a = dict(f=f.ctypes.data_as(vp), c=c.ctypes.data_as(vp), b=b.ctypes.data_as(vp), H=40, W=50, ft=0.5, ct=0.5, bt=0.5, border=1,
                 centers=centers.ptr, cap=1000, result=result.ptr, ws=ws.ptr, ws_bytes=need)
        a.update(kw)
        rc = lib.msam_seed_centers(a["f"], a["c"], a["b"], a["H"], a["W"], f64(a["ft"]), f64(a["ct"]), f64(a["bt"]), a["border"], a["centers"],
                                   a["cap"], a["result"], a["ws"], C.c_int64(a["ws_bytes"]), None)
        assert rc != 0 and "msam_seed_centers" in lib.emu_last_error().decode(), kw
        assert centers.untouched() and result.untouched() and ws.untouched(), kw
    assert lib.msam_seed_centers_workspace_bytes(0, 5, 1) == 0 and lib.msam_seed_centers_workspace_bytes(5, 32768, 1) == 0
    assert lib.msam_seed_centers_workspace_bytes(5, 5, 0) == 0


def test_the_file_alone_refuses_instead_of_failing_to_load(tmp_path):
    """labelprops.hip compiled on its own (as tests/test_host_labelprops.py does) has no component labelling: the entry says so."""
    alone = build_library(str(tmp_path), ROOT, files=["labelprops.hip"])
    alone.msam_seed_centers_workspace_bytes.restype = C.c_int64
    alone.emu_last_error.restype = C.c_char_p
    rc, centers, result = run(alone, maps_of(ties()))
    assert rc != 0 and "msam_label_components_async" in alone.emu_last_error().decode()
    assert centers.untouched() and result.untouched()
