"""msam_distance_targets (csrc/labelprops.hip) compiled for the host (tests/hip_host_shim.build_library) and driven through the C ABI
against tests/distance_targets_ref.py - the per-object crop form of torch_em's PerObjectDistanceTransform, so that the library's one
distance transform for all objects is what gets tested: the integer tables exactly, the three planes within 1e-6, guard words around
every buffer, the refusals.  Then, still without a device: the channel order and flags of ``PerObjectDistanceTransform`` (its device
call replaced by the host library) and ``DiceBasedDistanceLoss`` against a closed form and ``torch.autograd.gradcheck``.
tests/test_gpu_distance_targets.py runs the same label images on the device.

The bound on the planes: they lie in [0, 1] (or equal ``fill``) and come from exact integers below 2^24 through at most four fp32
roundings of at most 2^-24 relative each (square root, the sum with 1e-7, the division, the subtraction from 1) - below 4 * 2^-24 =
2.4e-7 in all, next to float64 rounding of the restatement; 1e-6 leaves a factor of four."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import distance_targets_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
GUARD, FILL = 64, -1234567
TOL = 1e-6
CASES = R.cases()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_distance_targets")), ROOT, files=["labelprops.hip"])
    lib.msam_distance_targets_workspace_bytes.restype = C.c_int64
    lib.emu_last_error.restype = C.c_char_p
    return lib


class Buf:
    """A buffer with guard words on both sides; ``shift`` moves the body by that many elements (to leave 16-byte alignment)."""

    def __init__(self, n, dtype=np.int32, shift=0):
        self.a = np.full(n + 2 * GUARD + 8, FILL, dtype)
        isz = self.a.itemsize
        pad = (-(self.a.ctypes.data + GUARD * isz) % 16) // isz         # elements up to the next 16-byte boundary
        self.n, self.off = n, GUARD + pad + shift

    @property
    def ptr(self):
        return vp(self.a.ctypes.data + self.off * self.a.itemsize)

    @property
    def body(self):
        return self.a[self.off:self.off + self.n]

    def intact(self):
        return bool((self.a[:self.off] == FILL).all() and (self.a[self.off + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.a == FILL).all())


def expected_bytes(h, w, n):
    return (8 * h * w + 15) // 16 * 16 + 44 * n + 12 * ((h + 31) // 32) * w


def run(lib, labels, n, fill=1.0, correct=1, shift=0):
    """``shift``: move labels and out off their 16-byte alignment (the library then takes its one-pixel-per-thread form)."""
    labels = np.ascontiguousarray(labels, np.int32)
    h, w = labels.shape
    need = int(lib.msam_distance_targets_workspace_bytes(h, w, n))
    assert need == expected_bytes(h, w, n)
    lab = Buf(h * w, shift=shift)
    lab.body[:] = labels.reshape(-1)
    bufs = {"out": Buf(3 * h * w, np.float32, shift=shift), "center": Buf(2 * n), "dmax2": Buf(n), "bbox": Buf(4 * n), "ws": Buf(need // 4)}
    rc = lib.msam_distance_targets(lab.ptr, h, w, n, correct, C.c_float(fill), bufs["out"].ptr, bufs["center"].ptr, bufs["dmax2"].ptr,
                                   bufs["bbox"].ptr, bufs["ws"].ptr, C.c_int64(need), None)
    assert lab.intact() and np.array_equal(lab.body, labels.reshape(-1))
    assert all(b.intact() for b in bufs.values())
    return rc, bufs


def same(bufs, want, shape):
    n = len(want["dmax2"])
    assert np.array_equal(bufs["center"].body.reshape(n, 2), want["center"])
    assert np.array_equal(bufs["dmax2"].body, want["dmax2"])
    assert np.array_equal(bufs["bbox"].body.reshape(n, 4), want["bbox"])
    got = bufs["out"].body.reshape(3, *shape).astype(np.float64)
    assert np.array_equal(got[0], want["out"][0])
    err = np.abs(got - want["out"]).max(axis=(1, 2))
    assert (err <= TOL).all(), err


@pytest.mark.parametrize("name", sorted(CASES))
def test_targets_equal_the_per_object_restatement(lib, name):
    labels, n = CASES[name]
    want = R.distance_targets(labels, n)
    rc, bufs = run(lib, labels, n)
    assert rc == 0, lib.emu_last_error().decode()
    same(bufs, want, labels.shape)
    got = bufs["out"].body.reshape(3, *labels.shape)
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_the_cases_are_what_they_are_for():
    """The properties the cases were chosen for hold in the restatement."""
    for name in ("full", "1x1"):
        labels, n = CASES[name]
        assert not R.find_boundaries_inner(labels).any()
        want = R.distance_targets(labels, n)
        assert want["dmax2"].tolist() == [0] and (want["out"][2] == 1.0).all()
    for name in ("ring", "c"):
        labels, n = CASES[name]
        ys, xs = np.nonzero(labels == 1)
        assert labels[int(np.round(ys.mean())), int(np.round(xs.mean()))] == 0          # the centroid lies outside
        cy, cx = R.distance_targets(labels, n)["center"][0]
        assert labels[cy, cx] == 1
        assert tuple(R.distance_targets(labels, n, correct_centers=False)["center"][0]) == (int(np.round(ys.mean())), int(np.round(xs.mean())))
    halves = 0
    for name in ("1x7", "bar", "big_ids"):
        labels, n = CASES[name]
        for o in range(1, n + 1):
            ys, xs = np.nonzero(labels == o)
            halves += int((2 * ys.sum()) % len(ys) == 0 and (2 * ys.sum() // len(ys)) % 2 == 1)
            halves += int((2 * xs.sum()) % len(xs) == 0 and (2 * xs.sum() // len(xs)) % 2 == 1)
    assert halves >= 3                                                                  # centroid coordinates at exactly .5
    for name in ("bar", "single_pixels"):
        labels, n = CASES[name]
        assert (R.distance_targets(labels, n)["dmax2"] == 0).any()
    assert CASES["checkerboard"][1] == 2048
    labels, n = CASES["out_of_range"]
    assert labels.max() > n and labels.min() < 0


def test_the_global_transform_is_the_per_object_one():
    """The claim under the shortcut, on the restatement alone: on every object pixel the distance to the nearest boundary pixel of the
    whole image equals the distance inside the object's bounding-box crop."""
    for name, (labels, n) in CASES.items():
        lab = np.where((labels >= 1) & (labels <= n), labels, 0)
        b = R.find_boundaries_inner(lab)
        if not b.any():
            continue
        d2 = R.LR.edt_squared(~b)
        want = R.distance_targets(labels, n)
        for o in range(1, n + 1):
            if (lab == o).any():
                assert int(d2[lab == o].max()) == int(want["dmax2"][o - 1]), (name, o)


def test_unaligned_buffers_take_the_narrow_form_with_the_same_result(lib):
    labels, n = CASES["64x64"]                                          # 4096 pixels: aligned buffers take four pixels per thread
    a, b = run(lib, labels, n)[1], run(lib, labels, n, shift=1)[1]
    assert all(np.array_equal(a[k].body, b[k].body) for k in ("out", "center", "dmax2", "bbox"))


def test_flags_fill_and_centres_without_correction(lib):
    labels, n = CASES["c"]
    rc, bufs = run(lib, labels, n, fill=-3.5, correct=0)
    assert rc == 0
    same(bufs, R.distance_targets(labels, n, fill=-3.5, correct_centers=False), labels.shape)
    cy, cx = bufs["center"].body
    assert labels[cy, cx] == 0


def test_no_objects_writes_background_everywhere(lib):
    labels = np.array([[0, 3, -1], [7, 0, 0]], np.int32)
    rc, bufs = run(lib, labels, 0, fill=0.25)
    assert rc == 0
    out = bufs["out"].body.reshape(3, 2, 3)
    assert (out[0] == 0).all() and (out[1:] == 0.25).all()


def test_two_runs_are_identical(lib):
    labels, n = CASES["130x257"]
    a, b = run(lib, labels, n)[1], run(lib, labels, n)[1]
    assert all(np.array_equal(a[k].body, b[k].body) for k in ("out", "center", "dmax2", "bbox"))


def test_refusals_leave_the_outputs_untouched(lib):
    labels = np.ascontiguousarray(CASES["33x65"][0], np.int32)
    n = CASES["33x65"][1]
    h, w = labels.shape
    need = int(lib.msam_distance_targets_workspace_bytes(h, w, n))
    base = dict(labels=labels.ctypes.data_as(vp), H=h, W=w, N=n, correct=1, ws_bytes=need)
    for kw in (dict(labels=None), dict(out=None), dict(center=None), dict(dmax2=None), dict(bbox=None), dict(ws=None), dict(H=0), dict(W=0),
               dict(H=-3), dict(H=32768), dict(W=32768), dict(N=-1), dict(correct=2), dict(correct=-1), dict(ws_bytes=need - 1), dict(ws="odd")):
        bufs = {"out": Buf(3 * h * w, np.float32), "center": Buf(2 * n), "dmax2": Buf(n), "bbox": Buf(4 * n), "ws": Buf(need // 4 + 1)}
        a = dict(base, **{k: b.ptr for k, b in bufs.items()})
        a.update(kw)
        if kw.get("ws") == "odd":
            a["ws"] = vp(bufs["ws"].ptr.value + 4)
        rc = lib.msam_distance_targets(a["labels"], a["H"], a["W"], a["N"], a["correct"], C.c_float(1.0), a["out"], a["center"], a["dmax2"],
                                       a["bbox"], a["ws"], C.c_int64(a["ws_bytes"]), None)
        assert rc != 0 and "msam_distance_targets" in lib.emu_last_error().decode(), kw
        assert all(b.untouched() for b in bufs.values()), kw
    q = lib.msam_distance_targets_workspace_bytes
    assert q(0, 5, 1) == 0 and q(5, 32768, 1) == 0 and q(5, 5, -1) == 0 and q(5, 5, 0) == expected_bytes(5, 5, 0)


# ------------------------------------------------------------------------------------------------ the transform and the loss, on the host

@pytest.fixture()
def host_transform(lib, monkeypatch):
    """``PerObjectDistanceTransform`` with ``ops.distance_targets`` replaced by the host build of the same entry point: every step of the
    transform around the library call runs as it does on the device."""
    from micro_sam_amd.training import label_transform as LT

    def distance_targets(labels, n_objects=None, correct_centers=True, fill=1.0):
        arr = labels.cpu().numpy()
        n = int(arr.max()) if n_objects is None else int(n_objects)
        rc, bufs = run(lib, arr, n, fill=fill, correct=int(correct_centers))
        assert rc == 0
        t = lambda k, *s: torch.from_numpy(bufs[k].body.copy()).reshape(*s)   # noqa: E731
        return LT.DistanceTargets(t("out", 3, *arr.shape), t("center", n, 2), t("dmax2", n), t("bbox", n, 4))
    monkeypatch.setattr(LT, "_distance_targets", distance_targets)
    monkeypatch.setattr(LT, "_device", lambda labels: torch.device("cpu"))
    return LT


def test_transform_channel_order_and_flags(host_transform):
    LT = host_transform
    seg = R.two_piece()
    want, lab = R.transform(seg)
    assert lab.max() == 3                                               # value 5: two components (one joined by a corner), value 2: one
    full = LT.PerObjectDistanceTransform(instances=True)(seg)
    assert isinstance(full, np.ndarray) and full.dtype == np.float32 and full.shape == (4, *seg.shape)
    assert np.array_equal(full[0], lab) and np.array_equal(full[1], want[1])
    assert np.abs(full[2:] - want[2:]).max() <= TOL
    default = LT.PerObjectDistanceTransform()(seg)
    assert default.shape == (3, *seg.shape) and np.array_equal(default, full[1:])
    for kw, rows in ((dict(foreground=False), [2, 3]), (dict(distances=False), [1, 3]), (dict(boundary_distances=False), [1, 2]),
                     (dict(distances=False, boundary_distances=False, instances=True), [0, 1])):
        got = LT.PerObjectDistanceTransform(**kw)(seg)
        assert np.array_equal(got, full[rows]), kw
    as_is, lab2 = R.transform(seg, apply_label=False)
    assert lab2.max() == 2
    got = LT.PerObjectDistanceTransform(instances=True, apply_label=False, distance_fill_value=0.0)(seg)
    assert np.array_equal(got[0], lab2) and np.abs(got[1:] - R.transform(seg, apply_label=False, fill=0.0)[0][1:]).max() <= TOL
    t = LT.PerObjectDistanceTransform(instances=True)(torch.from_numpy(seg))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), full)


def test_transform_min_size_removes_the_middle_id(host_transform):
    LT = host_transform
    seg = R.min_size_case()
    want, lab = R.transform(seg, min_size=25)
    assert lab.max() == 2 and (lab[seg == 2] == 0).all() and (lab[seg == 3] == 2).all()
    got = LT.PerObjectDistanceTransform(instances=True, min_size=25)(seg)
    assert np.array_equal(got[0], lab) and np.abs(got[1:] - want[1:]).max() <= TOL
    kept = LT.PerObjectDistanceTransform(instances=True, min_size=9)(seg)
    assert kept[0].max() == 3


def test_label_components_are_skimage_label_defaults():
    from micro_sam_amd.training.label_transform import label_components
    rng = np.random.default_rng(3)
    for seg in (R.two_piece(), rng.integers(0, 3, (17, 23)).astype(np.int32), np.zeros((4, 5), np.int32), np.full((3, 3), 9, np.int32),
                np.array([[1, 0], [0, 1]], np.int32), np.array([[0, 1], [1, 0]], np.int32), np.array([[4, 7, 4]], np.int32)):
        assert np.array_equal(label_components(seg), R.label_components(seg))


def test_transform_refuses_what_it_does_not_have(host_transform):
    LT = host_transform
    with pytest.raises(NotImplementedError, match="directed_distances"):
        LT.PerObjectDistanceTransform(directed_distances=True)
    with pytest.raises(NotImplementedError, match="3-d"):
        LT.PerObjectDistanceTransform()(np.zeros((2, 8, 8), np.int32))


def _dice(p, t):
    return 1.0 - 2.0 * (p * t).sum() / ((p * p).sum() + (t * t).sum())


@pytest.mark.parametrize("mask", [True, False])
def test_dice_based_distance_loss_closed_form(mask):
    from micro_sam_amd.training.joint_sam_trainer import DiceBasedDistanceLoss
    rng = np.random.default_rng(0)
    p, t = rng.random((2, 3, 8, 9)), rng.random((2, 3, 8, 9))
    t[:, 0] = t[:, 0] > 0.5
    m = t[:, 0] if mask else np.ones_like(t[:, 0])
    want = _dice(p[:, 0], t[:, 0]) + _dice(p[:, 1] * m, t[:, 1] * m) + _dice(p[:, 2] * m, t[:, 2] * m)
    got = DiceBasedDistanceLoss(mask_distances_in_bg=mask)(torch.from_numpy(p), torch.from_numpy(t))
    assert got.shape == () and abs(float(got) - want) <= 1e-12
    with pytest.raises(ValueError, match="3 channels"):
        DiceBasedDistanceLoss()(torch.zeros(1, 4, 3, 3), torch.zeros(1, 4, 3, 3))


def test_dice_based_distance_loss_gradient():
    from micro_sam_amd.training.joint_sam_trainer import DiceBasedDistanceLoss
    g = torch.Generator().manual_seed(1)
    p = torch.rand(2, 3, 8, 9, generator=g, dtype=torch.float64).requires_grad_()
    t = torch.rand(2, 3, 8, 9, generator=g, dtype=torch.float64)
    t[:, 0] = (t[:, 0] > 0.5).double()
    assert torch.autograd.gradcheck(DiceBasedDistanceLoss(), (p, t))
    assert torch.autograd.gradcheck(DiceBasedDistanceLoss(mask_distances_in_bg=False), (p, t))
