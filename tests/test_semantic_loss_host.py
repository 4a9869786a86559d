"""msam_semantic_loss_forward / _backward (csrc/semloss.hip) compiled for the host (tests/hip_host_shim.build_library) and driven through
the C ABI against tests/semantic_loss_ref.py, with guard words around every buffer: the integer counts exactly, the loss and every entry
of the gradient within the bound of the restatement (4 times the error of the fp32 torch composite against its fp64 self, floors of 2 ulps
of the loss and 2^-22 of the largest gradient entry), the two documented differences from torch, bit-identical repeats, the one-pixel
form against the four-pixel form, and the refusals.  tests/test_gpu_semantic_loss.py runs the same cases on the device.

Measured on the host build (over the cases; the test prints every figure): the kernel's loss error is 0 to 0.22 of the bound and its
gradient error 0.03 to 0.15 of the bound; the fp32 composite's own loss error is 0 to 7.5e-6 (the case with logits of +-80; below 5e-7
otherwise) and its gradient error 6.2e-8 to 3.7e-7 of the largest entry."""
import ctypes as C
import os

import numpy as np
import pytest

import semantic_loss_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
GUARD = 64
CASES = R.cases()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_semantic_loss")), ROOT, files=["semloss.hip"])
    lib.msam_semantic_loss_workspace_bytes.restype = C.c_int64
    lib.emu_last_error.restype = C.c_char_p
    return lib


class Buf:
    """A byte buffer with guard bytes on both sides, 16-byte aligned; ``shift`` moves the body by that many bytes."""

    def __init__(self, nbytes, shift=0):
        self.a = np.full(nbytes + 2 * GUARD + 32, 0xA5, np.uint8)
        self.n, self.off = nbytes, GUARD + (-(self.a.ctypes.data + GUARD) % 16) + shift

    @property
    def ptr(self):
        return vp(self.a.ctypes.data + self.off)

    def view(self, dtype):
        return self.a[self.off:self.off + self.n].view(dtype)

    def intact(self):
        return bool((self.a[:self.off] == 0xA5).all() and (self.a[self.off + self.n:] == 0xA5).all())

    def untouched(self):
        return bool((self.a == 0xA5).all())


def expected_bytes(b, c, hw):
    nwg = (b * hw + 2047) // 2048
    return nwg * (2 * c + 1) * 8 + (nwg * (c + 2) * 4 + 7) // 8 * 8


def run(lib, logits, target, dice_weight=1.0, ce_weight=1.0, softmax=True, upstream=1.0, shift=0):
    """Forward, then backward with ``upstream`` -> dict.  ``shift`` (bytes): moves logits, target and dlogits off their 16-byte
    alignment (the library then takes its one-pixel-per-thread form)."""
    b, c, h, w = logits.shape
    hw = h * w
    need = int(lib.msam_semantic_loss_workspace_bytes(b, c, hw))
    assert need == expected_bytes(b, c, hw)
    x, t = Buf(4 * b * c * hw, shift), Buf(4 * b * hw, shift)
    x.view(np.float32)[:] = logits.reshape(-1)
    t.view(np.int32)[:] = target.reshape(-1)
    ws, loss, stats, up, dx = Buf(need), Buf(4), Buf(8 * (3 * c + 5)), Buf(4), Buf(4 * b * c * hw, shift)
    up.view(np.float32)[0] = upstream
    args = (b, c, hw, C.c_float(dice_weight), C.c_float(ce_weight), int(softmax), C.c_double(R.EPS))
    rc = lib.msam_semantic_loss_forward(x.ptr, t.ptr, *args, ws.ptr, C.c_int64(need), loss.ptr, stats.ptr, None)
    assert rc == 0, lib.emu_last_error().decode()
    assert dx.untouched()
    rc = lib.msam_semantic_loss_backward(x.ptr, t.ptr, *args, stats.ptr, up.ptr, dx.ptr, None)
    assert rc == 0, lib.emu_last_error().decode()
    assert all(q.intact() for q in (x, t, ws, loss, stats, up, dx))
    assert np.array_equal(x.view(np.float32), logits.reshape(-1)) and np.array_equal(t.view(np.int32), target.reshape(-1))
    sd, si = stats.view(np.float64)[:2 * c + 3].copy(), stats.view(np.int64)[2 * c + 3:].copy()
    return {"loss": float(loss.view(np.float32)[0]), "num": sd[:c], "psq": sd[c:2 * c], "ce_sum": sd[2 * c], "dice": sd[2 * c + 1],
            "ce": sd[2 * c + 2], "count": si[:c], "n_valid": int(si[c]), "n_ignored": int(si[c + 1]),
            "grad": dx.view(np.float32).reshape(logits.shape).copy(), "stats_bytes": stats.view(np.uint8).copy()}


def run_case(lib, name, **kw):
    k = CASES[name]
    return run(lib, k["logits"], k["target"], k["dice_weight"], k["ce_weight"], k["softmax"], **kw)


def check_against_reference(name, got, scale=1.0):
    k = CASES[name]
    want, yard = R.reference(name)
    c = k["logits"].shape[1]
    per_class, valid, ignored = R.counts(k["target"], c)
    assert np.array_equal(got["count"], per_class) and got["n_valid"] == valid and got["n_ignored"] == ignored
    bl, bg, yl, yg = R.bounds(want, yard)
    el = abs(got["loss"] - want["loss"])
    eg = float(np.abs(got["grad"].astype(np.float64) - scale * want["grad"]).max())
    gmax = float(np.abs(want["grad"]).max())
    print(f"{name}: loss {want['loss']:.9g} error {el:.3g} = {el / bl:.3f} of the bound (composite {yl:.3g}); gradient error {eg:.3g} = "
          f"{eg / (scale * bg) if bg else 0:.3f} of the bound (composite {yg:.3g} = {yg / gmax if gmax else 0:.3g} of the largest entry)")
    assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all()
    assert el <= bl
    assert eg <= scale * bg
    # the two parts of the statistics are the restatement's (they are fp64 sums of fp32 terms)
    assert abs(got["dice"] - want["dice"]) <= bl and abs(got["ce"] - want["ce"]) <= max(bl, 2 * float(np.spacing(np.float32(abs(want["ce"])))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_and_gradient_equal_the_restatement(lib, name):
    check_against_reference(name, run_case(lib, name))


def test_the_cases_are_what_they_are_for():
    """The properties the cases were chosen for hold in the restatement."""
    def shape(name):
        return CASES[name]["logits"].shape
    assert shape("7x9_c2")[2] * shape("7x9_c2")[3] < 64
    assert (33 * 65) % 4 != 0 and (64 * 64) % 4 == 0 and (9 * 7) % 4 != 0 and (12 * 12) % 4 == 0
    assert 2 * 192 * 192 > 2048 and 513 * 1024 > 256 * 2048             # several workgroups; more partials than threads in the last stage
    t = CASES["33x65_c3_ignored"]["target"]
    assert (t == -100).sum() == 65 and (t == 3).sum() == 3 and (t == -1).sum() == 3 and (t == 1000).sum() == 1
    assert R.counts(CASES["16x16_c5_never"]["target"], 5)[0][4] == 0
    assert R.counts(CASES["8x8_c9_runtime"]["target"], 9)[0][7] == 0 and R.counts(CASES["8x8_c9_runtime"]["target"], 9)[2] == 9
    assert R.counts(CASES["8x8_c3_no_valid"]["target"], 3)[1] == 0
    want, _ = R.reference("8x8_c3_no_valid")
    assert want["ce"] == 0.0 and np.isfinite(want["loss"])
    assert set(np.unique(CASES["16x16_c3_pm80"]["logits"])) == {-80.0, 80.0}
    want, _ = R.reference("16x16_c3_raw_zero_channel")
    assert (want["grad"][:, 1] == 0).all() and np.abs(want["grad"][:, 0]).max() > 0


def test_documented_differences_from_torch(lib):
    """Ids outside [0, C) count as ignored (one-hot of zeros, no cross-entropy term), and without a valid pixel ce = 0 with a gradient
    that is the dice part's alone."""
    got = run_case(lib, "33x65_c3_ignored")
    assert got["n_ignored"] == 65 + 3 + 3 + 1 and got["n_valid"] == 2 * 33 * 65 - 72
    k = CASES["8x8_c3_no_valid"]
    got = run_case(lib, "8x8_c3_no_valid")
    assert got["n_valid"] == 0 and got["ce"] == 0.0 and got["ce_sum"] == 0.0 and (got["count"] == 0).all()
    assert got["loss"] == np.float32(got["dice"]) and got["dice"] == 3.0          # num = 0 for every class
    assert (got["grad"] == 0).all()
    only_ce = run(lib, k["logits"], k["target"], 0.0, 1.0)
    assert only_ce["loss"] == 0.0 and (only_ce["grad"] == 0).all()


def test_raw_predictions_with_an_empty_channel(lib):
    got = run_case(lib, "16x16_c3_raw_zero_channel")
    assert got["psq"][1] == 0.0 and got["count"][1] == 0 and got["num"][1] == 0.0
    assert (got["grad"][:, 1] == 0).all()


def test_large_logits_stay_finite(lib):
    got = run_case(lib, "16x16_c3_pm80")
    assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all() and np.isfinite(got["ce_sum"]) and got["ce"] > 10


def test_one_pixel_and_four_pixel_forms_agree(lib):
    """(2, 3, 64, 64) aligned takes four pixels per thread, shifted by one element one pixel per thread: another order of the sums, the
    same bound; the counts are equal."""
    a, b = run_case(lib, "64x64_c3"), run_case(lib, "64x64_c3", shift=4)
    assert np.array_equal(a["count"], b["count"]) and a["n_valid"] == b["n_valid"]
    check_against_reference("64x64_c3", b)
    want, yard = R.reference("64x64_c3")
    bl, bg, _, _ = R.bounds(want, yard)
    assert abs(a["loss"] - b["loss"]) <= 2 * bl and np.abs(a["grad"] - b["grad"]).max() <= 2 * bg
    for name in ("12x12_c12_runtime_vec", "192x192_c3_scaled"):
        check_against_reference(name, run_case(lib, name, shift=4))


@pytest.mark.parametrize("name", ["192x192_c3_scaled", "12x12_c12_runtime_vec", "33x65_c3_ignored"])
def test_two_runs_are_identical(lib, name):
    a, b = run_case(lib, name), run_case(lib, name)
    assert a["loss"] == b["loss"] and np.array_equal(a["stats_bytes"], b["stats_bytes"]) and np.array_equal(a["grad"], b["grad"])


def test_upstream_gradient_scales_the_result(lib):
    for name in ("33x65_c3_ignored", "8x8_c9_runtime", "16x16_c3_raw_zero_channel"):
        check_against_reference(name, run_case(lib, name, upstream=2.5), scale=2.5)
    a, b = run_case(lib, "64x64_c3"), run_case(lib, "64x64_c3", upstream=-2.0)
    assert np.array_equal(-2.0 * a["grad"], b["grad"])                   # a power of two: exactly


def test_refusals_leave_the_outputs_untouched(lib):
    k = CASES["33x65_c3_ignored"]
    b, c, h, w = k["logits"].shape
    hw = h * w
    need = int(lib.msam_semantic_loss_workspace_bytes(b, c, hw))
    x, t = np.ascontiguousarray(k["logits"]), np.ascontiguousarray(k["target"])
    base = dict(x=x.ctypes.data_as(vp), t=t.ctypes.data_as(vp), B=b, C=c, HW=hw, dw=1.0, cw=1.0, sm=1, eps=R.EPS, need=need)
    for kw in (dict(x=None), dict(t=None), dict(ws=None), dict(loss=None), dict(stats=None), dict(up=None), dict(dx=None), dict(B=0), dict(C=1),
               dict(C=33), dict(C=0), dict(HW=0), dict(HW=-5), dict(B=1 << 20, HW=1 << 10), dict(sm=0), dict(sm=2), dict(sm=-1), dict(eps=0.0),
               dict(dw=float("nan")), dict(cw=float("nan")), dict(need=need - 1), dict(ws="odd"), dict(stats="odd")):
        bufs = {"ws": Buf(need + 8), "loss": Buf(4), "stats": Buf(8 * (3 * c + 5) + 8), "up": Buf(4), "dx": Buf(4 * b * c * hw)}
        a = dict(base, **{n: q.ptr for n, q in bufs.items()})
        a.update(kw)
        for n in ("ws", "stats"):
            if kw.get(n) == "odd":
                a[n] = vp(bufs[n].ptr.value + 4)
        args = (a["B"], a["C"], a["HW"], C.c_float(a["dw"]), C.c_float(a["cw"]), a["sm"], C.c_double(a["eps"]))
        forward = not ({"up", "dx"} & set(kw))
        backward = not ({"ws", "loss", "need"} & set(kw))
        if forward:
            rc = lib.msam_semantic_loss_forward(a["x"], a["t"], *args, a["ws"], C.c_int64(a["need"]), a["loss"], a["stats"], None)
            assert rc != 0 and "msam_semantic_loss_forward" in lib.emu_last_error().decode(), kw
        if backward:
            rc = lib.msam_semantic_loss_backward(a["x"], a["t"], *args, a["stats"], a["up"], a["dx"], None)
            assert rc != 0 and "msam_semantic_loss_backward" in lib.emu_last_error().decode(), kw
        assert all(q.untouched() for q in bufs.values()), kw
    q = lib.msam_semantic_loss_workspace_bytes
    assert q(0, 3, 5) == 0 and q(1, 1, 5) == 0 and q(1, 33, 5) == 0 and q(1, 3, 0) == 0 and q(1 << 20, 2, 1 << 10) == 0
    assert q(1, 2, 1) == expected_bytes(1, 2, 1) == 5 * 8 + 16 and q(2, 3, 192 * 192) == expected_bytes(2, 3, 192 * 192)
