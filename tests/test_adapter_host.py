"""msam_adapter_bf16 (csrc/adapter.hip) compiled for the host (tests/hip_host_shim.build_library) and driven through its C ABI on the cases of
tests/adapter_ref.py, in both 16-bit types: every output element within the derived bound of the fp64 restatement, guard bytes around every
buffer intact (the kernel forms no address outside its operands - the ragged last tile included), bit-identical repeats, alpha = 0 and
Wu = 0 leave what the equation says, and the refusals leave x untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import adapter_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                                             # bytes on either side of every buffer
PATTERN = 0xA5
F32, BF16, F16 = 1, 2, 4                                                # include/msam_hip.h MSAM_F32 / MSAM_BF16 / MSAM_F16
CODE = {"bf16": BF16, "fp16": F16}
IDS = dict(ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_adapter")), ROOT, files=["adapter.hip"])
    lib.msam_adapter_bf16.restype = C.c_int
    lib.msam_adapter_bf16.argtypes = ([C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_int32] * 4 + [C.c_void_p])
    lib.emu_last_error.restype = C.c_char_p
    return lib


class Guarded:
    """A 64-byte aligned copy of ``arr`` with GUARD bytes of PATTERN before and after it."""

    def __init__(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self.raw = np.full(arr.nbytes + 2 * GUARD + 64, PATTERN, dtype=np.uint8)
        self.start = (-self.raw.ctypes.data) % 64 + GUARD
        self.view = self.raw[self.start:self.start + arr.nbytes].view(arr.dtype).reshape(arr.shape)
        self.view[...] = arr
        self.ptr = self.raw.ctypes.data + self.start
        self.nbytes = arr.nbytes

    def intact(self) -> bool:
        return bool((self.raw[:self.start] == PATTERN).all() and (self.raw[self.start + self.nbytes:] == PATTERN).all())


def bits16(t: torch.Tensor, dtype: str) -> np.ndarray:
    b = t.to(torch.float32).to(R.DTYPES[dtype])
    assert torch.equal(b.to(torch.float64), t.to(torch.float64))          # the operands are 16-bit values already
    return b.view(torch.int16).numpy().view(np.uint16)


def f32(t: torch.Tensor) -> np.ndarray:
    a = t.numpy().astype(np.float32)
    assert np.array_equal(a.astype(np.float64), t.numpy())               # ... and these fp32 values
    return a


def run(lib, ops, alpha: float, dtype: str, pad_y: int = 0, pad_x: int = 0):
    """ops: the dict of adapter_ref.make_case -> x after the call, float32 [R, D].  pad_y / pad_x: extra columns of the y / x rows (the row
    strides are then larger than D; the extra columns must come back unchanged)."""
    y, x = ops["y"], ops["x"]
    Rr, D = y.shape
    P = ops["wd"].shape[0]
    y16 = np.full((Rr, D + pad_y), 0x7FC1, np.uint16)                      # the padding columns: NaNs, never read
    y16[:, :D] = bits16(y, dtype)
    xs = np.full((Rr, D + pad_x), np.float32(-777.0))
    xs[:, :D] = f32(x)
    gy, gwd, gwu = Guarded(y16), Guarded(bits16(ops["wd"], dtype)), Guarded(bits16(ops["wu"], dtype))
    gbd, gbu, ga = Guarded(f32(ops["bd"])), Guarded(f32(ops["bu"])), Guarded(np.array([alpha], np.float32))
    gx = Guarded(xs)
    st = lib.msam_adapter_bf16(gy.ptr, D + pad_y, gwd.ptr, gbd.ptr, gwu.ptr, gbu.ptr, ga.ptr, gx.ptr, D + pad_x, Rr, D, P, CODE[dtype], None)
    assert st == 0, lib.emu_last_error()
    assert all(g.intact() for g in (gy, gwd, gwu, gbd, gbu, ga, gx))
    assert (gx.view[:, D:] == np.float32(-777.0)).all()
    return gx.view[:, :D].copy()


def within(got, want: torch.Tensor, bound: torch.Tensor):
    err = (torch.as_tensor(got, dtype=torch.float64) - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    assert bool((err <= bound).all()), f"worst error / bound = {worst:.3f}"
    return worst


EXTRA = [(33, 128, 96)]            # P = 96: the kernel's half-used second slab of the hidden


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.CASES + EXTRA, **IDS)
def test_against_fp64(lib, case, dtype):
    ops = R.make_case(case, dtype)
    zf = R.zero_fraction(ops["y"], ops["wd"], ops["bd"])
    assert 0.2 <= zf <= 0.8, zf                                             # the ReLU clips
    want, bound = R.forward(alpha=R.ALPHA, dtype=dtype, **ops)
    got = run(lib, ops, R.ALPHA, dtype)
    print("adapter", case, dtype, "zero fraction", round(zf, 3), "worst error / bound", within(got, want, bound))
    again = run(lib, ops, R.ALPHA, dtype)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))       # the same bits on every run


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_row_strides_larger_than_d(lib, dtype):
    case = (17, 128, 64)
    ops = R.make_case(case, dtype)
    want, bound = R.forward(alpha=R.ALPHA, dtype=dtype, **ops)
    got = run(lib, ops, R.ALPHA, dtype, pad_y=24, pad_x=5)
    within(got, want, bound)
    assert np.array_equal(got.view(np.uint32), run(lib, ops, R.ALPHA, dtype).view(np.uint32))    # the strides change no bit


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_alpha_zero_and_wu_zero(lib, dtype):
    case = (129, 768, 64)
    ops = R.make_case(case, dtype)
    got = run(lib, ops, 0.0, dtype)
    assert np.array_equal(got, f32(ops["x"]) + f32(ops["y"]))               # exactly x + y: one fp32 add
    zero = dict(ops, wu=torch.zeros_like(ops["wu"]))
    got = run(lib, zero, R.ALPHA, dtype)
    want = ops["x"] + ops["y"] + R.ALPHA * ops["bu"]
    # the product is exactly zero; what remains are two roundings, of alpha bu + y and of the add of x
    bound = 2 * R.U * (ops["x"].abs() + ops["y"].abs() + R.ALPHA * ops["bu"].abs())
    within(got, want, bound)


def test_refusals_leave_x_untouched(lib):
    Rr, D, P = 8, 256, 64
    gy, gwd, gwu = Guarded(np.zeros((Rr, D), np.uint16)), Guarded(np.zeros((160, D), np.uint16)), Guarded(np.zeros((D, 160), np.uint16))
    gbd, gbu, ga = Guarded(np.zeros(160, np.float32)), Guarded(np.zeros(D, np.float32)), Guarded(np.ones(1, np.float32))
    gx = Guarded(np.full((Rr, D), np.float32(-777.0)))

    def call(D=D, P=P, dtype16=BF16, alpha=ga.ptr, y=gy.ptr, x=gx.ptr, ldy=D, ldx=D, R_=Rr, wd=gwd.ptr, wu=gwu.ptr, bd=gbd.ptr, bu=gbu.ptr):
        return lib.msam_adapter_bf16(y, ldy, wd, bd, wu, bu, alpha, x, ldx, R_, D, P, dtype16, None)
    bad = [dict(D=192, ldy=192, ldx=192), dict(P=16), dict(P=160), dict(alpha=None), dict(dtype16=F32), dict(P=0), dict(D=0), dict(R_=0),
           dict(y=None), dict(x=None), dict(wd=None), dict(wu=None), dict(bd=None), dict(bu=None), dict(ldy=D - 8), dict(ldy=D + 4),
           dict(ldx=D - 1), dict(y=gy.ptr + 2), dict(P=48)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"msam_adapter_bf16" in lib.emu_last_error(), kw
    assert (gx.view == np.float32(-777.0)).all()
    assert all(g.intact() for g in (gy, gwd, gwu, gbd, gbu, ga, gx))
    assert call() == 0                                                       # the same buffers are fine with legal arguments
    assert (gx.view == np.float32(-777.0)).all()                             # zeros in: x + 0 + 1 (0 + 0) = x
