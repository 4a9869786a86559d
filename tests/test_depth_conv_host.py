"""msam_depth_conv3_bf16 (csrc/conv3d.hip) compiled for the host (tests/hip_host_shim.build_library) and driven through its C ABI on
the cases of tests/depth_conv_ref.py: every output element within the fp32 dot-product bound of torch's Conv3d in fp64, guard words around
every buffer intact (the kernel forms no address outside its operands), bit-identical repeats, the input gradient through W' against
the fp64 transpose convolution, and the refusals, which leave the output untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import depth_conv_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                                             # bytes on either side of every buffer
PATTERN = 0xA5


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_depth_conv")), ROOT, files=["conv3d.hip"])
    lib.msam_depth_conv3_bf16.restype = C.c_int
    lib.msam_depth_conv3_bf16.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p]
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


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    b = t.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(b.to(torch.float64), t.to(torch.float64))          # the operands are bf16 values already
    return b.view(torch.int16).numpy().view(np.uint16)


def run(lib, x, w2, bias, B, D, T):
    """x [M, Ci], w2 [Co, 3 Ci] (fp64 tensors of bf16 values), bias fp64 [Co] or None -> (out float32 [M, Co], the buffers)."""
    M, Ci = x.shape
    Co = w2.shape[0]
    gx, gw = Guarded(bf16_bits(x)), Guarded(bf16_bits(w2))
    gb = Guarded(bias.numpy().astype(np.float32)) if bias is not None else None
    go = Guarded(np.full((M, Co), np.float32(-777.0)))
    st = lib.msam_depth_conv3_bf16(gx.ptr, Ci, gw.ptr, gb.ptr if gb else None, go.ptr, Co, B, D, T, Ci, Co, None)
    assert st == 0, lib.emu_last_error()
    bufs = [gx, gw, go] + ([gb] if gb else [])
    assert all(g.intact() for g in bufs)
    return go.view.copy(), bufs


def within(got: np.ndarray, want: torch.Tensor, bound: torch.Tensor):
    err = (torch.as_tensor(got, dtype=torch.float64) - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    assert bool((err <= bound).all()), f"worst error / bound = {worst:.3f}"
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_forward_against_conv3d_fp64(lib, case, with_bias):
    from micro_sam_amd._depthconv import tap_major
    B, D, T, Ci, Co = case
    x, w, bias, _ = R.make_case(case)
    bias = bias if with_bias else None
    want, bound = R.forward(case, x, w, bias)
    got, _ = run(lib, x, tap_major(w), bias, B, D, T)
    print("forward", case, "worst error / bound", within(got, want, bound))
    again, _ = run(lib, x, tap_major(w), bias, B, D, T)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))       # the same bits on every run


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
def test_input_gradient_through_the_transposed_weight(lib, case):
    """dX = conv(dY, W') by the same entry point; where Ci is no multiple of 128 the rows of W' are zero-padded to the tile, as
    ``training.functional`` does, and the extra output columns are exact zeros."""
    from micro_sam_amd._depthconv import tap_major_transposed
    B, D, T, Ci, Co = case
    _, w, _, dy = R.make_case(case)
    want, bound = R.input_gradient(case, dy, w)
    wt = tap_major_transposed(w)
    rows = (Ci + 127) // 128 * 128
    wt = torch.cat([wt, torch.zeros(rows - Ci, 3 * Co, dtype=wt.dtype)])
    got, _ = run(lib, dy, wt, None, B, D, T)
    print("dX", case, "worst error / bound", within(got[:, :Ci], want, bound))
    assert not got[:, Ci:].any()


def test_a_leak_would_show():
    """The inputs make a wrong slice visible: the restatement WITHOUT the volume boundary (one volume of B D slices) differs from the
    right one by far more than the bound."""
    case = (2, 3, 80, 384, 384)
    B, D, T, Ci, Co = case
    x, w, bias, _ = R.make_case(case)
    want, bound = R.forward(case, x, w, bias)
    leaky, _ = R.forward((1, B * D, T, Ci, Co), x, w, bias)
    rows = slice((D - 1) * T, (D + 1) * T)                                   # the two slices at the volume boundary
    assert bool(((leaky - want).abs()[rows] > 20 * bound[rows]).all())


def test_refusals_leave_the_output_untouched(lib):
    B, D, T, Ci, Co = 1, 2, 16, 64, 128
    x = np.zeros((B * D * T, 128), np.uint16)
    w = np.zeros((256, 3 * 128), np.uint16)
    gx, gw, go = Guarded(x), Guarded(w), Guarded(np.full((B * D * T, 256), np.float32(-777.0)))

    def call(xp=None, wp=None, op=None, ldx=128, ldc=256, B=B, D=D, T=T, Ci=Ci, Co=Co):
        return lib.msam_depth_conv3_bf16(gx.ptr if xp is None else xp, ldx, gw.ptr if wp is None else wp, None,
                                         go.ptr if op is None else op, ldc, B, D, T, Ci, Co, None)
    bad = [dict(Ci=96), dict(Ci=0), dict(Co=192), dict(Co=64), dict(D=0), dict(B=0), dict(T=0), dict(ldx=32), dict(ldx=132), dict(ldc=64),
           dict(ldc=130), dict(xp=gx.ptr + 2), dict(op=go.ptr + 4)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"msam_depth_conv3_bf16" in lib.emu_last_error(), kw
    for kw in (dict(xp=0), dict(wp=0), dict(op=0)):
        ptrs = {k: None for k in kw}
        st = lib.msam_depth_conv3_bf16(None if "xp" in ptrs else gx.ptr, 128, None if "wp" in ptrs else gw.ptr, None,
                                       None if "op" in ptrs else go.ptr, 256, B, D, T, Ci, Co, None)
        assert st != 0 and b"null pointer" in lib.emu_last_error()
    assert (go.view == np.float32(-777.0)).all() and go.intact() and gx.intact() and gw.intact()
    assert call() == 0 and not (go.view[:, :Co] == np.float32(-777.0)).any()      # the same buffers are fine with legal arguments
    assert (go.view[:, Co:] == np.float32(-777.0)).all()                           # ldc > Co: the columns past Co are not written
