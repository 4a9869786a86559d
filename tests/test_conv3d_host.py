"""msam_conv3d_k3_bf16 and msam_conv3d_k3_wgrad_bf16 (csrc/conv3d.hip) compiled for the host (tests/hip_host_shim.build_library) and
driven through their C ABI on the cases of tests/conv3d_ref.py: every output element within the fp32 dot-product bound of torch's Conv3d
in fp64, guard bytes around every buffer intact (the kernels form no address outside their operands), bit-identical repeats, the input
gradient through W' against the fp64 transpose convolution, the weight gradient against fp64 autograd, and the refusals, which leave the
output untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conv3d_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                                             # bytes on either side of every buffer
PATTERN = 0xA5
IDS = dict(ids=lambda c: "x".join(map(str, c)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_conv3d")), ROOT, files=["conv3d.hip"])
    lib.msam_conv3d_k3_bf16.restype = C.c_int
    lib.msam_conv3d_k3_bf16.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p]
    lib.msam_conv3d_k3_wgrad_workspace_bytes.restype = C.c_int64
    lib.msam_conv3d_k3_wgrad_workspace_bytes.argtypes = [C.c_int32] * 6
    lib.msam_conv3d_k3_wgrad_bf16.restype = C.c_int
    lib.msam_conv3d_k3_wgrad_bf16.argtypes = ([C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int32] * 6 +
                                              [C.c_void_p])
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


def run(lib, x, w2, bias, geom):
    """x [M, Ci], w2 [Co', Kp] (fp64 tensors of bf16 values), bias fp64 [Co'] or None -> out float32 [M, Co']."""
    B, D, H, W = geom
    M, Ci = x.shape
    Co = w2.shape[0]
    gx, gw = Guarded(bf16_bits(x)), Guarded(bf16_bits(w2))
    gb = Guarded(bias.numpy().astype(np.float32)) if bias is not None else None
    go = Guarded(np.full((M, Co), np.float32(-777.0)))
    st = lib.msam_conv3d_k3_bf16(gx.ptr, Ci, gw.ptr, gb.ptr if gb else None, go.ptr, Co, B, D, H, W, Ci, Co, None)
    assert st == 0, lib.emu_last_error()
    assert all(g.intact() for g in [gx, gw, go] + ([gb] if gb else []))
    assert not (go.view == np.float32(-777.0)).any()
    return go.view.copy()


def within(got, want: torch.Tensor, bound: torch.Tensor):
    err = (torch.as_tensor(got, dtype=torch.float64) - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    assert bool((err <= bound).all()), f"worst error / bound = {worst:.3f}"
    return worst


@pytest.mark.parametrize("case", R.CASES, **IDS)
def test_forward_against_conv3d_fp64(lib, case):
    from micro_sam_amd._conv3d import padded_co, tap_major
    Co = case[5]
    x, w, bias, _ = R.make_case(case)
    want, bound = R.forward(case, x, w, bias)
    w2 = tap_major(w)
    assert w2.shape[0] == padded_co(Co) <= 2 * Co
    b2 = torch.nn.functional.pad(bias, (0, w2.shape[0] - Co))
    got = run(lib, x, w2, b2, case[:4])
    print("forward", case, "worst error / bound", within(got[:, :Co], want, bound))
    assert not got[:, Co:].any()                                            # the padded columns are exact zeros
    again = run(lib, x, w2, b2, case[:4])
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))       # the same bits on every run
    nobias = run(lib, x, w2, None, case[:4])
    want0, bound0 = R.forward(case, x, w, None)
    within(nobias[:, :Co], want0, bound0)


@pytest.mark.parametrize("case", R.CASES, **IDS)
def test_input_gradient_through_the_transposed_weight(lib, case):
    from micro_sam_amd._conv3d import tap_major_transposed
    Ci = case[4]
    _, w, _, dy = R.make_case(case)
    want, bound = R.input_gradient(case, dy, w)
    got = run(lib, dy, tap_major_transposed(w), None, case[:4])
    print("dX", case, "worst error / bound", within(got[:, :Ci], want, bound))
    assert not got[:, Ci:].any()


@pytest.mark.parametrize("case", R.CASES, **IDS)
def test_weight_gradient_against_fp64_autograd(lib, case):
    B, D, H, W, Ci, Co = case
    x, _, _, dy = R.make_case(case)
    _, (dw, bound), _ = R.autograd(case)
    need = lib.msam_conv3d_k3_wgrad_workspace_bytes(B, D, H, W, Ci, Co)
    assert need > 0

    def once():
        gx, gy = Guarded(bf16_bits(x)), Guarded(bf16_bits(dy))
        gw, gs = Guarded(np.full((27 * Ci, Co), np.float32(-777.0))), Guarded(np.zeros(need, np.uint8))
        st = lib.msam_conv3d_k3_wgrad_bf16(gx.ptr, Ci, gy.ptr, Co, gw.ptr, gs.ptr, need, B, D, H, W, Ci, Co, None)
        assert st == 0, lib.emu_last_error()
        assert gx.intact() and gy.intact() and gw.intact() and gs.intact()
        return gw.view.copy()
    got = once()
    mine = torch.as_tensor(got, dtype=torch.float64).reshape(27, Ci, Co).permute(2, 1, 0).reshape(Co, Ci, 3, 3, 3)
    print("dW", case, "worst error / bound", within(mine, dw, bound))
    assert np.array_equal(got.view(np.uint32), once().view(np.uint32))


def test_a_wrong_neighbour_would_show():
    """The inputs make a wrong tap visible: the restatement WITHOUT the volume boundary (one volume of B D slices) and the one WITHOUT
    the row boundary (rows of 2 W voxels) differ from the right one by far more than the bound."""
    case = (2, 3, 5, 7, 16, 8)
    B, D, H, W, Ci, Co = case
    x, w, bias, _ = R.make_case(case)
    want, bound = R.forward(case, x, w, bias)
    for other in ((1, B * D, H, W, Ci, Co), (B, D, H // 5, 5 * W, Ci, Co)):
        leaky, _ = R.forward(other, x, w, bias)
        assert bool(((leaky - want).abs() > 20 * bound).any())


def test_refusals_leave_the_output_untouched(lib):
    B, D, H, W, Ci, Co = 1, 2, 4, 4, 16, 16
    M, Kp = B * D * H * W, 448
    gx, gw = Guarded(np.zeros((M, 32), np.uint16)), Guarded(np.zeros((32, Kp), np.uint16))
    go = Guarded(np.full((M, 32), np.float32(-777.0)))

    def call(xp=None, wp=None, op=None, ldx=32, ldc=32, B=B, D=D, H=H, W=W, Ci=Ci, Co=Co):
        return lib.msam_conv3d_k3_bf16(gx.ptr if xp is None else xp, ldx, gw.ptr if wp is None else wp, None,
                                       go.ptr if op is None else op, ldc, B, D, H, W, Ci, Co, None)
    bad = [dict(Ci=12), dict(Ci=0), dict(Ci=4), dict(Ci=8192), dict(Co=8), dict(Co=24), dict(Co=0), dict(D=0), dict(B=0), dict(H=0),
           dict(W=0), dict(ldx=8), dict(ldx=20), dict(ldc=8), dict(ldc=18), dict(xp=gx.ptr + 2), dict(wp=gw.ptr + 8), dict(op=go.ptr + 4),
           dict(B=1 << 20, D=1 << 10, H=4, W=4)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert b"msam_conv3d_k3_bf16" in lib.emu_last_error(), kw
    for which in ("x", "w", "o"):
        st = lib.msam_conv3d_k3_bf16(None if which == "x" else gx.ptr, 32, None if which == "w" else gw.ptr, None,
                                     None if which == "o" else go.ptr, 32, B, D, H, W, Ci, Co, None)
        assert st == 1 and b"null pointer" in lib.emu_last_error()
    assert (go.view == np.float32(-777.0)).all() and go.intact() and gx.intact() and gw.intact()
    assert call() == 0 and not (go.view[:, :Co] == np.float32(-777.0)).any()      # the same buffers are fine with legal arguments
    assert (go.view[:, Co:] == np.float32(-777.0)).all()                           # ldc > Co: the columns past Co are not written

    # the weight gradient's refusals
    gy, gd = Guarded(np.zeros((M, 16), np.uint16)), Guarded(np.full((27 * Ci, 16), np.float32(-777.0)))
    need = lib.msam_conv3d_k3_wgrad_workspace_bytes(B, D, H, W, Ci, 16)
    gs = Guarded(np.zeros(need, np.uint8))
    assert lib.msam_conv3d_k3_wgrad_workspace_bytes(B, D, H, W, 12, 16) == -1

    def wcall(ws=need, ldx=32, ldy=16, Ci=Ci, Co=16, yp=None):
        return lib.msam_conv3d_k3_wgrad_bf16(gx.ptr, ldx, gy.ptr if yp is None else yp, ldy, gd.ptr, gs.ptr, ws, B, D, H, W, Ci, Co, None)
    for kw in (dict(ws=need - 1), dict(ldx=12), dict(ldy=8), dict(Ci=12), dict(Co=12), dict(Co=0), dict(yp=gy.ptr + 2)):
        assert wcall(**kw) == 1, kw
        assert b"msam_conv3d_k3_wgrad" in lib.emu_last_error(), kw
    assert (gd.view == np.float32(-777.0)).all() and gd.intact() and gs.intact()
    assert wcall() == 0 and not gd.view.any()                                      # zeros in, zeros out
