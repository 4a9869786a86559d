"""msam_instance_norm_stats / _apply / _backward and msam_column_sums_f32 (csrc/conv3d.hip) compiled for the host
(tests/hip_host_shim.build_library) and driven through their C ABI on the shapes and inputs of tests/instnorm_ref.py: forward with and
without residual and activation, the bf16 output, the backward pass, guard bytes around every buffer, bit-identical repeats, row strides
wider than C, and the refusals (V = 1 among them), which leave the outputs untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import instnorm_ref as R
from hip_host_shim import build_library
from test_conv3d_host import Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_instnorm")), ROOT, files=["conv3d.hip"])
    lib.msam_instance_norm_workspace_bytes.restype = i64
    lib.msam_instance_norm_workspace_bytes.argtypes = [i32, i64, i32]
    lib.msam_instance_norm_stats.argtypes = [vp, i64, i32, i64, i32, vp, vp, i64, vp]
    lib.msam_instance_norm_apply.argtypes = [vp, i64, vp, vp, i64, vp, i32, i64, i32, f32, f32, i32, vp, i64, vp, i64, vp]
    lib.msam_instance_norm_backward.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i32, i64, i32, f32, f32, i32, vp, i64, vp, i64, vp, vp, i64, vp]
    lib.msam_column_sums_f32.argtypes = [vp, i64, i64, i32, vp, vp, i64, vp]
    lib.emu_last_error.restype = C.c_char_p
    return lib


def stats_of(lib, g, shape, ld):
    B, V, Cc = shape
    need = lib.msam_instance_norm_workspace_bytes(B, V, Cc)
    assert need > 0
    ws, st = Guarded(np.zeros(need, np.uint8)), Guarded(np.full((B, Cc, 2), -7.0))
    assert lib.msam_instance_norm_stats(g.ptr, ld, B, V, Cc, st.ptr, ws.ptr, need, None) == 0, lib.emu_last_error()
    assert ws.intact() and st.intact() and g.intact()
    return st


def wide(t: torch.Tensor, ld: int) -> np.ndarray:
    """The rows of ``t`` in a matrix of row stride ``ld`` whose other columns hold a sentinel."""
    out = np.full((t.shape[0], ld), np.float32(-777.0))
    out[:, :t.shape[1]] = t.numpy()
    return out


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("with_r,act", R.CONFIGS)
def test_forward_and_backward_against_fp64(lib, shape, with_r, act):
    B, V, Cc = shape
    M, ld = B * V, Cc + 4                                                    # a row stride wider than C, as a column slice has
    a, r, dy = R.make(shape)
    ref = R.reference(shape, with_r, act)
    ga, gr, gy = Guarded(wide(a, ld)), Guarded(wide(r, ld)), Guarded(dy.numpy())
    sa = stats_of(lib, ga, shape, ld)
    sr = stats_of(lib, gr, shape, ld) if with_r else None
    want_mean = a.double().reshape(B, V, Cc).mean(1)
    assert np.allclose(sa.view[..., 0], want_mean.numpy(), rtol=1e-14, atol=0)
    assert np.allclose(sa.view[..., 1], a.double().reshape(B, V, Cc).var(1, unbiased=False).numpy(), rtol=1e-9, atol=0)

    def forward():
        o32, o16 = Guarded(np.full((M, ld), np.float32(-777.0))), Guarded(np.zeros((M, Cc), np.uint16))
        st = lib.msam_instance_norm_apply(ga.ptr, ld, sa.ptr, gr.ptr if with_r else None, ld, sr.ptr if with_r else None, B, V, Cc, R.EPS,
                                          R.SLOPE, int(act), o32.ptr, ld, o16.ptr, Cc, None)
        assert st == 0, lib.emu_last_error()
        assert o32.intact() and o16.intact() and ga.intact() and gr.intact()
        assert (o32.view[:, Cc:] == np.float32(-777.0)).all()
        return o32.view[:, :Cc].copy(), o16.view.copy()
    y32, y16 = forward()
    err = float((torch.as_tensor(y32).double() - ref["y"]).abs().max())
    print(f"forward {shape} residual={with_r} act={act}: error {err:.3e}, torch fp32 {ref['yard_y']:.3e}, allowed {ref['tol_y']:.3e}")
    assert err <= ref["tol_y"]
    R.bf16_check(torch.as_tensor(y16.view(np.int16)).view(torch.bfloat16), ref["y"])
    again32, again16 = forward()
    assert np.array_equal(y32.view(np.uint32), again32.view(np.uint32)) and np.array_equal(y16, again16)

    need = lib.msam_instance_norm_workspace_bytes(B, V, Cc)
    ws, sums = Guarded(np.zeros(need, np.uint8)), Guarded(np.zeros((B, Cc, 3)))
    da, dr = Guarded(np.full((M, Cc), np.float32(-777.0))), Guarded(np.full((M, Cc), np.float32(-777.0)))
    st = lib.msam_instance_norm_backward(gy.ptr, Cc, ga.ptr, ld, sa.ptr, gr.ptr if with_r else None, ld, sr.ptr if with_r else None, B, V, Cc,
                                         R.EPS, R.SLOPE, int(act), da.ptr, Cc, dr.ptr if with_r else None, Cc, sums.ptr, ws.ptr, need, None)
    assert st == 0, lib.emu_last_error()
    assert all(g.intact() for g in (ws, sums, da, dr, gy, ga, gr))
    errs = [float((torch.as_tensor(da.view).double() - ref["da"]).abs().max())]
    if with_r:
        errs.append(float((torch.as_tensor(dr.view).double() - ref["dr"]).abs().max()))
    else:
        assert (dr.view == np.float32(-777.0)).all()
    print(f"backward {shape} residual={with_r} act={act}: error {max(errs):.3e}, torch fp32 {ref['yard_g']:.3e}, allowed {ref['tol_g']:.3e}")
    assert max(errs) <= ref["tol_g"]


def test_column_sums(lib):
    x = torch.randn(1000, 16, generator=torch.Generator().manual_seed(0)) + 50
    need = lib.msam_instance_norm_workspace_bytes(1, 1000, 16)
    gx, ws, out = Guarded(x.numpy()), Guarded(np.zeros(need, np.uint8)), Guarded(np.zeros(16))
    assert lib.msam_column_sums_f32(gx.ptr, 16, 1000, 16, out.ptr, ws.ptr, need, None) == 0, lib.emu_last_error()
    assert gx.intact() and ws.intact() and out.intact()
    assert np.allclose(out.view, x.double().sum(0).numpy(), rtol=1e-14, atol=0)


def test_refusals_leave_the_outputs_untouched(lib):
    B, V, Cc = 1, 8, 8
    ga, st = Guarded(np.zeros((8, 8), np.float32)), Guarded(np.full((1, 8, 2), -7.0))
    need = lib.msam_instance_norm_workspace_bytes(B, V, Cc)
    ws, out = Guarded(np.zeros(need, np.uint8)), Guarded(np.full((8, 8), np.float32(-777.0)))
    assert lib.msam_instance_norm_workspace_bytes(1, 8, 12) == -1 and lib.msam_instance_norm_workspace_bytes(0, 8, 8) == -1

    def stats(V=V, Cc=Cc, ld=8, ws_bytes=need, xp=None):
        return lib.msam_instance_norm_stats(ga.ptr if xp is None else xp, ld, B, V, Cc, st.ptr, ws.ptr, ws_bytes, None)
    for kw in (dict(V=1), dict(Cc=12), dict(Cc=2), dict(Cc=2048), dict(ld=4), dict(ld=10), dict(ws_bytes=need - 8), dict(xp=ga.ptr + 4), dict(V=0)):
        assert stats(**kw) == 1, kw
        assert b"msam_instance_norm" in lib.emu_last_error(), kw
    assert b"V >= 2" in (stats(V=1), lib.emu_last_error())[1]
    assert (st.view == -7.0).all()

    def apply(V=V, ld=8, o=out.ptr, eps=1e-5):
        return lib.msam_instance_norm_apply(ga.ptr, ld, st.ptr, None, 0, None, B, V, Cc, eps, 0.01, 1, o, 8, None, 0, None)
    for kw in (dict(V=1), dict(ld=6), dict(o=None), dict(o=out.ptr + 4), dict(eps=-1.0)):
        assert apply(**kw) == 1, kw
    assert lib.msam_instance_norm_apply(ga.ptr, 8, st.ptr, ga.ptr, 8, None, B, V, Cc, 1e-5, 0.01, 1, out.ptr, 8, None, 0, None) == 1   # r without stats
    assert (out.view == np.float32(-777.0)).all() and out.intact()
    assert stats() == 0 and apply() == 0 and not out.view.any()                # zeros in: (0 - 0) rstd = 0
