"""The two geometries of the implicit-GEMM tile body (csrc/conv3d.hip) against each other, compiled for the host
(tests/hip_host_shim.build_library): msam_depth_conv3_bf16 on (B, D, T, Ci, Co) and msam_conv3d_k3_bf16 on (B, D, H = T, W = 1, Ci, Co)
with the depth taps embedded in the 27-tap weight (tests/depth_conv_ref.embed_in_cube) give the same bits.  Ci % 64 == 0 here, so no
k-tile mixes taps and the embedded zeros add exact zeros: the two entries do the same arithmetic in the same order."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_conv_ref as R
from hip_host_shim import build_library
from test_depth_conv_host import Guarded, bf16_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 1, 80, 64, 128), (2, 3, 80, 128, 128), (1, 3, 130, 64, 256)]        # (B, D, T, Ci, Co)
HEAD = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_conv_body")), ROOT, files=["conv3d.hip"])
    lib.msam_depth_conv3_bf16.restype = C.c_int
    lib.msam_depth_conv3_bf16.argtypes = HEAD + [C.c_int32] * 5 + [C.c_void_p]
    lib.msam_conv3d_k3_bf16.restype = C.c_int
    lib.msam_conv3d_k3_bf16.argtypes = HEAD + [C.c_int32] * 6 + [C.c_void_p]
    lib.emu_last_error.restype = C.c_char_p
    return lib


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_depth_entry_equals_cube_entry_on_the_embedded_weight(lib, case):
    from micro_sam_amd import _conv3d, _depthconv
    B, D, T, Ci, Co = case
    x, w, bias, _ = R.make_case(case)
    gx, gb = Guarded(bf16_bits(x)), Guarded(bias.numpy().astype(np.float32))
    gw3, gw27 = Guarded(bf16_bits(_depthconv.tap_major(w))), Guarded(bf16_bits(_conv3d.tap_major(R.embed_in_cube(w))))
    assert gw27.view.shape == (Co, 27 * Ci)
    depth, cube = (Guarded(np.full((B * D * T, Co), np.float32(-777.0))) for _ in range(2))
    assert lib.msam_depth_conv3_bf16(gx.ptr, Ci, gw3.ptr, gb.ptr, depth.ptr, Co, B, D, T, Ci, Co, None) == 0, lib.emu_last_error()
    assert lib.msam_conv3d_k3_bf16(gx.ptr, Ci, gw27.ptr, gb.ptr, cube.ptr, Co, B, D, T, 1, Ci, Co, None) == 0, lib.emu_last_error()
    assert all(g.intact() for g in (gx, gb, gw3, gw27, depth, cube))
    assert not (depth.view == np.float32(-777.0)).any()
    assert np.array_equal(depth.view.view(np.uint32), cube.view.view(np.uint32))
