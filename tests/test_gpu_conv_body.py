"""The two geometries of the implicit-GEMM tile body (csrc/conv3d.hip) against each other on the device: ``ops.depth_conv3`` on
(B, D, T, Ci, Co) and ``ops.conv3d_k3`` on (B, D, H = T, W = 1, Ci, Co) with the depth taps embedded in the 27-tap weight
(tests/depth_conv_ref.embed_in_cube) give the same bits - tests/test_conv_body_host.py says why they must."""
import pytest
import torch

import depth_conv_ref as R

pytestmark = pytest.mark.gpu

CASES = [(2, 3, 80, 128, 128), (1, 3, 130, 64, 256)]                    # (B, D, T, Ci, Co)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_depth_conv3_equals_conv3d_k3_on_the_embedded_weight(case):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import _conv3d, _depthconv, ops
    dev = torch.device("cuda")
    B, D, T, Ci, Co = case
    x, w, bias, _ = R.make_case(case)
    x16, b32 = x.to(dev, torch.bfloat16), bias.to(dev, torch.float32)
    depth = ops.depth_conv3(x16, _depthconv.tap_major(w).to(dev, torch.bfloat16), b32, B, D, T)
    cube = ops.conv3d_k3(x16, _conv3d.tap_major(R.embed_in_cube(w)).to(dev, torch.bfloat16), b32, B, D, T, 1)
    assert depth.shape == cube.shape == (B * D * T, Co) and bool(depth.any())
    assert torch.equal(depth, cube)
