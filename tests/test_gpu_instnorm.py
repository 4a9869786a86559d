"""``ops.instance_norm_stats`` / ``_apply`` / ``_backward`` and ``training.functional.instance_norm_act`` (csrc/conv3d.hip) on the device,
on the shapes, inputs and yardstick of tests/instnorm_ref.py: forward with and without residual and activation, the bf16 output, the
backward pass through autograd, the same bits on every run, and V = 1.

Measured on an MI355X (profiles/r10_simple_sam3d.md): see the table there; the kernels stay below torch's own fp32 error everywhere."""
import pytest
import torch

import instnorm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("with_r,act", R.CONFIGS)
def test_forward_and_backward_against_fp64(dev, shape, with_r, act):
    from micro_sam_amd import ops
    from micro_sam_amd.training import functional as HF
    B, V, C = shape
    a, r, dy = R.make(shape)
    ref = R.reference(shape, with_r, act)
    slope = R.SLOPE if act else None

    def run():
        aa = a.to(dev).reshape(B, V, 1, 1, C).requires_grad_()
        rr = r.to(dev).reshape(B, V, 1, 1, C).requires_grad_() if with_r else None
        y = HF.instance_norm_act(aa, rr, slope, R.EPS)
        y.backward(dy.to(dev).reshape(B, V, 1, 1, C))
        return y.detach().reshape(-1, C), aa.grad.reshape(-1, C), (rr.grad.reshape(-1, C) if with_r else None)
    y, da, dr = run()
    err = float((y.double().cpu() - ref["y"]).abs().max())
    print(f"forward {shape} residual={with_r} act={act}: error {err:.3e}, torch fp32 {ref['yard_y']:.3e}, ratio {err / ref['yard_y']:.3f}")
    assert err <= ref["tol_y"]
    errs = [float((da.double().cpu() - ref["da"]).abs().max())] + ([float((dr.double().cpu() - ref["dr"]).abs().max())] if with_r else [])
    print(f"backward {shape} residual={with_r} act={act}: error {max(errs):.3e}, torch fp32 {ref['yard_g']:.3e}, "
          f"ratio {max(errs) / ref['yard_g']:.3f}")
    assert max(errs) <= ref["tol_g"]
    again = run()
    assert torch.equal(y, again[0]) and torch.equal(da, again[1]) and (dr is None or torch.equal(dr, again[2]))

    # the ops level: statistics in fp64, both outputs of the fused pass
    a2, r2 = a.to(dev), r.to(dev)
    sa = ops.instance_norm_stats(a2, B, V)
    assert sa.dtype == torch.float64 and sa.shape == (B, C, 2)
    assert torch.allclose(sa[..., 0].cpu(), a.double().reshape(B, V, C).mean(1), rtol=1e-14, atol=0)
    assert torch.allclose(sa[..., 1].cpu(), a.double().reshape(B, V, C).var(1, unbiased=False), rtol=1e-9, atol=0)
    sr = ops.instance_norm_stats(r2, B, V) if with_r else None
    y32, y16 = ops.instance_norm_apply(a2, sa, B, V, r2 if with_r else None, sr, slope, R.EPS, want32=True, want16=True)
    assert torch.equal(y32, y)
    print("bf16 output: worst error in bf16 ulps", R.bf16_check(y16.cpu(), ref["y"]))


def test_one_voxel_raises(dev):
    from micro_sam_amd import ops
    from micro_sam_amd.training import functional as HF
    x = torch.zeros(2, 8, device=dev)
    with pytest.raises(ValueError, match="more than 1"):
        ops.instance_norm_stats(x, 2, 1)
    with pytest.raises(ValueError, match="more than 1"):
        HF.instance_norm_act(x.reshape(2, 1, 1, 1, 8))
    with pytest.raises(ValueError):
        ops.instance_norm_stats(torch.zeros(4, 12, device=dev), 1, 4)         # C = 12
    with pytest.raises(ValueError):
        ops.instance_norm_stats(x.cpu(), 1, 2)
    with pytest.raises(TypeError):
        ops.instance_norm_stats(x.double(), 1, 2)
    assert torch.equal(ops.column_sums(torch.ones(1000, 8, device=dev)), torch.full((8,), 1000.0, device=dev))
