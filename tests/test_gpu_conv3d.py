"""``ops.conv3d_k3`` / ``ops.conv3d_k3_wgrad`` / ``training.functional.conv3d_k3`` (csrc/conv3d.hip) on the device, on the cases and within
the bounds of tests/conv3d_ref.py: the forward pass and the input gradient through W' against torch's Conv3d in fp64 on the bf16-rounded
operands, the autograd function's dX, dW and db against fp64 autograd (the last case runs the weight gradient's split path), the same
bits on every run, a frozen weight, and the wrapper's refusals."""
import pytest
import torch

import conv3d_ref as R

pytestmark = pytest.mark.gpu
IDS = dict(ids=lambda c: "x".join(map(str, c)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    err = (got.detach().double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst error / bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{what}: worst error / bound = {worst:.3f}"


@pytest.mark.parametrize("case", R.CASES, **IDS)
def test_forward_against_conv3d_fp64(dev, case):
    from micro_sam_amd import ops
    from micro_sam_amd._conv3d import tap_major
    B, D, H, W, Ci, Co = case
    x, w, bias, _ = R.make_case(case)
    want, bound = R.forward(case, x, w, bias)
    x16 = x.to(dev, torch.bfloat16)
    w16 = tap_major(w).to(dev, torch.bfloat16)
    b = torch.nn.functional.pad(bias.float(), (0, w16.shape[0] - Co)).to(dev)
    out = ops.conv3d_k3(x16, w16, b, B, D, H, W)
    assert out.shape == (B * D * H * W, w16.shape[0]) and out.dtype == torch.float32
    within(out[:, :Co], want, bound, f"forward {case}")
    assert not out[:, Co:].any()
    assert torch.equal(out, ops.conv3d_k3(x16, w16, b, B, D, H, W))
    into = torch.full_like(out, -1.0)
    assert ops.conv3d_k3(x16, w16, b, B, D, H, W, out=into) is into and torch.equal(into, out)


@pytest.mark.parametrize("case", R.CASES, **IDS)
def test_input_gradient_through_the_transposed_weight(dev, case):
    from micro_sam_amd import ops
    from micro_sam_amd._conv3d import tap_major_transposed
    B, D, H, W, Ci, Co = case
    _, w, _, dy = R.make_case(case)
    want, bound = R.input_gradient(case, dy, w)
    dx = ops.conv3d_k3(dy.to(dev, torch.bfloat16), tap_major_transposed(w).to(dev, torch.bfloat16), None, B, D, H, W)
    within(dx[:, :Ci], want, bound, f"dX {case}")
    assert not dx[:, Ci:].any()


@pytest.mark.parametrize("case", R.CASES + [R.AUTOGRAD_ONLY], **IDS)
def test_autograd_against_fp64(dev, case):
    from micro_sam_amd.training import functional as HF
    B, D, H, W, Ci, Co = case
    xs, w, bias, dy = R.make_case(case)
    (dx, dx_bound), (dw, dw_bound), (db, db_bound) = R.autograd(case)

    def run(train_weight: bool):
        x = xs.float().reshape(B, D, H, W, Ci).to(dev).requires_grad_()
        weight = torch.nn.Parameter(w.float().to(dev), requires_grad=train_weight)
        b = torch.nn.Parameter(bias.float().to(dev), requires_grad=train_weight)
        out = HF.conv3d_k3(x, weight, b)
        assert out.shape == (B, D, H, W, Co)
        out.backward(dy.float().reshape(B, D, H, W, Co).to(dev))
        return out.detach(), x.grad, weight.grad, b.grad
    out, gx, gw, gb = run(True)
    want, bound = R.forward(case, xs, w, bias)
    within(out.reshape(-1, Co), want, bound, f"forward {case}")
    within(gx.reshape(-1, Ci), dx, dx_bound, f"dX {case}")
    within(gw, dw, dw_bound, f"dW {case}")
    within(gb, db, db_bound, f"db {case}")
    again = run(True)
    assert all(torch.equal(p, q) for p, q in zip((out, gx, gw, gb), again))                 # the same bits on every run
    _, fx, fw, fb = run(False)                                                              # a frozen weight: dX alone, the same bits
    assert fw is None and fb is None and torch.equal(fx, gx)


def test_wrapper_refusals(dev):
    from micro_sam_amd import ops
    from micro_sam_amd._conv3d import padded_k
    x = torch.zeros(2 * 2 * 4 * 4, 16, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(16, padded_k(16), dtype=torch.bfloat16, device=dev)
    assert ops.conv3d_k3(x, w, None, 2, 2, 4, 4).shape == (64, 16)
    with pytest.raises(ValueError):
        ops.conv3d_k3(x, w, None, 2, 2, 4, 3)                                # B D H W is not the number of rows
    with pytest.raises(ValueError):
        ops.conv3d_k3(x, w, None, 2, 0, 4, 4)
    with pytest.raises(ValueError):
        ops.conv3d_k3(x[:, :12].contiguous(), w[:, :padded_k(12)].contiguous(), None, 2, 2, 4, 4)      # Ci = 12
    with pytest.raises(ValueError):
        ops.conv3d_k3(x.cpu(), w, None, 2, 2, 4, 4)
    with pytest.raises(TypeError):
        ops.conv3d_k3(x.float(), w, None, 2, 2, 4, 4)
    with pytest.raises(TypeError):
        ops.conv3d_k3(x, w.float(), None, 2, 2, 4, 4)
    with pytest.raises(ValueError):
        ops.conv3d_k3(x, w, torch.zeros(8, device=dev), 2, 2, 4, 4)          # bias [Co']
    with pytest.raises(ValueError):
        ops.conv3d_k3(x, w[:8].contiguous(), None, 2, 2, 4, 4)               # Co' % 16
    with pytest.raises(ValueError):
        ops.conv3d_k3_wgrad(x, torch.zeros(64, 12, dtype=torch.bfloat16, device=dev), 2, 2, 4, 4)
