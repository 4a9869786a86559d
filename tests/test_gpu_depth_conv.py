"""``ops.depth_conv3`` / ``training.functional.depth_conv3`` (csrc/conv3d.hip) on the device, on the cases and within the bounds of
tests/depth_conv_ref.py: the forward pass and the input gradient through W' against torch's Conv3d in fp64 on the bf16-rounded operands,
dX, dW and db of the autograd function against the fp64 autograd of the same restatement, and identical bits on a second run.  One more
case (SPLIT_CASE) takes the weight gradient through the in-place split-K products, which the small cases are too short for."""
import pytest
import torch

import depth_conv_ref as R

pytestmark = pytest.mark.gpu

GRIDS = {80: (8, 10), 128: (8, 16), 200: (10, 20), 4096: (64, 64)}       # T = H W of the autograd function's [B D, H, W, C]
SPLIT_CASE = (1, 3, 4096, 128, 128)                                     # contractions of 8192 and 12288 rows: split-K, read in place
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def ref(case):
    """The operands and the fp64 results of a case, computed once and shared."""
    if case not in _REF:
        x, w, bias, dy = R.make_case(case)
        _REF[case] = dict(x=x, w=w, bias=bias, dy=dy, fwd_bias=R.forward(case, x, w, bias), fwd=R.forward(case, x, w, None),
                          grads=R.autograd(case, x, w, bias, dy))
    return _REF[case]


def within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str):
    err = (got.detach().double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(what, "worst error / bound =", worst)
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_forward_against_conv3d_fp64(dev, case, with_bias):
    from micro_sam_amd import ops
    from micro_sam_amd._depthconv import tap_major
    B, D, T, Ci, Co = case
    r = ref(case)
    x16 = r["x"].to(dev, torch.bfloat16)
    w16 = tap_major(r["w"]).to(dev, torch.bfloat16)
    bias = r["bias"].to(dev, torch.float32) if with_bias else None
    want, bound = r["fwd_bias" if with_bias else "fwd"]
    out = ops.depth_conv3(x16, w16, bias, B, D, T)
    assert out.shape == (B * D * T, Co) and out.dtype == torch.float32
    within(out, want, bound, f"forward {case}")
    assert torch.equal(out, ops.depth_conv3(x16, w16, bias, B, D, T))
    into = torch.full_like(out, -777.0)
    assert ops.depth_conv3(x16, w16, bias, B, D, T, out=into) is into and torch.equal(into, out)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
def test_input_gradient_through_the_transposed_weight(dev, case):
    from micro_sam_amd import ops
    from micro_sam_amd._depthconv import tap_major_transposed
    B, D, T, Ci, Co = case
    r = ref(case)
    wt = tap_major_transposed(r["w"])
    wt = torch.cat([wt, torch.zeros((Ci + 127) // 128 * 128 - Ci, 3 * Co, dtype=wt.dtype)])      # rows padded to the tile, as functional does
    dx = ops.depth_conv3(r["dy"].to(dev, torch.bfloat16), wt.to(dev, torch.bfloat16), None, B, D, T)
    want, bound = r["grads"][0]
    within(dx[:, :Ci], want, bound, f"dX {case}")
    assert not dx[:, Ci:].any()


@pytest.mark.parametrize("case", R.CASES + [SPLIT_CASE], ids=lambda c: "x".join(map(str, c)))
def test_autograd_function_against_fp64_autograd(dev, case):
    from micro_sam_amd.training import functional as HF
    B, D, T, Ci, Co = case
    r = ref(case)
    h, w_ = GRIDS[T]
    dy = r["dy"].to(dev, torch.float32).reshape(B * D, h, w_, Co)
    runs = []
    for _ in range(2):
        x = r["x"].to(dev, torch.float32).reshape(B * D, h, w_, Ci).requires_grad_()
        weight = torch.nn.Parameter(r["w"].to(dev, torch.float32))
        bias = torch.nn.Parameter(r["bias"].to(dev, torch.float32))
        out = HF.depth_conv3(x, weight, bias, D)
        (out * dy).sum().backward()
        runs.append((out.detach(), x.grad, weight.grad, bias.grad))
    out, dx, dw, db = runs[0]
    assert out.shape == (B * D, h, w_, Co) and dw.shape == (Co, Ci, 3, 1, 1)
    within(out.reshape(-1, Co), *r["fwd_bias"], f"forward {case}")
    (wdx, bdx), (wdw, bdw), (wdb, bdb) = r["grads"]
    within(dx.reshape(-1, Ci), wdx, bdx, f"dX {case}")
    within(dw, wdw, bdw, f"dW {case}")
    within(db, wdb, bdb, f"db {case}")
    if D == 1:
        assert not dw[:, :, 0].any() and not dw[:, :, 2].any()             # no neighbour: the outer taps get exact zeros
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                           # the same bits on every run
    # a frozen weight: the input gradient alone, the same bits
    x = r["x"].to(dev, torch.float32).reshape(B * D, h, w_, Ci).requires_grad_()
    frozen = torch.nn.Parameter(r["w"].to(dev, torch.float32), requires_grad=False)
    HF.depth_conv3(x, frozen, None, D).backward(dy)
    assert torch.equal(x.grad, dx) and frozen.grad is None


def test_wrapper_refusals(dev):
    from micro_sam_amd import ops
    x = torch.zeros((64, 64), dtype=torch.bfloat16, device=dev)
    w = torch.zeros((128, 192), dtype=torch.bfloat16, device=dev)
    assert ops.depth_conv3(x, w, None, 2, 2, 16).shape == (64, 128)
    with pytest.raises(ValueError):
        ops.depth_conv3(x, w, None, 2, 2, 15)                              # B D T is not the number of rows
    with pytest.raises(ValueError):
        ops.depth_conv3(x, w, None, 2, 0, 16)
    with pytest.raises(TypeError):
        ops.depth_conv3(x.float(), w, None, 2, 2, 16)
    with pytest.raises(ValueError):
        ops.depth_conv3(x, w[:64].contiguous(), None, 2, 2, 16)             # Co % 128
    with pytest.raises(ValueError):
        ops.depth_conv3(x[:, :32].contiguous(), w[:, :96].contiguous(), None, 2, 2, 16)       # Ci % 64
    with pytest.raises(ValueError):
        ops.depth_conv3(x, w, torch.zeros(64, device=dev), 2, 2, 16)       # bias [Co]
    with pytest.raises(ValueError):
        ops.depth_conv3(x.cpu(), w, None, 2, 2, 16)
