"""msam_adapter_bf16 (csrc/adapter.hip) on the device through ``ops.adapter_``: the cases and the derived bound of tests/adapter_ref.py in both
16-bit types, bit-identical repeats, row strides larger than D, alpha = 0 and Wu = 0, and the refusals of the tensor boundary."""
import pytest
import torch

import adapter_ref as R

pytestmark = pytest.mark.gpu
IDS = dict(ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
EXTRA = [(33, 128, 96), (4099, 768, 64)]            # the half-used slab (P = 96); more tiles than compute units, with a ragged last one


def device_operands(ops, dtype, alpha, pad_y=0, pad_x=0):
    dt, dev = R.DTYPES[dtype], "cuda"
    y, x = ops["y"], ops["x"]
    Rr, D = y.shape
    ybuf = torch.full((Rr, D + pad_y), float("nan"), dtype=dt, device=dev)
    ybuf[:, :D] = y.to(dt)
    xbuf = torch.full((Rr, D + pad_x), -777.0, dtype=torch.float32, device=dev)
    xbuf[:, :D] = x.to(torch.float32)
    f = lambda t: t.to(torch.float32).to(dev).contiguous()
    h = lambda t: t.to(dt).to(dev).contiguous()
    return dict(x=xbuf[:, :D], y=ybuf[:, :D], wd=h(ops["wd"]), bd=f(ops["bd"]), wu=h(ops["wu"]), bu=f(ops["bu"]),
                alpha=torch.tensor([alpha], dtype=torch.float32, device=dev)), xbuf


def run(ops, dtype, alpha=R.ALPHA, **pads):
    from micro_sam_amd import ops as O
    args, xbuf = device_operands(ops, dtype, alpha, **pads)
    out = O.adapter_(**args)
    assert out is args["x"]
    D = ops["y"].shape[1]
    assert bool((xbuf[:, D:] == -777.0).all())
    return xbuf[:, :D].cpu()


def within(got, want, bound):
    err = (got.double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    assert bool((err <= bound).all()), f"worst error / bound = {worst:.3f}"
    return worst


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.CASES + EXTRA, **IDS)
def test_against_fp64(case, dtype):
    ops = R.make_case(case, dtype)
    want, bound = R.forward(alpha=R.ALPHA, dtype=dtype, **ops)
    got = run(ops, dtype)
    print("adapter", case, dtype, "worst error / bound", within(got, want, bound))
    assert torch.equal(got, run(ops, dtype))                                 # the same bits on every run


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_row_strides_larger_than_d(dtype):
    ops = R.make_case((129, 768, 64), dtype)
    want, bound = R.forward(alpha=R.ALPHA, dtype=dtype, **ops)
    got = run(ops, dtype, pad_y=24, pad_x=5)
    within(got, want, bound)
    assert torch.equal(got, run(ops, dtype))                                 # the strides change no bit


def test_alpha_zero_and_wu_zero():
    ops = R.make_case((129, 768, 64), "bf16")
    got = run(ops, "bf16", alpha=0.0)
    assert torch.equal(got, ops["x"].float() + ops["y"].float())             # exactly x + y: one fp32 add
    got = run(dict(ops, wu=torch.zeros_like(ops["wu"])), "bf16")
    want = ops["x"] + ops["y"] + R.ALPHA * ops["bu"]
    within(got, want, 2 * R.U * (ops["x"].abs() + ops["y"].abs() + R.ALPHA * ops["bu"].abs()))


def test_refusals_at_the_tensor_boundary():
    from micro_sam_amd import ops as O
    args, xbuf = device_operands(R.make_case((17, 128, 64), "bf16"), "bf16", 1.0)
    before = xbuf.clone()
    bad = [dict(alpha=args["alpha"].cpu()), dict(alpha=torch.ones(2, device="cuda")), dict(wd=args["wd"][:16].contiguous(), bd=args["bd"][:16]),
           dict(wu=args["wu"].to(torch.float16)), dict(y=args["y"].float()), dict(x=args["x"].to(torch.bfloat16)), dict(bd=args["bd"][:32]),
           dict(bu=args["bu"].double()), dict(y=args["y"][:, :64], x=args["x"][:, :64]), dict(y=args["y"][1:])]
    for change in bad:
        with pytest.raises((ValueError, TypeError)):
            O.adapter_(**dict(args, **change))
    torch.cuda.synchronize()
    assert torch.equal(xbuf, before)
