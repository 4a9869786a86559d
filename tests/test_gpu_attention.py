"""window_attention_kernel and global_attention_kernel (csrc/attention.hip) on the device, called directly through ops.window_attention /
ops.global_attention on generated 16-bit q, k, v (no GEMM in front), in all four builds of each - stored head_dim 64 / 96 (80 real
channels) times bf16 / fp16 - against the fp64 attention of tests/attention_ref.py, computed on the device one (image, head) at a time,
and within its ELEMENTWISE rounding bound (2 u (P @ |v|) plus small terms; derivation in attention_ref's docstring).  B = 2 images of 3
heads with independent data per (image, head): the smallest shape that exercises the decomposition of the workgroup index.

tests/test_attention_ref_host.py proves that each of the defects these kernels are prone to (a rel-pos index off by one, swapped tables
or sign, a dropped key tile, two V rows swapped, the bias-only padding tokens taken as zero or masked, heads or images crossed, the
padded head_dim's scale) is at least 4 bounds from the reference on one of these generators, so a kernel with such a defect fails here.

Every case prints its max |got - ref| / bound (pytest -s); a value above 1 fails the test.  The same kernel source executed on the host
(tests/test_attention_kernel_host_emulation.py) reaches 0.46 - 0.64 of the bound.  The device values have NOT been recorded yet:
profiles/r09_attention_err_over_bound.md holds the host values and the place for the device table.
"""
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

B, HEADS = 2, 3
CASES = [(kind, dtype, hs, gen) for kind in ("window", "global") for dtype in (torch.bfloat16, torch.float16) for hs in (64, 96)
         for gen in R.GENERATORS[kind]]
IDS = [f"{kind}-{'fp16' if dtype == torch.float16 else 'bf16'}-hd{hs}-{gen}" for kind, dtype, hs, gen in CASES]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import ops
    return ops, torch.device("cuda")


def _call(ops, kind, inp):
    if kind == "window":
        return ops.window_attention(inp["q"], inp["k"], inp["v"], inp["rel_h"], inp["rel_w"], inp["qkv_bias"], scale=inp["scale"])
    return ops.global_attention(inp["q"], inp["k"], inp["v"], inp["rel_h"], inp["rel_w"], scale=inp["scale"])


def _within(where, err, bound, rows=None):
    """|got - ref| <= bound on ``rows`` (a bool mask over the B * 4096 tokens, or everything); the message names the worst element."""
    if rows is not None:
        err, bound = err[rows], bound[rows]
    bad = err > bound
    if bool(bad.any()):
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.inf, 0.0))
        i = int(ratio.argmax())
        r, c = divmod(i, err.shape[1])
        pytest.fail(f"{where}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst |got - ref| / bound = "
                    f"{float(ratio.reshape(-1)[i]):.3g} at row {r} (of the rows compared) channel {c}: err {float(err[r, c]):.3g}, "
                    f"bound {float(bound[r, c]):.3g}")


@pytest.mark.parametrize("kind,dtype,hs,gen", CASES, ids=IDS)
def test_attention_kernel_within_the_rounding_bound(env, kind, dtype, hs, gen):
    ops, dev = env
    inp = {n: (t.to(dev) if torch.is_tensor(t) else t) for n, t in R.make_inputs(kind, gen, dtype, hs, B, HEADS, seed=5).items()}
    got = _call(ops, kind, inp)
    again = _call(ops, kind, inp)
    assert got.shape == (B * R.TOK, HEADS * hs) and got.dtype == dtype
    assert bool(torch.isfinite(got).all())
    ref, bound = R.attention_ref(kind, inp)
    err = (got.double() - ref).abs()
    live = bound > 0
    print(f"\n{kind} {str(dtype)[6:]} hd{hs} {gen}: max |got - ref| / bound = {float((err[live] / bound[live]).max()):.3f}")
    _within("whole output", err, bound)
    if kind == "window":
        t = torch.arange(B * R.TOK, device=dev) % R.TOK
        y, x = t // 64, t % 64
        _within("edge windows (y >= 56 or x >= 56)", err, bound, (y >= 56) | (x >= 56))
        _within("last query tile of the windows (queries 192..195)", err, bound, (y % 14 == 13) & (x % 14 >= 10))
    if hs == 96:
        assert float(got.reshape(-1, HEADS, hs)[..., 80:].abs().max()) == 0.0           # padded channels: exactly zero
    assert torch.equal(got, again)                                                         # no atomics: run to run identical
    one = {n: (t[1:2].contiguous() if n in ("q", "k", "v") else t) for n, t in inp.items()}
    assert torch.equal(_call(ops, kind, one), got[R.TOK:])                                 # image 1 alone = image 1 of the batch
