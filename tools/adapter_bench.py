"""Times of the AdaptFormer branch on the device (profiles/peft_adapter.md): the fused launch (ops.adapter_, csrc/adapter.hip) against the same
branch composed from two msam_gemm_bf16 calls (ReLU, then residual; the bottleneck padded from 64 to the GEMM's 128-column tile, alpha folded
into the up projection) plus the add of y that no GEMM epilogue takes, at vit_b's width for B = 1 and B = 8 images; and the whole encoder with
and without adapters in all twelve blocks.  Device events around windows of at least ``--window`` seconds, fused and composed windows
alternating, the median and the spread of ``--repeats`` windows.  Writes one JSON line (and ``--out``).

    python tools/adapter_bench.py --out peft_adapter.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_MEASURED = 6.29e12        # bytes / s, a float4 copy on this chip (8.0e12 nominal)


def window(fn, seconds: float):
    """-> microseconds per call over a window of at least ``seconds`` (device events; the count is fixed from a short calibration)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        fn()
    b.record()
    b.synchronize()
    n = max(10, int(seconds * 1e3 / max(a.elapsed_time(b) / 10, 1e-4)))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def summary(xs):
    return {"median_us": round(statistics.median(xs), 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2)}


def branch(B: int, args):
    from micro_sam_amd import ops
    from micro_sam_amd._lib import ACT_RELU
    R, D, P = B * 4096, 768, 64
    g = torch.Generator().manual_seed(B)
    dev = "cuda"
    y = torch.randn(R, D, generator=g).to(torch.bfloat16).to(dev)
    wd = (torch.randn(P, D, generator=g) * D ** -0.5).to(torch.bfloat16).to(dev)
    wu = (torch.randn(D, P, generator=g) * P ** -0.5).to(torch.bfloat16).to(dev)
    bd, bu = (torch.randn(P, generator=g) * 0.5).to(dev), torch.randn(D, generator=g).to(dev)
    alpha = torch.tensor([0.75], device=dev)
    x0 = (torch.randn(R, D, generator=g) * 3).to(dev)
    # composed: the bottleneck padded to the GEMM's 128-column tile with zero rows / columns, alpha folded into the up projection
    wd2 = torch.zeros(128, D, dtype=torch.bfloat16, device=dev)
    wd2[:P] = wd
    bd2 = torch.zeros(128, device=dev)
    bd2[:P] = bd
    wu2 = torch.zeros(D, 128, dtype=torch.bfloat16, device=dev)
    wu2[:, :P] = (wu.float() * 0.75).to(torch.bfloat16)
    bu2 = bu * 0.75
    hid = torch.empty(R, 128, dtype=torch.bfloat16, device=dev)
    xf, xc = x0.clone(), x0.clone()

    def fused():
        ops.adapter_(xf, y, wd, bd, wu, bu, alpha)

    def two_gemms():
        ops.gemm(y, wd2, bd2, act=ACT_RELU, out=hid)
        ops.gemm(hid, wu2, bu2, resid=xc, out=xc)

    def composed():
        two_gemms()
        xc.add_(y)
    # the two forms agree (one application each, from the same x)
    fused()
    composed()
    torch.cuda.synchronize()
    agree = float((xf - xc).abs().max())
    t = {"fused": [], "two_gemms": [], "composed": []}
    for _ in range(args.repeats):
        for name, fn in (("fused", fused), ("two_gemms", two_gemms), ("composed", composed)):
            xf.copy_(x0)
            xc.copy_(x0)                                   # (the stream is accumulated into: keep it finite over a window)
            t[name].append(window(fn, args.window))
    floor = R * D * 10 / HBM_MEASURED * 1e6
    return {"R": R, "D": D, "P": P, "fused": summary(t["fused"]), "two_gemms": summary(t["two_gemms"]), "composed_with_add_y": summary(t["composed"]),
            "byte_floor_us": round(floor, 2), "fused_share_of_floor": round(floor / statistics.median(t["fused"]), 3),
            "max_abs_difference_fused_vs_composed": agree}


def encoder(B: int, args):
    from micro_sam_amd import util
    from micro_sam_amd.models import peft_sam
    from micro_sam_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict("vit_b", 0)
    plain = util.get_sam_model("vit_b", device="cuda", state_dict=sd).model.image_encoder
    adapted = util.get_sam_model("vit_b", device="cuda", state_dict=sd, flexible_load_checkpoint=True,
                                 peft_kwargs=dict(peft_module=peft_sam.AdaptFormer)).model
    with torch.no_grad():                                  # the flexible load leaves the wrapped MLPs at their initial values: copy them
        for a, b in zip(adapted.image_encoder.blocks, plain.blocks):
            a.mlp.mlp_proj.load_state_dict(b.mlp.state_dict())
            a.mlp.up_proj.weight.normal_(0, 0.1)
    adapted.image_encoder.invalidate()
    x = torch.randn(B, 3, 1024, 1024, generator=torch.Generator().manual_seed(5)).cuda()
    t = {"plain": [], "adapted": []}
    for _ in range(args.repeats):
        for name, enc in (("plain", plain), ("adapted", adapted.image_encoder)):
            t[name].append(window(lambda: enc(x), args.window))
    return {"B": B, "plain": summary(t["plain"]), "adapters_in_12_blocks": summary(t["adapted"]),
            "added_us_per_block": round((statistics.median(t["adapted"]) - statistics.median(t["plain"])) / 12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adapter_bench: needs the GPU (a CPU run gives no time)")
    res = {"branch": [branch(B, args) for B in (1, 8)], "encoder": [encoder(B, args) for B in (1, 8)],
           "window_s": args.window, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
