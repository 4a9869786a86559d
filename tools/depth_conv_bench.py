"""Time of the 3-d adapter's depth convolution on the device (profiles/r09_sam3d.md), forward + backward (dX, dW, db), at the workload's
shape B = 1, D = 8, T = 4096, Ci = Co = 384 (one adapter of vit_b on a volume of eight 1024 x 1024 slices), in three forms:

  (a) ``training.functional.depth_conv3`` - csrc/conv3d.hip's tile body in its depth geometry, on token-major rows;
  (b) what the library could do before that kernel: ``torch.cat`` of the three shifted, zero-padded copies of x, [M, 3 Ci] fp32, and
      ``training.functional.linear`` on it;
  (c) ``F.conv3d`` on bf16 channels-first tensors, with the permute + cast to channels-first before it and the permute + cast back
      after it (what the reference's ``NDBlockWrapper`` does, under bf16 autocast).

Every figure is the median over ``--reps`` windows of at least ``--inner`` calls and at least ``--window-ms`` milliseconds each, between two
device events, after ``--warmup`` calls; the forms alternate window by window (tools/window_timer.py; profiles/r09_sam3d.md's figures came from
fixed windows of 5 calls, about 2 ms each, and are not comparable).  "bytes": what each form's launches read and write, every operand counted once per launch that
touches it, computed from the shapes below (``algorithm_bytes``) - not a counter reading.  The line "source" names the kernel sources
the numbers belong to.

    python tools/depth_conv_bench.py [--reps 7] [--inner 3] [--window-ms 200] [--warmup 3] [--depth 8]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

import window_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def algorithm_bytes(m: int, ci: int, co: int):
    """Bytes per forward + backward call of the three forms (module docstring)."""
    w = 3 * ci * co * 2
    a = (m * ci * 4 + 2 * m * ci * 2) + (m * ci * 2 + w + m * co * 4)                  # cast + transpose of x; the kernel
    a += (m * co * 4 + 2 * m * co * 2) + (m * co * 2 + w + m * ci * 4)                 # cast + transpose of dY (+ db); dX by the kernel
    a += 3 * (m * co * 2 + m * ci * 2) + 3 * ci * co * 4                               # dW: three products over the rows
    k = 3 * ci
    b = (m * ci * 4 + m * k * 4) + (m * k * 4 + 2 * m * k * 2) + (m * k * 2 + w + m * co * 4)      # cat; cast + transpose; product
    b += (m * co * 4 + 2 * m * co * 2) + (m * co * 2 + w + m * k * 4) + (m * co * 2 + m * k * 2 + k * co * 4)   # dY; d cols; dW
    b += m * k * 4 + m * ci * 4                                                       # the three slices of d cols added into dX
    c = (m * ci * 4 + m * ci * 2) + (m * ci * 2 + w + m * co * 2) + (m * co * 2 + m * co * 4)      # to channels-first; conv; back
    c += (m * co * 4 + m * co * 2) + (m * co * 2 + w + m * ci * 2) + (m * co * 2 + m * ci * 2 + w) + (m * ci * 2 + m * ci * 4)
    return {"a": a, "b": b, "c": c}


def main():
    ap = argparse.ArgumentParser()
    window_timer.add_arguments(ap)
    ap.add_argument("--depth", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/depth_conv_bench.py measures on the device; there is none")
    import bench
    from micro_sam_amd.training import functional as HF
    B, D, S, Ci, Co = 1, args.depth, 64, 384, 384
    T, M = S * S, B * D * S * S
    print(json.dumps({"source": bench.csrc_sha16(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner,
                      "window_ms": args.window_ms, "warmup": args.warmup, "shape": {"B": B, "D": D, "T": T, "Ci": Ci, "Co": Co, "M": M}}), flush=True)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B * D, S, S, Ci, generator=g).cuda().requires_grad_()
    weight = torch.nn.Parameter((torch.randn(Co, Ci, 3, 1, 1, generator=g) * (3 * Ci) ** -0.5).cuda())
    bias = torch.nn.Parameter(torch.randn(Co, generator=g).cuda())
    w16 = torch.nn.Parameter(weight.detach().to(torch.bfloat16))
    b16 = torch.nn.Parameter(bias.detach().to(torch.bfloat16))
    dy = torch.randn(B * D, S, S, Co, generator=g).cuda()
    leaves = (x, weight, bias, w16, b16)
    kept = {}

    def finish(name, out):
        for t in leaves:
            t.grad = None
        out.backward(dy)
        kept[name] = (out.detach(), x.grad, weight.grad if weight.grad is not None else w16.grad.float())

    def form_a():
        finish("a", HF.depth_conv3(x, weight, bias, D))

    def form_b():
        v = x.reshape(B, D, T, Ci)
        z = torch.zeros_like(v[:, :1])
        cols = torch.cat([torch.cat([z, v[:, :-1]], 1), v, torch.cat([v[:, 1:], z], 1)], dim=-1)      # [B, D, T, 3 Ci]: the im2col copy
        w2 = weight.reshape(Co, Ci, 3).permute(0, 2, 1).reshape(Co, 3 * Ci)
        finish("b", HF.linear(cols, w2, bias).reshape(B * D, S, S, Co))

    def form_c():
        v = x.reshape(B, D, S, S, Ci).permute(0, 4, 1, 2, 3).to(torch.bfloat16).contiguous()
        y = F.conv3d(v, w16, b16, padding="same")
        finish("c", y.permute(0, 2, 3, 4, 1).float().contiguous().reshape(B * D, S, S, Co))

    forms = {"a": form_a, "b": form_b, "c": form_c}
    timed = window_timer.compare(forms, args)                           # (a library without this convolution: the other forms still count)
    nbytes = algorithm_bytes(M, Ci, Co)
    flops = 2.0 * M * 3 * Ci * Co * 3                                   # forward, dX, dW
    row = {"flops_forward_backward": flops, "failed": timed.pop("failed", {})}
    for k in forms:
        med = timed[k]["ms"]
        row[k] = dict(timed[k], algorithm_bytes=nbytes[k], bytes_per_s=nbytes[k] / (med * 1e-3), flops_per_s=flops / (med * 1e-3))
    for k in forms:
        if k != "a":
            row[k]["ms_over_a"] = row[k]["ms"] / row["a"]["ms"]
            row[k]["difference_from_a_over_max"] = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(kept[k], kept["a"])]
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
