"""Timing of ``ops.label_props`` (csrc/labelprops.hip) on the device (profiles/r10_label_props.md): a 1024 x 1024 seeded Voronoi label
image with about 300 objects and a background band (tests/labelprops_ref.voronoi), labels and ids already on the device.  Per variant
the time of a call between device events (median and spread over --reps calls after a warm-up), in a separate pass the device time of
every kernel of one call (torch profiler), and next to them the host restatement on the same image (tests/labelprops_ref.label_props:
scipy's exact EDT + a loop over the objects) and ``util.get_centers_and_bounding_boxes`` from a numpy array (upload, call, download).

    python tools/label_props_bench.py [--reps 50] [--size 1024] [--seeds 350]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _event_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _kernel_times(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if ev.device_type is not None and str(ev.device_type).endswith("CUDA") and t > 0:
            rows[ev.key[:60]] = round(t / 1e3, 4)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--seeds", type=int, default=350)
    args = ap.parse_args()
    import labelprops_ref as R
    from micro_sam_amd import ops, util
    sha = hashlib.sha256(open(os.path.join(ROOT, "micro_sam_amd", "csrc", "labelprops.hip"), "rb").read()).hexdigest()[:16]
    seg = R.voronoi(args.size, args.size, args.seeds, 5)
    t0 = time.perf_counter()
    want = R.label_props(seg)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.label_props(seg)
    host_s = min(host_s, time.perf_counter() - t0)
    labels = torch.from_numpy(seg).cuda()
    ids = torch.from_numpy(want["ids"].astype(np.int32)).cuda()
    got = ops.label_props(labels, ids)
    same = all(np.array_equal(getattr(got, k).cpu().numpy(), want[k]) for k in ("area", "bbox", "coord_sum", "center"))
    print(json.dumps({"labelprops_hip_sha256_16": sha, "size": args.size, "objects": int(len(want["ids"])), "background_share": float((seg == 0).mean()),
                      "equal_to_restatement": bool(same), "host_restatement_s": host_s, "device": torch.cuda.get_device_name(0)}), flush=True)
    variants = {"label_props(ids given)": lambda: ops.label_props(labels, ids),
                "label_props(ids=None: torch.unique)": lambda: ops.label_props(labels),
                "label_props(centers=False)": lambda: ops.label_props(labels, ids, centers=False),
                "edt_squared(labels != 0)": lambda: ops.edt_squared(labels),
                "util.get_centers_and_bounding_boxes(numpy)": lambda: util.get_centers_and_bounding_boxes(seg)}
    for name, fn in variants.items():
        ms = _event_times(fn, args.reps)
        row = {"variant": name, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_p90": float(np.percentile(ms, 90)), "reps": args.reps}
        print(json.dumps(row), flush=True)
    for name in ("label_props(ids given)", "edt_squared(labels != 0)"):
        try:
            print(json.dumps({"kernels_ms_of_one_call": name, **_kernel_times(variants[name])}), flush=True)
        except Exception as exc:          # (profiler unavailable: event times only)
            print("profiler:", exc, flush=True)


if __name__ == "__main__":
    main()
