"""Timing of the device label transform (``training.label_transform.PerObjectDistanceTransform`` -> ``ops.distance_targets``,
csrc/labelprops.hip) next to the host restatement of torch_em's per-object loop (tests/distance_targets_ref.py) on the same image: a
512 x 512 seeded Voronoi label image with about 200 objects (tests/labelprops_ref.voronoi).  The device figure is a host clock around the
whole call from a numpy array - connected components on the host, upload, relabelling, the kernels, and a device synchronise - and, next
to it, ``ops.distance_targets`` alone on labels already on the device; medians and spread over --reps calls after a warm-up.

    python tools/distance_targets_bench.py [--reps 30] [--size 512] [--seeds 240]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--seeds", type=int, default=240)
    args = ap.parse_args()
    import distance_targets_ref as R
    import labelprops_ref as LR
    from micro_sam_amd import ops
    from micro_sam_amd.training.label_transform import PerObjectDistanceTransform
    if not torch.cuda.is_available():
        raise SystemExit("distance_targets_bench: needs a GPU (a CPU run gives no timing)")
    seg = LR.voronoi(args.size, args.size, args.seeds, 5)
    want, lab = R.transform(seg, apply_label=True)
    n = int(lab.max())
    tr = PerObjectDistanceTransform(instances=True)
    got = tr(seg)
    err = float(np.abs(got.astype(np.float64) - want).max())
    lab_dev = torch.from_numpy(lab).cuda()
    res = {"size": args.size, "objects": n, "background_share": round(float((lab == 0).mean()), 3), "max_abs_error_vs_host": err,
           "device_transform_from_numpy": _stats(_wall(lambda: tr(seg), args.reps)),
           "device_transform_without_apply_label": _stats(_wall(lambda: PerObjectDistanceTransform(instances=True, apply_label=False)(lab), args.reps)),
           "ops_distance_targets_labels_on_device": _stats(_wall(lambda: ops.distance_targets(lab_dev, n_objects=n), args.reps))}
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        R.transform(seg, apply_label=True)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_restatement"] = _stats(host)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        R.distance_targets(lab, n)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_restatement_without_apply_label"] = _stats(host)
    res["ratio_host_over_device"] = round(res["host_restatement"]["median_ms"] / res["device_transform_from_numpy"]["median_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
