"""Timing and accuracy of visualization.compute_pca on the device (profiles/r07_embedding_pca.md): for one 2-d embedding and for a 16-slice
stack (synthetic embeddings of tests/embedding_pca_ref.py, already on the device) the wall time of a call (synchronised), the device time
of the pca kernels and of all kernels of the call (torch profiler), the host eigen step (the copy of the Gram matrices, np.linalg.eigh, the
upload of the components; timed after a synchronisation), next to sklearn's PCA - the CPU restatement - on the same float32 input; then
the error figures of tests/test_gpu_visualization.py on its numeric shapes.

    python tools/pca_bench.py [--reps 10] [--no-cpu]
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


def _device_times(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    total = pca = 0.0
    each = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if ev.device_type is not None and str(ev.device_type).endswith("CUDA"):
            total += t
            if "pca_" in ev.key:
                pca += t
                name = ev.key[ev.key.index("pca_"):].split("(")[0].split("<")[0]
                each[name] = each.get(name, 0.0) + t / 1e3
    return pca / 1e3, total / 1e3, each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import embedding_pca_ref as REF
    from micro_sam_amd import visualization as VIS

    eig_ms = []
    components = VIS._components

    def timed_components(gram, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = components(gram, k)
        torch.cuda.synchronize()
        eig_ms.append((time.perf_counter() - t0) * 1e3)
        return out
    VIS._components = timed_components

    one = REF.synthetic_embedding(320, 256, 64, 64)[None]
    stack = np.stack([REF.synthetic_embedding(320, 256, 64, 64, noise_seed=z)[None] for z in range(16)])
    for name, emb, units in (("2d 256 x 64 x 64", one, 1), ("3d 16 x 256 x 64 x 64", stack, 16)):
        dev = torch.from_numpy(emb).cuda()
        VIS.compute_pca(dev)
        torch.cuda.synchronize()
        walls, eigs = [], []
        for _ in range(args.reps):
            del eig_ms[:]
            t0 = time.perf_counter()
            VIS.compute_pca(dev)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            eigs.append(sum(eig_ms))
        try:
            k_pca, k_all, each = _device_times(lambda: VIS.compute_pca(dev))
        except Exception as exc:          # (profiler unavailable: wall times only)
            print("profiler:", exc)
            k_pca, k_all, each = float("nan"), float("nan"), {}
        row = {"case": name, "units": units, "wall_ms_median": float(np.median(walls)), "host_eigh_ms_median": float(np.median(eigs)),
               "pca_kernels_ms": k_pca, "all_kernels_ms": k_all, "pca_kernels_ms_per_unit": k_pca / units, "kernels_ms": each}
        if not args.no_cpu:
            t0 = time.perf_counter()
            REF.compute_pca(emb, 3, True, np.float32)
            row["cpu_sklearn_float32_s"] = time.perf_counter() - t0
        print(json.dumps(row), flush=True)
    VIS._components = components

    for c, h, w in REF.SHAPES:
        emb = REF.synthetic_embedding(c + h, c, h, w)[None]
        dev = torch.from_numpy(emb).cuda()
        err, r = REF.check_float(VIS.compute_pca(dev, as_rgb=False).cpu().numpy(), emb)
        frac = REF.check_rgb(VIS.compute_pca(dev).cpu().numpy(), emb)
        print(json.dumps({"shape": [c, h, w], "float_error": err, "r": r, "ratio": err / r, "uint8_differing": frac}), flush=True)


if __name__ == "__main__":
    main()
