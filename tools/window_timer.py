"""The window timer of tools/conv3d_bench.py and tools/depth_conv_bench.py: after ``warmup`` calls of every form, ``reps`` windows per form
of at least ``inner`` calls and at least ``window_ms`` milliseconds each, between two device events; the forms alternate window by window,
so every form sees the same machine.  A window of a few milliseconds would measure the clock and the scheduler as much as the kernels
(profiles/r09_sam3d.md saw 40 % outliers with 5-call windows, profiles/r10_simple_sam3d.md under 1 % with 200 ms ones)."""
import numpy as np
import torch


def add_arguments(ap) -> None:
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=200.0)


def window(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner                                    # ms per call


def calls_per_window(fn, args, cap: int = 20000) -> int:
    """The calls a window needs to last ``window_ms``: grown until a window of that many calls is MEASURED to last that long - a window of
    three calls costs more per call than a long one, so its time alone would size the windows too short.  (``cap``: a call the clock reads
    as next to nothing must not ask for millions.)"""
    inner = args.inner
    while inner < cap:
        total = window(fn, inner) * inner
        if total >= args.window_ms:
            break
        inner = min(cap, max(inner + 1, int(np.ceil(1.1 * inner * args.window_ms / max(total, 1e-3)))))
    return inner


def compare(forms, args):
    """{name: callable} -> {name: {"ms" (the median), "ms_min_max", "calls_per_window"}}; a form that raises in its warm-up is dropped
    from ``forms`` and reported under "failed"."""
    times, failed = {k: [] for k in forms}, {}
    for k, fn in list(forms.items()):
        try:
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
        except Exception as exc:
            failed[k] = repr(exc)[:300]
            del forms[k]
    inner = {k: calls_per_window(fn, args) for k, fn in forms.items()}
    for _ in range(args.reps):
        for k, fn in forms.items():
            times[k].append(window(fn, inner[k]))
    row = {k: {"ms": float(np.median(times[k])), "ms_min_max": [min(times[k]), max(times[k])], "calls_per_window": inner[k]} for k in forms}
    if failed:
        row["failed"] = failed
    return row
