"""The boundary of ``ops.seed_centers`` (micro_sam_amd/_promptseeds.py), checked the way tests/test_ops_boundary_host.py checks the
wrappers defined in ops.py itself, with the same recorder and the same single-fault mutations (tests/ops_boundary_table.py): valid
arguments reach msam_seed_centers with the expected scalars, and every single fault - a wrong type, rank, size, stride or device of one
of the three maps, a side the kernels cannot index, a threshold numpy could not compare the way the kernel does - is refused before any
library call, with a message that names the argument.  Also here, without a GPU: how a threshold is rounded."""
import re

import numpy as np
import pytest
import torch

from ops_boundary_table import Entry, mutations, recording, z

MAPS = ("foreground", "center_distances", "boundary_distances")
THRESHOLDS = ("foreground_threshold", "center_distance_threshold", "boundary_distance_threshold")


def _check(calls, kw):
    a = calls[0][1]
    assert [a[i] for i in range(3)] == [kw[n].data_ptr() for n in MAPS]
    assert (a[3], a[4]) == (6, 10) and a[8] == 1 and a[10] == 30                     # H, W, avoid_image_border, max_centers
    assert (a[5], a[6], a[7]) == (float(np.float32(0.45)), 0.55, float(np.float32(0.3)))
    assert a[13] >= 64 and all(a[i] for i in (9, 11, 12))


ENTRY = Entry("ops", "seed_centers",
              lambda: dict(foreground=z(6, 10), center_distances=z(6, 10), boundary_distances=z(6, 10), foreground_threshold=0.45,
                           center_distance_threshold=np.float64(0.55), boundary_distance_threshold=np.float32(0.3)),
              ["msam_seed_centers"], check=_check,
              # foreground defines H and W; a map of another size is blamed on the map that disagrees with it
              free={"foreground:0", "foreground:1"},
              scalars=[("no rows", {n: z(0, 10) for n in MAPS}, "foreground"), ("no columns", {n: z(6, 0) for n in MAPS}, "foreground"),
                       ("a side of 32768", {n: z(32768, 1) for n in MAPS}, "foreground"),
                       ("foreground one row short", {"foreground": z(5, 10)}, "center_distances")]
              + [(f"{t} NaN", {t: float("nan")}, t) for t in THRESHOLDS]
              + [(f"{t} np.float64 NaN", {t: np.float64("nan")}, t) for t in THRESHOLDS]
              + [("a threshold that is a string", {"foreground_threshold": "0.5"}, "foreground_threshold"),
                 ("a threshold that is a tensor", {"center_distance_threshold": torch.tensor(0.5)}, "center_distance_threshold"),
                 ("a complex threshold", {"boundary_distance_threshold": 0.5 + 0j}, "boundary_distance_threshold"),
                 ("a bool threshold", {"foreground_threshold": True}, "foreground_threshold"),
                 ("a long double threshold", {"foreground_threshold": np.longdouble(0.5)}, "foreground_threshold")])
CASES = [label for label, _, _ in mutations(ENTRY, ENTRY.build())]


def test_valid_arguments_reach_the_kernel():
    kw = ENTRY.build()
    with recording() as rec:
        out = ENTRY.fn()(**kw)
    assert rec.names() == ENTRY.expect
    ENTRY.check(rec.calls, kw)
    assert out.n == 0 and not out.undefined and out.centers.dtype == torch.int32 and tuple(out.centers.shape) == (0, 2)
    labels = set(CASES)
    assert {f"{n}:{k}" for n in MAPS for k in ("dtype", "strides", "rank", "device")} <= labels
    assert {f"{n}:size{d}" for n in MAPS[1:] for d in (0, 1)} <= labels


@pytest.mark.parametrize("label", CASES)
def test_single_fault_is_refused_before_any_call(label):
    (name, kw), = [(n, k) for lab, n, k in mutations(ENTRY, ENTRY.build()) if lab == label]
    with recording() as rec:
        with pytest.raises((ValueError, TypeError)) as err:
            ENTRY.fn()(**kw)
    assert not rec.calls, f"refused after {rec.names()}"
    assert re.search(rf"\b{name}\b", str(err.value)), f"the message does not name {name}: {err.value}"


def test_thresholds_compare_as_numpy_compares_a_float32_array():
    """The kernel compares in fp64; the number it is given makes that numpy's ``map < threshold`` on a float32 map."""
    from micro_sam_amd._promptseeds import _threshold
    t32 = np.float32(0.45)
    near = np.array([np.nextafter(t32, np.float32(-1)), t32, np.nextafter(t32, np.float32(2))], np.float32)
    for value in (0.45, np.float64(0.45), np.float32(0.45), np.float16(0.45), 1, np.int64(1), 0.1 + 0.2, 1e-50, -1e300, np.float64(1e300),
                  float("inf"), np.float64("-inf"), 1e300):
        t = _threshold("t", value)
        assert isinstance(t, float)
        probe = np.concatenate([near, np.array([0, 1, np.nextafter(np.float32(1), np.float32(0)), np.inf, -np.inf, np.nan, 3.4e38], np.float32)])
        with np.errstate(over="ignore"):
            assert np.array_equal(probe.astype(np.float64) < t, probe < value), value
    assert _threshold("t", 0.45) == float(t32) != 0.45 and _threshold("t", np.float64(0.45)) == 0.45
