"""The boundary of ``ops.mask_moments`` / ``ops.mask_shift`` (micro_sam_amd/_track.py), checked the way tests/test_ops_boundary_host.py
checks the wrappers defined in ops.py itself, with the same recorder and the same single-fault mutations (tests/ops_boundary_table.py):
valid arguments reach msam_mask_moments / msam_mask_shift with the expected scalars, and every single fault - a wrong type, a
non-contiguous view, an extra dimension, one element short, another device, sides out of range - is refused before any library call,
with a message that names the argument."""
import re

import pytest
import torch

from ops_boundary_table import Entry, i32, mutations, recording, z

P, H, W = 3, 40, 70                        # two word rows


def _check_moments(calls, kw):
    a = calls[0][1]
    assert a[0] == kw["bits"].data_ptr() and a[1:4] == [P, H, W] and a[4] and a[5] is None


def _check_shift(calls, kw):
    a = calls[0][1]
    assert a[0] == kw["bits"].data_ptr() and a[1:4] == [P, H, W] and a[4] == kw["shifts"].data_ptr() and a[5] not in (None, a[0]) and a[6] is None


_SIDES = [("no rows", {"height": 0}, "height"), ("too many rows", {"height": 32768}, "height"), ("no columns", {"width": 0}, "width"),
          ("another word row", {"height": 65}, "bits"), ("a narrower image", {"width": 69}, "bits")]
ENTRIES = [
    Entry("ops", "mask_moments", lambda: dict(bits=z(P, 2, W, dt=i32), height=H, width=W), ["msam_mask_moments"], free=("bits:0",),
          check=_check_moments, scalars=_SIDES),
    Entry("ops", "mask_shift", lambda: dict(bits=z(P, 2, W, dt=i32), height=H, width=W, shifts=z(P, 2, dt=torch.float64)),
          ["msam_mask_shift"], free=("bits:0",), check=_check_shift,
          scalars=_SIDES + [("shifts of another call", {"shifts": z(P + 1, 2, dt=torch.float64)}, "shifts"),
                            ("shifts as a list", {"shifts": [[0.0, 0.0]] * P}, "shifts")]),
]
CASES = [(e, label) for e in ENTRIES for label, _, _ in mutations(e, e.build())]


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_valid_arguments_reach_the_kernel(entry):
    kw = entry.build()
    with recording() as rec:
        out = entry.fn()(**kw)
    assert rec.names() == entry.expect
    entry.check(rec.calls, kw)
    assert out.dtype == (torch.int64 if entry.name == "mask_moments" else torch.int32)
    assert tuple(out.shape) == ((P, 3) if entry.name == "mask_moments" else (P, 2, W))
    labels = {label for label, _, _ in mutations(entry, kw)}
    assert {"bits:dtype", "bits:strides", "bits:rank", "bits:device", "bits:size1", "bits:size2"} <= labels
    if entry.name == "mask_shift":
        assert {"shifts:dtype", "shifts:strides", "shifts:rank", "shifts:device", "shifts:size0", "shifts:size1"} <= labels


@pytest.mark.parametrize("entry,label", CASES, ids=[f"{e.name}-{label}" for e, label in CASES])
def test_single_fault_is_refused_before_any_call(entry, label):
    (name, kw), = [(n, k) for lab, n, k in mutations(entry, entry.build()) if lab == label]
    with recording() as rec:
        with pytest.raises((ValueError, TypeError)) as err:
            entry.fn()(**kw)
    assert not rec.calls, f"refused after {rec.names()}"
    assert re.search(rf"\b{name}\b", str(err.value)), f"the message does not name {name}: {err.value}"


def test_the_word_type_and_an_empty_stack():
    from micro_sam_amd import ops
    with recording() as rec:
        assert ops.mask_moments(z(0, 2, W, dt=i32), H, W).shape == (0, 3)
        assert ops.mask_shift(z(0, 2, W, dt=i32), H, W, z(0, 2, dt=torch.float64)).shape == (0, 2, W)
    assert not rec.calls                                              # nothing to do launches nothing
    with recording() as rec:
        ops.mask_moments(z(P, 2, W, dt=torch.uint32), H, W)           # the words may be typed as they are
    assert rec.names() == ["msam_mask_moments"]
    with recording() as rec:
        with pytest.raises(ValueError, match="bits"):
            ops.mask_moments(z(65536, 1, 1, dt=i32), 1, 1)            # more objects than a call takes
    assert not rec.calls
