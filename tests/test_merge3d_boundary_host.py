"""The tensor-to-pointer boundary of ``ops.close_gaps_z``, ``ops.label_z_ranges`` and ``ops.apply_label_lut`` (micro_sam_amd/_merge3d.py),
checked the way tests/test_ops_boundary_host.py checks the wrappers defined in ops.py itself, with the same recorder and the same
single-fault mutations (tests/ops_boundary_table.py): valid arguments reach the entry point of csrc/merge3d.hip with the expected
scalars, and every single fault - a wrong type, rank, size, stride or device of one tensor, a workspace that is too small, a gap or a
count out of range - is refused before any library call, with a message that names the argument."""
import re

import pytest
import torch

from ops_boundary_table import Entry, blob, i32, mutations, recording, z

ANY_SHAPE = "labels of any shape are taken: one more dimension is no fault"


def _close_check(calls, kw):
    a = calls[0][1]
    assert a[0] == kw["labels"].data_ptr() and tuple(a[1:6]) == (3, 5, 7, 2, 9)
    assert a[8] == kw["workspace"].data_ptr() and a[9] == kw["workspace"].numel()


def _ranges_check(calls, kw):
    a = calls[0][1]
    assert a[0] == kw["labels"].data_ptr() and tuple(a[1:5]) == (3, 5, 7, 11)


def _lut_check(calls, kw):
    a = calls[0][1]
    assert (a[0], a[1], a[2], a[3], a[4]) == (kw["labels"].data_ptr(), 3 * 5 * 7, kw["lut"].data_ptr(), 6, kw["out"].data_ptr())


VOLUME = {"labels:0", "labels:1", "labels:2"}
ENTRIES = [
    Entry("ops", "close_gaps_z", lambda: dict(labels=z(3, 5, 7, dt=i32), gap=2, id_limit=9, workspace=blob(64)), ["msam_close_gaps"],
          free=VOLUME, check=_close_check,
          scalars=[("gap = 0", {"gap": 0}, "gap"), ("gap = -1", {"gap": -1}, "gap"), ("gap a float", {"gap": 1.0}, "gap"),
                   ("gap a bool", {"gap": True}, "gap"), ("id_limit = 0", {"id_limit": 0}, "id_limit"),
                   ("id_limit a float", {"id_limit": 9.0}, "id_limit"), ("workspace one byte short", {"workspace": blob(63)}, "workspace"),
                   ("workspace off a 4-byte boundary", {"workspace": blob(70)[2:68]}, "workspace")]),
    Entry("ops", "label_z_ranges", lambda: dict(labels=z(3, 5, 7, dt=i32), n_ids=11), ["msam_label_z_ranges"], free=VOLUME,
          check=_ranges_check,
          scalars=[("n_ids = 0", {"n_ids": 0}, "n_ids"), ("n_ids above 2^30", {"n_ids": 2 ** 30 + 1}, "n_ids"),
                   ("n_ids a float", {"n_ids": 11.0}, "n_ids")]),
    Entry("ops", "apply_label_lut", lambda: dict(labels=z(3, 5, 7, dt=i32), lut=z(6, dt=i32), out=z(3, 5, 7, dt=i32)),
          ["msam_apply_label_lut"], free=VOLUME | {"lut:0"}, check=_lut_check, blame={"labels:rank": "out"},
          scalars=[("an empty lut", {"lut": z(0, dt=i32)}, "lut")]),
]
BY_ID = {e.id: e for e in ENTRIES}


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.id)
def test_valid_arguments_reach_the_kernel(entry):
    kw = entry.build()
    with recording() as rec:
        entry.fn()(**kw)
    assert rec.names() == entry.expect
    entry.check(rec.calls, kw)


def _labels():
    return [(e.id, label) for e in ENTRIES for label, _, _ in mutations(e, e.build())]


@pytest.mark.parametrize("eid,label", _labels())
def test_single_fault_is_refused_before_any_call(eid, label):
    entry = BY_ID[eid]
    (name, kw), = [(n, k) for lab, n, k in mutations(entry, entry.build()) if lab == label]
    with recording() as rec:
        with pytest.raises((ValueError, TypeError)) as err:
            entry.fn()(**kw)
    assert not rec.calls, f"refused after {rec.names()}"
    assert re.search(rf"\b{name}\b", str(err.value)), f"the message does not name {name}: {err.value}"


def test_every_tensor_argument_is_mutated():
    for entry in ENTRIES:
        kw = entry.build()
        mutated = {name for _, name, _ in mutations(entry, kw)} | set(entry.blame.values())
        assert {k for k, v in kw.items() if isinstance(v, torch.Tensor)} <= mutated
    assert len(_labels()) >= 40


def test_defaults_and_the_empty_volume():
    """Without a workspace the wrapper allocates what the query asks for; without an id limit it reads the volume's maximum; an empty
    volume is answered without a launch."""
    with recording() as rec:
        from micro_sam_amd import ops
        labels = z(2, 4, 4, dt=i32)
        labels[1, 2, 2] = 6
        out, result = ops.close_gaps_z(labels, 1)
        a = rec.calls[0][1]
        assert tuple(a[1:6]) == (2, 4, 4, 1, 7) and a[9] == 64 and out.shape == labels.shape and result.shape == (4,)
        out, flag = ops.apply_label_lut(labels, z(7, dt=i32))
        assert rec.names() == ["msam_close_gaps", "msam_apply_label_lut"] and out is not labels and out.shape == labels.shape
        n = len(rec.calls)
        empty = z(0, 4, 4, dt=i32)
        out, result = ops.close_gaps_z(empty, 1)
        assert out.shape == (0, 4, 4) and result.tolist() == [1, 0, 0, 0]
        zr, flag = ops.label_z_ranges(empty, 3)
        assert zr.tolist() == [[0, -1]] * 3 and flag.tolist() == [0]
        out, flag = ops.apply_label_lut(empty, z(3, dt=i32))
        assert out.shape == (0, 4, 4) and len(rec.calls) == n
