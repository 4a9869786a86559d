"""The tensor-to-pointer boundary of ``ops.adapter_`` (micro_sam_amd/_adapter.py), checked the way tests/test_ops_boundary_host.py checks the
wrappers defined in ops.py itself, with the same recorder and the same single-fault mutations (tests/ops_boundary_table.py): valid arguments
reach msam_adapter_bf16 with the expected scalars, and every single fault - a wrong type, rank, size, stride or device of one tensor, an
unsupported width - is refused before any library call, with a message that names the argument."""
import re

import pytest
import torch

from ops_boundary_table import BF16, Entry, bf16, f16, mutations, recording, z


def _check(calls, kw):
    a = calls[0][1]
    assert (a[1], a[8], a[9], a[10], a[11], a[12]) == (128, 128, 6, 128, 64, BF16)
    assert a[0] == kw["y"].data_ptr() and a[7] == kw["x"].data_ptr() and a[6] == kw["alpha"].data_ptr()


ENTRY = Entry("ops", "adapter_",
              lambda: dict(x=z(6, 128), y=z(6, 128, dt=bf16), wd=z(64, 128, dt=bf16), bd=z(64), wu=z(128, 64, dt=bf16), bu=z(128), alpha=z(1)),
              ["msam_adapter_bf16"], check=_check, blame={"x:size0": "y"},
              scalars=[("P = 48", {"wd": z(48, 128, dt=bf16), "bd": z(48), "wu": z(128, 48, dt=bf16)}, "wd"),
                       ("P = 160", {"wd": z(160, 128, dt=bf16), "bd": z(160), "wu": z(128, 160, dt=bf16)}, "wd"),
                       ("D = 192", {"x": z(6, 192), "y": z(6, 192, dt=bf16), "wd": z(64, 192, dt=bf16), "wu": z(192, 64, dt=bf16), "bu": z(192)}, "x"),
                       ("fp16 weights with a bf16 y", {"wd": z(64, 128, dt=f16)}, "wd"),
                       ("y fp32", {"y": z(6, 128)}, "y"),
                       ("y rows not in eights", {"y": z(6, 132, dt=bf16)[:, :128]}, "y"),
                       ("y not on a 16-byte boundary", {"y": z(6, 136, dt=bf16)[:, 4:132]}, "y")])


def test_valid_arguments_reach_the_kernel():
    kw = ENTRY.build()
    with recording() as rec:
        out = ENTRY.fn()(**kw)
    assert out is kw["x"] and rec.names() == ENTRY.expect
    _check(rec.calls, kw)
    # views with contiguous rows are handed over with their strides
    kw = dict(kw, x=z(6, 133)[:, :128], y=z(6, 136, dt=bf16)[:, :128])
    with recording() as rec:
        ENTRY.fn()(**kw)
    a = rec.calls[0][1]
    assert (a[1], a[8]) == (136, 133)


def _labels():
    return [label for label, _, _ in mutations(ENTRY, ENTRY.build())]


@pytest.mark.parametrize("label", _labels())
def test_single_fault_is_refused_before_any_call(label):
    (name, kw), = [(n, k) for lab, n, k in mutations(ENTRY, ENTRY.build()) if lab == label]
    with recording() as rec:
        with pytest.raises((ValueError, TypeError)) as err:
            ENTRY.fn()(**kw)
    assert not rec.calls, f"refused after {rec.names()}"
    assert re.search(rf"\b{name}\b", str(err.value)), f"the message does not name {name}: {err.value}"


def test_every_tensor_argument_is_mutated():
    kw = ENTRY.build()
    mutated = {name for _, name, _ in mutations(ENTRY, kw)} | set(ENTRY.blame.values())
    assert {k for k, v in kw.items() if isinstance(v, torch.Tensor)} <= mutated
    assert len(_labels()) >= 30
