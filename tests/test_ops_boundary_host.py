"""The tensor -> pointer boundary of micro_sam_amd.ops / micro_sam_amd.strict, without a GPU.

The C entry points see addresses and a few integers; a dtype, a stride, a device or a tensor's real size is what the Python wrapper
checks or nobody does.  Two harnesses:

* the RECORDER (tests/ops_boundary_table.py ``recording``): ``_lib.load()`` hands out an object that notes name and arguments of every ``msam_*`` call and
  returns 0, so no kernel can run.  ``TABLE`` has one entry per public wrapper that hands a ``data_ptr()`` to the library: a builder
  of valid arguments (small CPU tensors) and, derived from it, the single-fault mutations - every tensor argument in turn with a
  wrong dtype, as a non-contiguous view, with one more dimension, one element short in every dimension the wrapper checks, and on
  another device (a ``meta`` tensor) - plus the scalar mismatches listed per entry.  A refusal is a ``ValueError`` / ``TypeError``
  that names the argument, with ZERO recorded calls.  ``SKIP`` lists, with a reason each, the mutations that are no fault for a
  wrapper (it converts the argument, or the dimension is free).  Size queries (``*_bytes``) and ``msam_decoder_dtype`` take no
  pointer and are answered without being recorded.
* the HOST LIBRARY (tests/host_product.py): the accepted cases that had no value test - fp16 outputs of ``layernorm`` / ``gemm``,
  row-strided ``cast_transpose`` - against fp64; the bodies are those of tests/test_gpu_ops_boundary.py.

``test_every_pointer_wrapper_is_in_the_table`` walks the public functions of both modules, so a new wrapper cannot stay outside.
The classes of strict.py (StrictEncoder / StrictDecoder) own whole models and build their buffers themselves, like the
msam_encoder_forward / msam_decoder_forward struct builders of modeling.py; they are not part of this table."""
import inspect
import re

import pytest
import torch

import test_gpu_ops_boundary as G
from host_product import product_on_host
from ops_boundary_table import BY_ID, EXEMPT, TABLE, mutations, recording, tensor_paths


def _public_functions():
    from micro_sam_amd import ops, strict
    for mod, short in ((ops, "ops"), (strict, "strict")):
        for name, fn in inspect.getmembers(mod, inspect.isfunction):
            if fn.__module__ == mod.__name__ and not name.startswith("_"):
                yield f"{short}.{name}", fn


def _run_valid(entry):
    kw = entry.build()
    with recording() as rec:
        entry.fn()(**kw)
    return kw, rec.calls


def test_every_pointer_wrapper_is_in_the_table():
    seen = set()
    for ident, fn in _public_functions():
        seen.add(ident)
        if ident in BY_ID:
            entry = BY_ID[ident]
            kw, calls = _run_valid(entry)
            assert calls, f"{ident}: the valid arguments recorded no library call"
            mutated = {name for _, name, _ in mutations(entry, kw)}
            for name, _ in tensor_paths(kw):
                assert name in mutated, f"{ident}: no mutation of tensor argument {name}"
            params = inspect.signature(fn).parameters
            assert set(kw) <= set(params), f"{ident}: the builder passes unknown arguments"
        else:
            assert ident in EXEMPT, f"{ident} is neither in TABLE nor in EXEMPT"
            with recording() as rec:
                EXEMPT[ident][1](fn)
            assert not rec.calls, f"{ident} is exempt but handed pointers to {rec.names()}"
    assert set(BY_ID) <= seen and set(EXEMPT) <= seen, "TABLE / EXEMPT name functions that do not exist"
    for e in TABLE:
        assert all(e.skip.values()), f"{e.id}: a skipped mutation without a reason"


@pytest.mark.parametrize("entry", TABLE, ids=[e.id for e in TABLE])
def test_valid_arguments_reach_the_expected_entry_points(entry):
    kw, calls = _run_valid(entry)
    assert [c[0] for c in calls] == entry.expect
    if entry.check is not None:
        entry.check(calls, kw)


def _cases():
    for entry in TABLE:
        for label, name, _ in mutations(entry, entry.build()):
            yield pytest.param(entry, label, id=f"{entry.id}-{label}")


@pytest.mark.parametrize("entry,label", list(_cases()))
def test_single_fault_is_refused_before_any_call(entry, label):
    (name, kw), = [(n, k) for lab, n, k in mutations(entry, entry.build()) if lab == label]
    with recording() as rec:
        with pytest.raises((ValueError, TypeError)) as err:
            entry.fn()(**kw)
    assert not rec.calls, f"refused after {rec.names()}"
    assert re.search(rf"\b{name.split('[')[0]}\b", str(err.value)), f"the message does not name {name}: {err.value}"


def test_refusals_survive_python_O():
    """No ``assert`` guards a hand-over: the source of both modules has none outside docstrings."""
    import ast
    from micro_sam_amd import ops, strict
    for mod in (ops, strict):
        tree = ast.parse(inspect.getsource(mod))
        assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)], mod.__name__
        assert "F32 if" not in inspect.getsource(mod)


# ------------------------------------------------------------------------------------------------------------- host library

@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    with product_on_host(str(tmp_path_factory.mktemp("host_boundary"))):
        yield torch.device("cpu")


test_layernorm_fp16_output = G.test_layernorm_fp16_output
test_gemm_fp16_output = G.test_gemm_fp16_output
test_cast_transpose_row_strided = G.test_cast_transpose_row_strided
