"""CPU side of the device pin of the weights-stationary decoder GEMM (tests/test_gpu_wsgemm.py, tests/wsgemm_ref.py).

1. The device bodies run against the host-compiled library (tests/host_product.py): the same generators, references, sentinels and
   refusals.  The emulation runs the workgroups of a launch one after the other with the kernel's own grid, so the persistent loop takes
   the same number of iterations per workgroup as on the device; what the CPU cannot show - the MFMA register layouts, the buffer
   descriptors, the order of the memory operations in flight - is the device file's part.  M = 49280 and M = 32768 are left to the
   device, to keep this file under a minute: the emulation needs up to 5 s per launch there, and M = 34880 already mixes two and three
   iterations (both register sets in use, the clamp and the guarded store taken both ways).
2. The suite has teeth: each defect of ``wsgemm_ref.DEFECTS`` is applied to the REFERENCE path (``expected(..., defect=...)``) and must
   break bit equality with the correct reference on the generators' cases - so a kernel with that defect cannot pass.
3. The generators' own conditions."""
import pytest
import torch

import test_gpu_wsgemm as T
import wsgemm_ref as R
from host_product import product_on_host
from test_gpu_wsgemm import (test_gaussian, test_head_major, test_kv_split, test_layernorm_epilogues, test_plain,  # noqa: F401
                             test_refusal_by_the_wrapper, test_refusals, test_residual, test_residual_in_place, test_table)


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    with product_on_host(str(tmp_path_factory.mktemp("host_wsgemm"))):
        yield torch.device("cpu")


# ---- 1. the persistent loop on the host library

@pytest.mark.parametrize("kind", list(T.LOOP_KINDS))
@pytest.mark.parametrize("M", [m for m in T.LOOP_M if m not in (32768, 49280)])
def test_persistent_loop(dev, M, kind):
    T.run_persistent(dev, M, kind)


# ---- 2. every defect breaks bit equality

def _differs(c, defect, **lay):
    good, bad = R.expected(c, defect=defect, **lay), R.expected(c, **lay)
    return any(not R.same_bits(good[k], bad[k]) for k in good)


def test_every_defect_is_listed():
    assert set(R.DEFECTS) == {"tile_stride_off", "stale_tile", "last_tile_clamped", "table_row_off", "table_col_le4", "resid_nowrap",
                              "vt_untransposed", "head_batch_per_tile", "ln64_index_unwrapped", "truncate", "double_round"}


@pytest.mark.parametrize("defect", R.TILE_DEFECTS)
def test_tile_defects_break_bit_equality(dev, defect):
    """A tile computed from another tile's rows of A, at the smallest M of the persistent-loop cases that has a second pass, in the
    layouts the loop is tested in."""
    N, K, gen, launch = T.LOOP_KINDS["k128-plain"]
    assert _differs(R.exact_case(16448, N, K, 700 + 448 + N + 3 * K, **gen), defect), defect
    N, K, gen, launch = T.LOOP_KINDS["kv-split"]
    assert _differs(R.exact_case(16448, N, K, 700 + 448 + N + 3 * K, **gen), defect, **launch), defect
    if defect == "last_tile_clamped":                                   # needs no second pass: shows at the small shapes too
        assert _differs(R.exact_case(64, 128, 128, 100 + 64 + 128 + 3 * 128), defect)


@pytest.mark.parametrize("N,K", T.NK)
def test_epilogue_defects_break_bit_equality(dev, N, K):
    c = R.exact_case(128, N, K, 200 + N + 3 * K + 4, table=4)
    assert _differs(c, "table_row_off")
    c = R.exact_case(192, N, K, 300 + N + 3 * K + 40, resid=True, resid_rows=40)
    assert _differs(c, "resid_nowrap")
    for d in ("truncate", "double_round"):
        assert _differs(c, d), d
    c = R.exact_case(64, N, K, 1100 + N + K, table=6)                  # the confirmed bug: a [7, 6] table with table_cols = 6
    bad, good = R.expected(c, defect="table_col_le4")["out"], R.expected(c)["out"]
    assert R.same_bits(bad[:, :6], good[:, :6]) and R.same_bits(bad[:, 8:], good[:, 8:])
    assert not R.same_bits(bad[:, 6:8], good[:, 6:8]) and bool(torch.isinf(bad[6, 6:8].float()).all())   # row 6: past the last table row
    c = R.exact_case(192, N, K, 500 + N + 3 * K + 48 + 128, table=128)
    assert _differs(c, "head_batch_per_tile", head_major=1, tokens=48)
    assert not _differs(c, "head_batch_per_tile", head_major=1, tokens=64)       # whole tiles per image: nothing to get wrong
    c = R.exact_case(384, N, K, 600 + N + 3 * K + 64 + 1, table=(128 if N == 256 else 64))
    assert _differs(c, "vt_untransposed", kv_split=1, tokens=64)
    c = R.ln_case(192, N, K, 800 + 2 + N + 3 * K, 2)
    assert _differs(c, "ln64_index_unwrapped", ln_mode=2, ln_eps=1e-6)


# ---- 3. the generators' conditions

@pytest.mark.parametrize("N,K", T.NK)
def test_generator_conditions(dev, N, K):
    """exact_case asserts them itself; restated here on its reference: >= 25 % inexact and >= 1 % exact ties in the decoder's type, every
    result where that type's spacing is >= 2, integer-valued, rows of A distinct across the whole M - at a persistent-loop M as well."""
    d = R.d16()
    for M, gen in ((192, dict(table=64, resid=True, resid_rows=40)), (16448, {})):
        c = R.exact_case(M, N, K, 1200 + N + K, **gen)
        v = c["ref"].float()
        inexact, ties = R.G.shares(v, d)
        assert inexact >= 0.25 and ties >= 0.01, (inexact, ties)
        assert float(c["ref"].abs().min()) > R.THRESH16[d] and bool((c["ref"] == c["ref"].round()).all())
        assert torch.unique(c["A"].float(), dim=0).shape[0] == M
    c = R.ln_case(192, N, K, 1300 + N + K, 2, resid_rows=40)
    assert bool((c["ref"][c["const_row"]] == 7).all()) and torch.unique(c["ln_w"]).numel() == 64 and torch.unique(c["ln_b"]).numel() == 64
