"""CPU side of the GEMM family's device pin (tests/test_gpu_gemm_routes.py, tests/gemm_ref.py).

1. The device bodies of routes 1 - 5, 7, 8 and 9 run against the host-compiled library (tests/host_product.py), as
   tests/test_host_kernel_suite.py does for tests/test_gpu_kernels.py: the same generators, references, route assertions and sentinels.  The
   host MFMA accumulates in double and rounds once, so the integer cases are exact here as well; what the CPU cannot show - the MFMA register
   layouts, the buffer-descriptor clamps, the LDS-DMA, the hardware conversions - is the device file's part.  Route 6 (gemm256_kernel at
   256 tiles and more) stays with tests/test_gemm_kernel_host_emulation.py and the device.
   No case is left out for its run time: the emulation takes well under a second for every one of them.
2. The suite has teeth: each defect below is applied to the REFERENCE path (``gemm_ref.expected(..., defect=...)``, a deliberately wrong
   product) and must break bit equality with the correct reference on the generators' cases - so a kernel with that defect cannot pass.
3. The generators' own conditions (>= 25 % of the 16-bit results inexact, >= 1 % exact ties, distinct rows / columns), the coverage of
   route 1's case table, and the design error of the GELU approximation."""
import itertools

import pytest
import torch

import gemm_ref as G
import test_gpu_gemm_routes as R
from host_product import product_on_host

BF, H, F32, F8 = torch.bfloat16, torch.float16, torch.float32, G.FP8_T


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    with product_on_host(str(tmp_path_factory.mktemp("host_gemm_routes"))):
        yield torch.device("cpu")


# ---- 1. the device bodies on the host library: the device file's own case tables

@pytest.mark.parametrize("M,N,K,vname,ename,od", R.route1_cases())
def test_route1_gemm_kernel(env, M, N, K, vname, ename, od):
    R.test_route1_gemm_kernel(env, M, N, K, vname, ename, od)


@pytest.mark.parametrize("dt,glds", [(BF, 0), (BF, 1), (H, 0)])
@pytest.mark.parametrize("head_dim,heads,tokens,K", [(64, 2, 65, 64), (80, 8, 70, 128)])
def test_route2_qkv_split(env, head_dim, heads, tokens, K, dt, glds):
    R.test_route2_qkv_split(env, head_dim, heads, tokens, K, dt, glds)


@pytest.mark.parametrize("dt,glds,K", [(BF, 0, 64), (BF, 1, 192), (H, 0, 128)])
def test_route2_kv_split(env, dt, glds, K):
    R.test_route2_kv_split(env, dt, glds, K)


@pytest.mark.parametrize("dt,od", [(BF, BF), (H, H), (H, BF)])
@pytest.mark.parametrize("M,N,K,relu", [(129, 128, 128, True), (1, 384, 64, False), (300, 128, 192, True)])
def test_route3_hi_lo_pairs(env, M, N, K, relu, dt, od):
    R.test_route3_hi_lo_pairs(env, M, N, K, relu, dt, od)


@pytest.mark.parametrize("dt", [BF, H])
@pytest.mark.parametrize("pick", [(1,), (3, 2), (0, 1, 2, 3, 4)])
def test_route4_group(env, pick, dt):
    R.test_route4_group(env, pick, dt)


@pytest.mark.parametrize("dt", [BF, H])
@pytest.mark.parametrize("M,N,K,split", [(129, 128, 512, 8), (128, 256, 256, 2), (1, 128, 128, 2)])
def test_route5_split_k(env, M, N, K, split, dt):
    R.test_route5_split_k(env, M, N, K, split, dt)


@pytest.mark.parametrize("M,K,ename,N", R.route7_cases())
def test_route7_fp8(env, M, K, ename, N):
    R.test_route7_fp8(env, M, K, ename, N)


@pytest.mark.parametrize("M,K,dt,mode,ename", R.route8_cases())
def test_route8_fused_layernorm(env, M, K, dt, mode, ename):
    R.test_route8_fused_layernorm(env, M, K, dt, mode, ename)


@pytest.mark.parametrize("vname,M,N,K", [("bf16", 300, 128, 128), ("bf16-glds", 129, 384, 64), ("fp16", 127, 128, 192)])
def test_route9_gelu(env, vname, M, N, K):
    R.test_route9_gelu(env, vname, M, N, K)


test_refusals_single = R.test_refusals_single
test_refusals_group = R.test_refusals_group


# ---- 2. every defect breaks bit equality

def _differs(c, defect, **lay):
    good, bad = G.expected(c, **lay), G.expected(c, defect=defect, **lay)
    return any(not G.same_bits(good[k], bad[k]) for k in good)


@pytest.mark.parametrize("od", [BF, H])
@pytest.mark.parametrize("defect", ["truncate", "double_round", "drop_ktile", "dup_ktile", "swap_rows", "swap_aw_frag", "table_row_off",
                                    "resid_nowrap", "table_col_le", "lda_as_k"])
def test_defect_breaks_bit_equality_plain(defect, od):
    """Plain output, 16-bit and fp32: rounding defects (truncation instead of RNE, double rounding through the other 16-bit type), a
    dropped / duplicated k-tile, two rows of a 16-row fragment swapped, the A and W fragments of a tile swapped, the table row off by one,
    ``row % resid_rows`` ignored, the table applied at ``col <= table_cols``, ``lda`` taken as K."""
    for M, N, K in [(129, 128, 128), (17, 384, 64)]:
        c = G.exact_case(M, N, K, od, 11 + M, out_dtype=od, table=4, resid=F32, resid_rows=(5 if M > 5 else 0))
        if defect == "resid_nowrap" and not c["resid_rows"]:
            continue
        assert _differs(c, defect), (defect, M, N, K)
        if defect not in ("truncate", "double_round"):
            assert _differs(dict(c, out_dtype=F32), defect), (defect, M, N, K, "fp32 output")


@pytest.mark.parametrize("od", [BF, H])
def test_defect_breaks_bit_equality_layouts(od):
    """Heads / which crossed in the q / k / v split, vT written untransposed, the hi / lo thirds swapped, lo from the unrounded hi."""
    c = G.exact_case(130, 384, 64, od, 21, out_dtype=od)
    assert _differs(c, "qkv_cross", out_mode=1, heads=2, head_dim=64, tokens=65)
    c = G.exact_case(256, 256, 64, od, 22, out_dtype=od, table=128)
    assert _differs(c, "vt_untransposed", out_mode=2, tokens=128)
    c = G.exact_case(129, 128, 64, od, 23, out_dtype=od, relu=True)
    assert _differs(c, "hilo_swapped", out_mode=3) and _differs(c, "lo_from_unrounded", out_mode=3)
    for d in ("truncate", "double_round"):
        assert _differs(c, d, out_mode=3), d


# ---- 3. the generators' conditions, the case table, the GELU design error

@pytest.mark.parametrize("od", [BF, H])
@pytest.mark.parametrize("dt", [BF, H, F8])
@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (300, 384, 256), (129, 256, 512)])
def test_generator_conditions(M, N, K, dt, od):
    """exact_case asserts them itself; restated here on its reference: >= 25 % inexact and >= 1 % exact ties in the 16-bit output type, all
    results where that type's spacing is >= 2, integer-valued below 2^22, distinct rows and columns."""
    if dt == F8:
        N, K = 256 * ((N + 255) // 256), 128 * ((K + 127) // 128)
    for epi in ({}, dict(table=4, resid=F32, resid_rows=0), dict(relu=True)):
        if dt == F8 and "table" in epi:
            epi = dict(resid=F32)
        c = G.exact_case(M, N, K, dt, 31 + M, out_dtype=od, **epi)
        v = G.act64(c["ref"], c).float()
        inexact, ties = G.shares(v, od)
        assert inexact >= 0.25 and ties >= 0.01, (inexact, ties)
        assert float(c["ref"].abs().min()) > G.THRESH16[od]
        exact16 = G.rne16(v, od).float() == v
        assert abs(float((~exact16).float().mean()) - inexact) < 1e-12          # the bit test agrees with the cast
        assert G._distinct(c["A"], c["W"])


def test_route1_case_table_covers_every_axis():
    cases = [p.values for p in R.route1_cases()]
    assert {(M, K, v) for M, N, K, v, e, od in cases} == set(itertools.product((1, 127, 129, 300), (64, 128, 192, 256), [v[0] for v in R.VARIANTS]))
    assert {(e, v) for M, N, K, v, e, od in cases} == set(itertools.product([e[0] for e in R.EPIS], [v[0] for v in R.VARIANTS]))
    assert {N for M, N, K, v, e, od in cases} == {128, 384}
    assert {(v, od) for M, N, K, v, e, od in cases} >= {("fp16", BF), ("bf16", H), ("bf16", BF), ("fp16", H), ("bf16-glds", F32)}


def test_gelu_design_error():
    """The formula of ``gelu_erf2`` with common.h's constants, in float64, against erf-GELU on a dense grid over [-12, 12]: 5.5e-5 at
    x = -1.88 - the first term of route 9's allowance."""
    err, at = G.gelu_design_error()
    print("FIG gelu design error", err, "at", at)
    assert 5.0e-5 <= err <= 6.0e-5 and abs(at + 1.88) < 0.05, (err, at)
