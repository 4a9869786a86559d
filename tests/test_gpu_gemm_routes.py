"""Device pin of every launch route of the GEMM family (csrc/gemm.hip) - harness, generators and references in tests/gemm_ref.py.

Per route one parametrised body; a case
(a) runs the integer ``exact_case`` and requires every output (plain, q / k / v, k / vT, hi | lo | hi) to EQUAL the exact result, or its
    round-to-nearest-even 16-bit cast, bit for bit;
(b) asserts the kernel family the launch recorded (``route_taken``: 0 = gemm256_kernel, 5 = gemm_kernel / gemm_ln_kernel / grouped,
    None = split-K, which is not profiled);
(c) runs twice and requires the same bits;
(d) for 16-bit outputs runs the Gaussian ``random_case`` with an fp32 and with the 16-bit output: the 16-bit one must equal the RNE cast of
    the fp32 one of the SAME route bit for bit (the two launches differ in the pack instruction only), and the fp32 one must meet
    tests/test_gpu_kernels.py's own bound, 1e-3 + 1e-4 |ref|, against a float64 product of the same operands.
The fused LayerNorm and the GELU epilogue are not integer-exact; their bodies state their checks.  Leading dimensions exceed the logical
widths everywhere (lda = K + 8, ldw = K + 16, ldc = N + 4, table_ld = table_cols + 4, ldr = N + 8) and every buffer carries NaN sentinels.

Shapes that the routes' own constraints force away from a round number: a q / k / v split needs N = 3 heads head_dim, so the 256 x 256
kernel's split runs at N = 4608 (24 heads of 64; M = 15 x 239 = 3585: 15 x 18 = 270 tiles, the last row tile with one live row, tiles
straddling images) and the fp8 one at N = 768; head_dim 80 needs heads % 8 == 0 (N = 1920).

The bodies also run on the CPU against the host-compiled library (tests/test_gemm_routes_host.py).  Lines starting with "FIG" carry the
figures recorded in profiles/gemm_routes_device.md (pytest -s)."""
import itertools

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

BF, H, F32, F8 = torch.bfloat16, torch.float16, torch.float32, G.FP8_T
OTHER = {BF: H, H: BF}
NAME = {BF: "bf16", H: "fp16", F32: "fp32", F8: "fp8"}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _fig(route, case, **kv):
    print("FIG", route, case, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _kw(c, out_dtype, *, pads=(8, 16, 4), inplace=False, **launch):
    """``G.call``'s keywords of case ``c``: padded leading dimensions everywhere."""
    M, N, K = c["M"], c["N"], c["K"]
    kw = G.operands(c)
    kw.update(launch)
    kw.update(lda=K + pads[0], ldw=K + pads[1], out_dtype=out_dtype)
    mode = launch.get("out_mode", 0)
    if mode == 0 and not launch.get("split_k"):
        kw["ldc"] = N + pads[2]
    if "table" in c:
        kw["table_ld"] = c["table"].shape[1] + 4
    if inplace:
        kw["inplace"] = True
    elif "resid" in c:
        kw["ldr"] = N + 8
    return kw


def run_route(dev, route, name, *, M, N, K, dt, out_dtype, family, seed, epi=None, inplace=False, pads=(8, 16, 4), **launch):
    """(a) - (d) of the module docstring for one launch configuration; ``epi`` = the generators' epilogue keywords."""
    epi = dict(epi or {})
    mode = launch.get("out_mode", 0)
    lay = {k: launch[k] for k in ("heads", "head_dim", "tokens") if k in launch}
    c = G.exact_case(M, N, K, dt, seed, out_dtype=out_dtype, dev=dev, **epi)
    kw = _kw(c, out_dtype, pads=pads, inplace=inplace, **launch)
    r1, fam = G.route_taken(lambda: G.call(dev, c["A"], c["W"], **kw))
    assert fam == family, f"{route} {name}: launch recorded family {fam}, expected {family}"                  # (b)
    exp = G.expected(c, dev, out_mode=mode, **lay)
    G.assert_bits(r1, exp, f"{route} {name} exact")                                                             # (a)
    r2 = G.call(dev, c["A"], c["W"], **kw)
    G.assert_bits(r2, r1.tensors(), f"{route} {name} second run")                                               # (c)
    ratio = None
    if out_dtype != F32:                                                                                        # (d)
        cr = G.random_case(M, N, K, dt, seed + 1, out_dtype=out_dtype, dev=dev, **epi)
        tw = {k: v for k, v in launch.items() if k not in ("out_mode", "heads", "head_dim", "tokens")}
        r32 = G.call(dev, cr["A"], cr["W"], **_kw(cr, F32, pads=pads, **tw))
        r16 = G.call(dev, cr["A"], cr["W"], **_kw(cr, out_dtype, pads=pads, **launch))
        G.assert_bits(r16, G.expected(cr, dev, out_mode=mode, v32=r32.out, **lay), f"{route} {name} 16-bit output vs RNE of the fp32 twin")
        ratio = G.err_over_tol(r32.out, G.act64(cr["ref"].to(dev), cr), 1e-3, 1e-4)
        assert ratio <= 1.0, f"{route} {name}: fp32 output vs float64: err / tol = {ratio}"
    _fig(route, name, family=fam, err_over_tol=ratio)


# ---- route 1: gemm_kernel - bf16 register staging, bf16 LDS-DMA, fp16

VARIANTS = [("bf16", BF, 0), ("bf16-glds", BF, 1), ("fp16", H, 0)]
# (name, generator keywords, in place, 16-bit output?)
EPIS = [
    ("bias", {}, False, False),
    ("table4", dict(table=4), False, True),
    ("table128", dict(table=128), False, False),
    ("tableN", dict(table="N"), False, True),
    ("resid-f32", dict(resid=F32), False, True),
    ("resid-bf16-wrap5", dict(resid=BF, resid_rows=5), False, False),
    ("resid-fp16-wrap5", dict(resid=H, resid_rows=5), False, True),
    ("resid-fp16", dict(resid=H), False, False),
    ("resid-bf16", dict(resid=BF), False, True),
    ("inplace", dict(resid=F32), True, False),
    ("relu", dict(relu=True), False, True),
    ("table4-resid-f32-wrap5-relu", dict(table=4, resid=F32, resid_rows=5, relu=True), False, True),
]


def route1_cases():
    """Not the full product: every M meets every K under every variant; every epilogue meets every variant; both N; 16-bit outputs of
    the operands' type and - every fourth 16-bit case - of the other one (fp16 operands with a bf16 output and the reverse)."""
    cases = []
    for i, (M, K) in enumerate(itertools.product((1, 127, 129, 300), (64, 128, 192, 256))):
        for v, (vname, dt, glds) in enumerate(VARIANTS):
            ename, epi, inplace, o16 = EPIS[(i + 4 * v) % len(EPIS)]
            N = (128, 384)[(i + v) % 2]
            od = F32 if not o16 else (OTHER[dt] if (i + v) % 4 == 3 else dt)
            cases.append(pytest.param(M, N, K, vname, ename, od, id=f"{vname}-M{M}-N{N}-K{K}-{ename}-{NAME[od]}"))
    return cases


def _epi(ename, N):
    for nm, epi, inplace, _ in EPIS:
        if nm == ename:
            epi = dict(epi)
            if epi.get("table") == "N":
                epi["table"] = N
            return epi, inplace
    raise KeyError(ename)


@pytest.mark.parametrize("M,N,K,vname,ename,od", route1_cases())
def test_route1_gemm_kernel(env, M, N, K, vname, ename, od):
    dt, glds = {v[0]: v[1:] for v in VARIANTS}[vname]
    epi, inplace = _epi(ename, N)
    run_route(env, "route1", f"{vname}-M{M}-N{N}-K{K}-{ename}-{NAME[od]}", M=M, N=N, K=K, dt=dt, out_dtype=od, family=5,
              seed=1000 + M + 3 * K + N, epi=epi, inplace=inplace, use_glds=glds)


# ---- route 2: q / k / v split and k / vT split on the 128 x 128 kernel

@pytest.mark.parametrize("dt,glds", [(BF, 0), (BF, 1), (H, 0)])
@pytest.mark.parametrize("head_dim,heads,tokens,K", [(64, 2, 65, 64), (80, 8, 70, 128)])
def test_route2_qkv_split(env, head_dim, heads, tokens, K, dt, glds):
    N = 3 * heads * head_dim
    run_route(env, "route2", f"qkv-hd{head_dim}-{NAME[dt]}-glds{glds}", M=2 * tokens, N=N, K=K, dt=dt, out_dtype=dt, family=5,
              seed=2000 + head_dim + glds, use_glds=glds, out_mode=1, heads=heads, head_dim=head_dim, tokens=tokens)


@pytest.mark.parametrize("dt,glds,K", [(BF, 0, 64), (BF, 1, 192), (H, 0, 128)])
def test_route2_kv_split(env, dt, glds, K):
    """tokens = 128, M = 256 (two images): k row-major, vT per (b, d, t); the positional table on the k half."""
    run_route(env, "route2", f"kv-{NAME[dt]}-glds{glds}-K{K}", M=256, N=256, K=K, dt=dt, out_dtype=dt, family=5, seed=2100 + K,
              epi=dict(table=128), use_glds=glds, out_mode=2, tokens=128)


# ---- route 3: out_mode 3, hi | lo | hi operand pairs (ldc == 3 N), ragged M

@pytest.mark.parametrize("dt,od", [(BF, BF), (H, H), (H, BF)])
@pytest.mark.parametrize("M,N,K,relu", [(129, 128, 128, True), (1, 384, 64, False), (300, 128, 192, True)])
def test_route3_hi_lo_pairs(env, M, N, K, relu, dt, od):
    run_route(env, "route3", f"hilo-{NAME[dt]}-{NAME[od]}-M{M}-N{N}-K{K}", M=M, N=N, K=K, dt=dt, out_dtype=od, family=5,
              seed=3000 + M + K, epi=dict(relu=relu), out_mode=3)


# ---- route 4: msam_gemm_group_bf16

def _group_items(dt, dev):
    """Five products of different M, N, K (2, 3, 4, 1 and 3 tiles: the grid is as wide as the largest, the others' surplus workgroups
    return at once) with different epilogues, one k / vT split and one hi | lo | hi item."""
    o = dt
    spec = [
        dict(M=129, N=128, K=64, od=F32, epi={}, launch={}),
        dict(M=1, N=384, K=192, od=o, epi=dict(table=4), launch={}),
        dict(M=256, N=256, K=128, od=o, epi=dict(table=128), launch=dict(out_mode=2, tokens=128)),
        dict(M=127, N=128, K=256, od=o, epi=dict(relu=True), launch=dict(out_mode=3)),
        dict(M=300, N=128, K=128, od=o, epi=dict(resid=dt, resid_rows=5), launch={}),
    ]
    items = []
    for i, s in enumerate(spec):
        c = G.exact_case(s["M"], s["N"], s["K"], dt, 4000 + i, out_dtype=s["od"], dev=dev, **s["epi"])
        items.append((c, s, dict(A=c["A"], W=c["W"], **_kw(c, s["od"], **s["launch"]))))
    return items


@pytest.mark.parametrize("dt", [BF, H])
@pytest.mark.parametrize("pick", [(1,), (3, 2), (0, 1, 2, 3, 4)])
def test_route4_group(env, pick, dt):
    pool = _group_items(dt, env)
    items = [pool[i] for i in pick]
    (status, res), fam = G.route_taken(lambda: G.call_group(env, [kw for _, _, kw in items]))
    assert fam == 5
    status2, res2 = G.call_group(env, [kw for _, _, kw in items])
    for (c, s, kw), r, r2 in zip(items, res, res2):
        what = f"route4 n={len(pick)} {NAME[dt]} item M={s['M']}"
        lay = {k: s["launch"][k] for k in ("tokens",) if k in s["launch"]}
        G.assert_bits(r, G.expected(c, env, out_mode=s["launch"].get("out_mode", 0), **lay), what + " exact")
        alone = G.call(env, **kw)
        G.assert_bits(r, alone.tensors(), what + " vs the same product launched alone")
        G.assert_bits(r2, r.tensors(), what + " second run")
    _fig("route4", f"n{len(pick)}-{NAME[dt]}", family=fam)


# ---- route 5: split-K

@pytest.mark.parametrize("dt", [BF, H])
@pytest.mark.parametrize("M,N,K,split", [(129, 128, 512, 8), (128, 256, 256, 2), (1, 128, 128, 2)])
def test_route5_split_k(env, M, N, K, split, dt):
    c = G.exact_case(M, N, K, dt, 5000 + M + K, bias=False, dev=env)
    kw = _kw(c, F32, split_k=split)
    r1, fam = G.route_taken(lambda: G.call(env, c["A"], c["W"], **kw))
    assert fam is None, f"split-K recorded a launch of family {fam}"
    G.assert_bits(r1, G.expected(c, env), "route5 exact")
    o = G.exact_case(130, 128, 256, dt, 5999, bias=False, dev=env)               # another shape in between: the workspace is reused
    G.assert_bits(G.call(env, o["A"], o["W"], **_kw(o, F32, split_k=4)), G.expected(o, env), "route5 other shape")
    G.assert_bits(G.call(env, c["A"], c["W"], **kw), r1.tensors(), "route5 second run after another shape")
    _fig("route5", f"{NAME[dt]}-M{M}-N{N}-K{K}-s{split}", family=fam)


# ---- route 6: gemm256_kernel (device only: the host suite keeps the emulation test of tests/test_gemm_kernel_host_emulation.py)

@pytest.fixture
def staging():
    from micro_sam_amd import _lib

    def set_(s):
        assert _lib.load().msam_gemm256_set_staging(s) == 0
    yield set_
    _lib.load().msam_gemm256_set_staging(-1)


def _gelu_checks(dev, route, name, c, pads, od16, family, **launch):
    """Route 9's checks for one launch configuration: pre-activation v from the twin launch without activation (same route, same bits);
    |GELU output - erf-GELU(v) in float64| <= design error of the approximation + 16 * 2^-24 * max(1, |v|) (six fp32 operations and the
    1-ulp exp2); finite, <= 0 and >= -1e-6 for v <= -8; the 16-bit GELU output == rne16 of the fp32 one."""
    design, _ = G.gelu_design_error()
    rv, fam = G.route_taken(lambda: G.call(dev, c["A"], c["W"], **_kw(c, F32, pads=pads, **launch)))
    assert fam == family
    v = rv.out.double()
    assert float(v.min()) <= -8.0 and float(v.max()) >= 8.0, (float(v.min()), float(v.max()))
    rg, fam = G.route_taken(lambda: G.call(dev, c["A"], c["W"], **_kw(c, F32, pads=pads, act=G.ACT_GELU, **launch)))
    assert fam == family
    g = rg.out.double()
    assert bool(torch.isfinite(g).all())
    allow = design + 16 * 2.0 ** -24 * v.abs().clamp(min=1.0)
    ratio = float(((g - G.gelu64(v)).abs() / allow).max())
    assert ratio <= 1.0, f"{route} {name}: GELU err / allowance = {ratio}"
    far = g[v <= -8.0]
    assert far.numel() > 0 and bool((far <= 0).all()) and bool((far >= -1e-6).all())
    r16 = G.call(dev, c["A"], c["W"], **_kw(c, od16, pads=pads, act=G.ACT_GELU, **launch))
    G.assert_bits(r16, {"out": G.rne16(rg.out, od16)}, f"{route} {name} 16-bit GELU output vs RNE of the fp32 one")
    _fig(route, name, family=fam, gelu_err_over_allowance=ratio, design_error=design)


R6_VARIANTS = [("st0", BF, 0), ("st1", BF, 1), ("st2", BF, 2), ("st3", BF, 3), ("fp16", H, 3)]
R6_EPIS = ["bias", "gelu16", "inplace", "qkv"]


def route6_cases():
    cases = []
    for i, K in enumerate((64, 128, 192, 320)):
        for v, (vname, dt, st) in enumerate(R6_VARIANTS):
            cases.append(pytest.param(vname, K, (3841, 4096)[(i + v) % 2], R6_EPIS[(i + v) % 4], id=f"{vname}-K{K}-{R6_EPIS[(i + v) % 4]}"))
    return cases


@pytest.mark.parametrize("vname,K,M,ename", route6_cases())
def test_route6_gemm256(env, staging, vname, K, M, ename):
    """N = 4096; M = 3841: exactly 16 x 16 = 256 tiles, the last row tile with one live row; K = 64 / 128 / 192 / 320 = 1, 2, 3, 5 k-tiles."""
    dt, st = {v[0]: v[1:] for v in R6_VARIANTS}[vname]
    staging(st)
    name = f"{vname}-M{M}-K{K}-{ename}"
    if ename == "qkv":
        run_route(env, "route6", name, M=3585, N=4608, K=K, dt=dt, out_dtype=dt, family=0, seed=6000 + K, out_mode=1, heads=24,
                  head_dim=64, tokens=239)
    elif ename == "gelu16":
        _gelu_checks(env, "route6", name, G.random_case(M, 4096, K, dt, 6100 + K, scale=3.0, dev=env), (8, 16, 4), dt, 0)
    elif ename == "inplace":
        run_route(env, "route6", name, M=M, N=4096, K=K, dt=dt, out_dtype=F32, family=0, seed=6200 + K, epi=dict(resid=F32), inplace=True)
    else:
        run_route(env, "route6", name, M=M, N=4096, K=K, dt=dt, out_dtype=(F32, dt)[K // 64 % 2], family=0, seed=6300 + K)


@pytest.mark.parametrize("name,M,dt,od,family,epi,launch", [
    ("240-tiles", 3840, BF, BF, 5, {}, {}),
    ("256-tiles", 3841, BF, BF, 0, {}, {}),
    ("256-tiles-glds", 3841, BF, F32, 5, {}, dict(use_glds=1)),
    ("256-tiles-table", 3841, BF, F32, 5, dict(table=128), {}),
    ("256-tiles-resid-wrap", 3841, BF, F32, 5, dict(resid=F32, resid_rows=5), {}),
    ("256-tiles-resid-bf16", 3841, BF, F32, 5, dict(resid=BF), {}),
    ("256-tiles-fp16-operands-bf16-output", 3841, H, BF, 5, {}, {}),
    ("256-tiles-bf16-operands-fp16-output", 3841, BF, H, 5, {}, {}),
])
def test_route6_dispatch_boundary(env, name, M, dt, od, family, epi, launch):
    """The launcher's 256-tile threshold and each of its fall-backs to the 128 x 128 kernel, exact either way.  (gemm256_kernel packs
    16-bit outputs by its OPERAND type, so a 16-bit output of the other type has to stay on the 128 x 128 kernel in both directions.)"""
    run_route(env, "route6-dispatch", name, M=M, N=4096, K=64, dt=dt, out_dtype=od, family=family, seed=6400 + M, epi=epi, **launch)


# ---- route 7: fp8 e4m3 operands (always gemm256_kernel<1, FP8>; no tile threshold)

R7_EPIS = [("plain", 256), ("inplace", 512), ("qkv", 768), ("bf16", 256), ("plain", 512), ("bf16", 512)]


def route7_cases():
    return [pytest.param(M, K, *R7_EPIS[i % len(R7_EPIS)], id=f"M{M}-K{K}-{R7_EPIS[i % len(R7_EPIS)][0]}-N{R7_EPIS[i % len(R7_EPIS)][1]}")
            for i, (M, K) in enumerate(itertools.product((1, 37, 257), (128, 256, 384)))]


@pytest.mark.parametrize("M,K,ename,N", route7_cases())
def test_route7_fp8(env, M, K, ename, N):
    """lda = K + 16; power-of-two row / column scales keep (a) exact: acc * rs * cs + bias is one exactly representable value."""
    name, pads = f"M{M}-N{N}-K{K}-{ename}", (16, 32, 4)
    if ename == "qkv":
        M2 = M if M > 1 else 2
        run_route(env, "route7", name, M=M2, N=N, K=K, dt=F8, out_dtype=BF, family=0, seed=7000 + M + K, pads=pads, out_mode=1, heads=4,
                  head_dim=64, tokens=M2 if M2 % 2 else M2 // 2)
    elif ename == "inplace":
        run_route(env, "route7", name, M=M, N=N, K=K, dt=F8, out_dtype=F32, family=0, seed=7000 + M + K, pads=pads, epi=dict(resid=F32),
                  inplace=True)
    else:
        run_route(env, "route7", name, M=M, N=N, K=K, dt=F8, out_dtype=BF if ename == "bf16" else F32, family=0, seed=7000 + M + K, pads=pads)


# ---- route 8: gemm_ln_kernel

R8_EPIS = [("table", dict(table=128)), ("resid16-wrap5", dict(resid="dt", resid_rows=5)), ("inplace", dict(resid=F32))]


def route8_cases():
    cases = []
    for i, (M, K) in enumerate(itertools.product((1, 63, 65, 130), (64, 128, 192))):
        for dt in (BF, H):
            j = i + (dt == H)
            cases.append(pytest.param(M, K, dt, 1 + (j // 3 + i) % 2, R8_EPIS[j % 3][0], id=f"{NAME[dt]}-M{M}-K{K}-mode{1 + (j // 3 + i) % 2}-{R8_EPIS[j % 3][0]}"))
    return cases


LN_TOL = (2e-4, 1e-4)            # tests/test_gpu_kernels.py test_gemm_fused_layernorm, fp32 output


@pytest.mark.parametrize("M,K,dt,mode,ename", route8_cases())
def test_route8_fused_layernorm(env, M, K, dt, mode, ename):
    """LayerNorm is not integer-exact:
    * the fp32 output against a float64 LayerNorm (+ exact GELU, mode 2) of the float64 pre-activation at 2e-4 + 1e-4 |ref|;
    * ``out`` in the 16-bit type, ``ln_out_b`` and ``ln_out_a`` with and without ``ln_add`` (mode 1) == the RNE casts of the fp32 ``out`` of
      the twin launch, bit for bit (out_a = rne16(out32 + ln_add), the sum in fp32);
    * integer rows: a constant row (pre-activation 1000 in all 256 columns) must give ln_b exactly (mode 2: the GELU of it, within the
      bound) and finite; a row 4096 + d, d in [-2, 2], within the bound - the two-pass variance."""
    dev = env
    epi = dict(dict(R8_EPIS)[ename])
    inplace = ename == "inplace"
    if epi.get("resid") == "dt":
        epi["resid"] = dt
    g = torch.Generator().manual_seed(8000 + M + K + mode)
    eps = 1e-5 if mode == 1 else 1e-6
    nw = 256 if mode == 1 else 64
    ln_w, ln_b = torch.randn(nw, generator=g) * 0.2 + 1, torch.randn(nw, generator=g)
    add = torch.randn(M, 256, generator=g)
    c = G.random_case(M, 256, K, dt, 8100 + M + K, dev=dev, **epi)
    ln = dict(ln_mode=mode, ln_w=ln_w, ln_b=ln_b, ln_eps=eps)
    ref = G.layernorm64(c["ref"].to(dev), ln_w.to(dev), ln_b.to(dev), eps, mode)
    r32, fam = G.route_taken(lambda: G.call(dev, c["A"], c["W"], **_kw(c, F32, inplace=inplace, **ln)))
    assert fam == 5
    ratio = G.err_over_tol(r32.out, ref, *LN_TOL)
    assert ratio <= 1.0, f"route8: fp32 output vs float64 LayerNorm: err / tol = {ratio}"
    G.assert_bits(G.call(dev, c["A"], c["W"], **_kw(c, F32, inplace=inplace, **ln)), r32.tensors(), "route8 second run")
    r16 = G.call(dev, c["A"], c["W"], **_kw(c, dt, ln_out_b=mode == 1, ln_out_a=mode == 1, ln_add=add if mode == 1 else None, **ln))
    exp = {"out": G.rne16(r32.out, dt)}
    if mode == 1:
        exp["out_b"] = exp["out"]
        exp["out_a"] = G.rne16(r32.out + add.to(dev), dt)
    G.assert_bits(r16, exp, "route8 16-bit outputs vs RNE of the fp32 twin")
    if mode == 1:
        ra = G.call(dev, c["A"], c["W"], **_kw(c, OTHER[dt], ln_out_a=True, **ln))          # out_a without ln_add; out in the other 16-bit type
        G.assert_bits(ra, {"out": G.rne16(r32.out, OTHER[dt]), "out_a": exp["out"]}, "route8 ln_out_a without ln_add")
    # integer rows through an fp32 residual in place: the last row constant, the first (if there are two) 4096 + d
    ci = G.exact_case(M, 256, K, dt, 8200 + M + K, bias=False, check_shares=False)
    ci["bias"] = torch.randint(-8, 9, (256,), generator=g).float()
    ci["A"][M - 1] = 0
    res = torch.randint(-1000, 1001, (M, 256), generator=g).float()
    res[M - 1] = 1000 - ci["bias"]
    if M > 1:
        ci["A"][0] = 0
        res[0] = 4096 + torch.randint(-2, 3, (256,), generator=g).float() - ci["bias"]
    ci["resid"] = res
    pre = G.preact64(ci, dev)
    assert bool((pre[M - 1] == 1000).all()) and (M == 1 or bool(((pre[0] - 4096).abs() <= 2).all()))
    ri = G.call(dev, ci["A"], ci["W"], **_kw(ci, F32, inplace=True, **ln))
    refi = G.layernorm64(pre, ln_w.to(dev), ln_b.to(dev), eps, mode)
    assert bool(torch.isfinite(ri.out).all())
    if mode == 1:
        G.assert_bits({"out": ri.out[M - 1]}, {"out": ln_b}, "route8 constant row == ln_b")
    ratio_i = G.err_over_tol(ri.out, refi, *LN_TOL)
    assert ratio_i <= 1.0, f"route8: integer rows vs float64 LayerNorm: err / tol = {ratio_i}"
    _fig("route8", f"{NAME[dt]}-M{M}-K{K}-mode{mode}-{ename}", family=fam, err_over_tol=ratio, integer_rows_err_over_tol=ratio_i)


# ---- route 9: GELU epilogue of the 128 x 128 kernel (the 256 x 256 kernel's: route 6, "gelu16")

@pytest.mark.parametrize("vname,M,N,K", [("bf16", 300, 128, 128), ("bf16-glds", 129, 384, 64), ("fp16", 127, 128, 192)])
def test_route9_gelu(env, vname, M, N, K):
    dt, glds = {v[0]: v[1:] for v in VARIANTS}[vname]
    _gelu_checks(env, "route9", f"{vname}-M{M}-N{N}-K{K}", G.random_case(M, N, K, dt, 9000 + K, scale=3.0, dev=env), (8, 16, 4), dt, 5, use_glds=glds)


# ---- argument refusals: non-zero status, outputs untouched (G.call checks the sentinels of a refused call)

def _plain(dt=BF, M=128, N=128, K=64):
    return G.exact_case(M, N, K, dt, 9900, bias=False)


def test_refusals_single(env):
    """Each refused call differs from an accepted one in the offending field alone."""
    ln2 = dict(ln_mode=2, ln_w=torch.ones(64), ln_b=torch.zeros(64))
    for what, (N, K), good, bad in [
            ("out_mode 3 with an fp32 output", (128, 64), dict(out_mode=3, out_dtype=BF), dict(out_mode=3, out_dtype=F32)),
            ("out_mode 3 with ldc != 3 N", (128, 64), dict(out_mode=3, out_dtype=H), dict(out_mode=3, out_dtype=H, ldc=3 * 128 + 4)),
            ("split-K with ldc != N", (128, 128), dict(split_k=2), dict(split_k=2, ldc=132)),
            ("ln_out_a with ln_mode 2", (256, 64), ln2, dict(ln2, ln_out_a=True))]:
        c = _plain(N=N, K=K)
        assert G.call(env, c["A"], c["W"], **good).status == 0, what
        r = G.call(env, c["A"], c["W"], expect_ok=False, **bad)
        assert r.status != 0 and r.error, what
    f8 = G.exact_case(4, 256, 128, F8, 9901, bias=False)
    sc = dict(row_scale=f8["row_scale"], col_scale=f8["col_scale"])
    assert G.call(env, f8["A"], f8["W"], out_dtype=BF, **sc).status == 0
    for what, bad in [("fp8 with a table", dict(table=torch.zeros(7, 128))), ("fp8 with use_glds", dict(use_glds=1)),
                      ("fp8 with an fp16 output (the kernel packs bf16)", dict(out_dtype=H))]:
        r = G.call(env, f8["A"], f8["W"], expect_ok=False, **sc, **bad)
        assert r.status != 0 and r.error, what


def test_refusals_group(env):
    c, h = _plain(), _plain(H)
    item = dict(A=c["A"], W=c["W"])
    item_h = dict(A=h["A"], W=h["W"])
    q = G.exact_case(128, 384, 64, BF, 9903, bias=False)
    for what, items, n in [("n = 0", [item], 0), ("n = 6", [item] * 6, 6),
                           ("a qkv-split item", [item, dict(A=q["A"], W=q["W"], out_dtype=BF, out_mode=1, heads=2, head_dim=64, tokens=64)], None),
                           ("mixed fp16 / bf16 items", [item, item_h], None)]:
        status, res = G.call_group(env, items, expect_ok=False, n=n)
        assert status != 0, what
    assert G.call_group(env, [item, item])[0] == 0
