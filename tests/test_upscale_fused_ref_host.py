"""The proof behind tests/test_gpu_upscale_fused.py, on the CPU.

1. The fp64 reference of tests/upscale_fused_ref.py equals torch's conv_transpose2d formulation of the operation.
2. The bound is not too tight for an honest kernel: the arithmetic restated in fp64 with a rounding at exactly the kernel's rounding
   points lies within ONE bound of the reference on every generator, for every LayerNorm form, both GELU forms and both 16-bit types; the
   running error analysis of the packed-fp16 GELU covers the emulated nine operations on ALL fp16 inputs.
3. Every defect of upscale_fused_ref.MUTATIONS (the kernel's typical ones, and "eps_slip": a LayerNorm eps of 1e-5 for 1e-6) is caught
   by the criterion meant for it, on a named generator (CASES below):
     bound   at least 4 elementwise bounds from the reference (a kernel within one bound of the truth is then 3 bounds from the mutant);
     mean    every (prompt, mask) plane's mean error above 1.5 x the restatement's (the device test's mean criterion).  No defect of the list
             NEEDS it - each is either 4 bounds out or invisible to it as well - so its figure is printed next to the bound's for every
             mutant of the first kind: it is the sharper of the two wherever a defect touches a whole plane (no_b1: 23 bounds, 800 x the mean);
     diff    out(a + d) - out(a) outside the differential bound.
   INVISIBLE to all three, and shown to be so below:
     "out16_truncated" (an fp16 output that is the fp32 output with its low bits cut off instead of rounded): at most one fp16 ulp of the
         output, inside the bound, plane means 1.2 - 1.4 x the restatement's.  What catches it on the device is the exact invariant "the fp16
         output is the fp16 rounding of the fp32 output".
     "tanh_gelu": the tanh approximation is within 4.8e-4 of erf-GELU, the size of ONE fp16 rounding of a GELU argument of 1: alone it is
         0.1 - 0.9 of the restatement's mean error, and a restatement with a once-rounded tanh-GELU in place of either GELU form has 0.8 - 1.3 x
         the mean error of the honest one (BELOW it against the nine roundings of the packed-fp16 form).  Nothing on the device catches it; a
         kernel with it would be a different, equally accurate GELU.
4. The real kernel source on the host shim (built as tests/test_upfused_kernel_host_emulation.py builds it, with an entry that takes KS, the
   grid, out16 and the range map) lies inside the bound and the mean criterion for KS in {1, 2, 4, 8, 16}, grids smaller than, equal to and
   larger than the item count (uneven shares, a workgroup with nothing to do), P up to 3, in every instantiation the launcher can reach.
   LEFT OUT: up_gelu16 = 2 (no exponential: wrong by design, a timing experiment) and 3 (a packed-exponential experiment).
5. The generators' stated domains hold.

Every test prints its figure (pytest -s); profiles/r15_upscale_fused_err.md records them."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upscale_fused_ref as R
from hip_host_shim import build
from test_upfused_kernel_host_emulation import DEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
DIDS = ["bf16", "fp16"]

# mutation -> (criterion, generator, P, KS, grid, keyword arguments of make)
CASES = {
    "last_tile_not_stored": ("bound", "diffuse", 3, 1, 2, {}),
    "last_tile_next_base": ("bound", "diffuse", 3, 1, 2, {}),
    "first_tile_stale_hyper": ("bound", "diffuse", 3, 1, 2, {}),
    "tile_repeated_at_clamp": ("bound", "diffuse", 3, 1, 2, {}),
    "split_rows_crossed": ("bound", "diffuse", 2, 4, 8, {}),
    "subpixels_crossed": ("bound", "diffuse", 1, 16, 16, {}),
    "mask0_ignored": ("bound", "diffuse", 2, 16, 32, {}),
    "mask_rows_crossed": ("bound", "diffuse", 2, 16, 32, {}),
    "hyper_ld_128": ("bound", "diffuse", 3, 16, 48, {"hyper_ld": 36}),
    "hyper_channels_32": ("bound", "diffuse", 2, 16, 32, {}),
    "no_b1": ("bound", "diffuse", 1, 16, 16, {}),
    "no_b2": ("bound", "diffuse", 1, 16, 16, {}),
    "no_ln_b": ("bound", "diffuse", 1, 16, 16, {}),
    "no_eps": ("bound", "flat", 1, 16, 16, {}),
    "eps_slip": ("bound", "flat", 1, 16, 16, {}),
    "ln_wrong_64": ("bound", "diffuse", 1, 16, 16, {}),
    "blocked_as_row_major": ("bound", "diffuse", 1, 16, 16, {}),
    "tanh_gelu": ("invisible", "diffuse", 1, 16, 16, {}),
    "hyper_lo_dropped": ("diff", "hyper_pair", 1, 16, 16, {}),
    "out16_truncated": ("invisible", "diffuse", 1, 16, 16, {}),
}


def _routes(dtype):
    """(the shipped route of the type's build, the other GELU form where the build has one)"""
    return [R.route("cen", True), R.route("cen", False)] if dtype == torch.float16 else [R.route("cen", False)]


def _ratio(err, bound):
    r = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))          # (a non-finite mutant is as far as can be)
    return float(r.max())


@functools.lru_cache(maxsize=None)
def _truth(gen, dtype, P, ln, gelu16, out16=False, **kw):
    inp = R.make(gen, dtype, P, centred=(ln == "cen"), seed=1, **kw)
    rt = R.route(ln, gelu16, out16)
    return inp, rt, R.ref(inp, rt)


def test_every_mutation_has_a_case_and_the_key_splits_follow_the_launcher():
    assert set(CASES) == set(R.MUTATIONS)
    cus = 256
    assert [R.key_splits(P, cus) for P in (1, 31, 32, 33, 63, 64, 127, 128, 255, 256, 511, 512, 513)] == \
        [(16, 16), (16, 496), (16, 512), (16, 512), (16, 512), (8, 512), (8, 512), (4, 512), (4, 512), (2, 512), (2, 512), (1, 512), (1, 512)]
    assert R.key_splits(3, 304) == (16, 48) and R.key_splits(75, 304) == (16, 608) and R.key_splits(76, 304) == (8, 608)
    assert R.key_splits(607, 304) == (2, 608) and R.key_splits(609, 304) == (1, 608)


# --------------------------------------------------------------------------------------------------------------- 1. the reference
def test_reference_is_torchs_conv_transpose_formulation():
    inp = R.make("diffuse", torch.float16, 2, centred=False, seed=3, hyper_ld=36, mask0=0, nmask=3)
    ct1 = inp["w1"].double().reshape(2, 2, 64, 256).permute(3, 2, 0, 1)                            # [in, out, kh, kw]
    ct2 = inp["w2"].double().reshape(2, 2, 32, 64).permute(3, 2, 0, 1)
    src = inp["keys"].double().transpose(1, 2).reshape(2, 256, 64, 64)
    up = F.conv_transpose2d(src, ct1, inp["b1"][:64].double(), stride=2)
    mu = up.mean(1, keepdim=True)
    var = ((up - mu) ** 2).mean(1, keepdim=True)
    up = (up - mu) / torch.sqrt(var + R.f32(1e-6)) * inp["ln_w"].double().view(1, -1, 1, 1) + inp["ln_b"].double().view(1, -1, 1, 1)
    up = F.gelu(F.conv_transpose2d(F.gelu(up), ct2, inp["b2"].double(), stride=2))
    want = torch.einsum("nmc,nchw->nmhw", inp["hyper"][:, 0:3, :32].double(), up)
    got, _ = R.ref(inp)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"\nreference against conv_transpose2d: max difference {err:.2e} of the scale")
    assert err <= 1e-12
    assert torch.equal(R.unpixels(R.pixels(got.reshape(2, 3, 4096, 4, 4))), got.reshape(2, 3, 4096, 4, 4))


# --------------------------------------------------------------------------------------------------------------- 2. honest from below
def test_packed_fp16_gelu_analysis_covers_every_fp16_input():
    x = R._all_fp16()
    x = x[x.abs() <= 4096.0]
    err = (R.gelu_pk16(x) - R.gelu_erf(x)).abs()
    bound = R.gelu_err(x, torch.zeros_like(x), True, R.UH, R.SUBH)
    print(f"\npacked-fp16 GELU over {x.numel()} fp16 inputs: max error {float(err.max()):.3e}, max error / analysis {float((err / bound).max()):.3f}; "
          f"formula distance {R.A_FORMULA:.3e}, K32 {R.K32:.3f}")
    assert float((err / bound).max()) <= 1.0
    assert 4e-5 <= R.A_FORMULA <= 7e-5 and R.K32 <= 2.0
    dense = torch.linspace(-12.0, 12.0, 200001, dtype=torch.float64)
    d = (R.gelu_erf(dense[1:]) - R.gelu_erf(dense[:-1])).abs() / (dense[1] - dense[0])
    assert float(d.max()) <= R.GELU_SLOPE                                                         # erf-GELU's slope


def _restate_cases():
    for dtype, did in zip(DTYPES, DIDS):
        for gen in R.GENERATORS:
            for ln in R.ROUTE_LN:
                if (gen == "large_mean") and ln == "cen":
                    continue
                for g16 in ((True, False) if dtype == torch.float16 else (False,)):
                    yield pytest.param(gen, dtype, ln, g16, id=f"{gen}-{did}-{ln}-{'gelu16' if g16 else 'gelu32'}")


@pytest.mark.parametrize("gen,dtype,ln,g16", list(_restate_cases()))
def test_rounded_restatement_is_within_one_bound(gen, dtype, ln, g16):
    inp, rt, (ref, bound) = _truth(gen, dtype, 1, ln, g16)
    assert bool(torch.isfinite(bound).all()), "sig - E2 <= 0: outside the bound's domain"
    worst = 0.0
    for out16 in (False, True):
        rt2 = dict(rt, out16=out16)
        b = R.ref(inp, rt2)[1] if out16 else bound
        worst = max(worst, _ratio((R.restate(inp, rt2) - ref).abs(), b))
    print(f"\nrestatement / {gen} / {ln} / gelu16={g16}: max |restated - ref| / bound = {worst:.3f}; "
          f"median bound {float(bound.median() / ref.abs().max()):.2e} of the scale")
    assert worst <= 1.0, worst


# --------------------------------------------------------------------------------------------------------------- 3. mutations
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutation_is_caught_by_its_criterion(mutation, dtype):
    crit, gen, P, ks, grid, kw = CASES[mutation]
    for rt0 in _routes(dtype):
        out16 = mutation == "out16_truncated"
        inp, rt, (ref, bound) = _truth(gen, dtype, P, rt0["ln"], rt0["gelu16"], out16, **kw)
        what = f"{mutation} / {gen} / {DIDS[DTYPES.index(dtype)]} / gelu16={rt['gelu16']}"
        if crit == "bound":
            mut = R.mutated(inp, mutation, ks, grid)
            ratio = _ratio((mut - ref).abs(), bound)
            means = R.plane_means(torch.nan_to_num(mut - ref, nan=1e30, posinf=1e30, neginf=1e30)) / R.plane_means(R.restate(inp, rt) - ref)
            print(f"\n{what}: max |mutant - ref| / bound = {ratio:.1f}; plane means {float(means.min()):.3g} .. {float(means.max()):.3g} x the restatement's")
            assert ratio >= 4.0, ratio
        elif crit == "mean":
            base = R.plane_means(R.restate(inp, rt) - ref)
            mut = R.plane_means(R.restate(inp, rt, mutation=mutation) - ref)
            print(f"\n{what}: mean |mutant - ref| / mean |restated - ref| per plane = {(mut / base).flatten().tolist()}")
            assert bool((mut > R.MEAN_MARGIN * base).all())
        elif crit == "diff":
            got = R.mutated(dict(inp, hyper=inp["hyper_d"]), mutation, rt=rt) - R.mutated(inp, mutation, rt=rt)
            honest = R.restate(dict(inp, hyper=inp["hyper_d"]), rt) - R.restate(inp, rt)
            (_, _, want, dbound), = R.diff_bound_chunks(inp, inp["hyper_d"], rt, chunk=P)
            r_mut, r_ok = _ratio((got - want).abs(), dbound), _ratio((honest - want).abs(), dbound)
            print(f"\n{what}: |difference - d.G2| / differential bound: mutant {r_mut:.1f}, restatement {r_ok:.3f}")
            assert r_mut >= 4.0 and r_ok <= 1.0
            # ... and the elementwise bound of the plain launch does not see it
            assert _ratio((R.mutated(inp, mutation, rt=rt) - ref).abs(), bound) <= 1.0
        else:
            mut, ok = R.restate(inp, rt, mutation=mutation), R.restate(inp, rt)
            ratio = _ratio((mut - ref).abs(), bound)
            means = (R.plane_means(mut - ref) / R.plane_means(ok - ref)).flatten()
            print(f"\n{what}: INVISIBLE to the three criteria: max |mutant - ref| / bound = {ratio:.3f}, plane means {means.tolist()} of the "
                  f"restatement's; the exact invariant sees {int((mut != ok).sum())} of {mut.numel()} elements differ")
            assert ratio < 4.0 and float(means.max()) <= R.MEAN_MARGIN
            if mutation == "out16_truncated":
                assert torch.equal(ok, R.restate(inp, dict(rt, out16=False)).to(torch.float16).double()) and not torch.equal(mut, ok)


# --------------------------------------------------------------------------------------------------------------- 4. the kernel source
ENTRY = r"""
extern "C" void emu_up_fused_geo(int inst, const u16* keys, int blocked, int P, int KS, int grid, const u16* w1, const float* b1, const float* lnw,
                                 const float* lnb, float eps, const u16* w2, const float* b2, const float* hyper, int hyper_ld, int mask0, int nmask,
                                 void* out, int out16, float* range) {
    UpArgs a{};
    a.keys = keys; a.w1 = w1; a.b1 = b1; a.lnw = lnw; a.lnb = lnb; a.eps = eps; a.w2 = w2; a.b2 = b2; a.hyper = hyper; a.hyper_ld = hyper_ld;
    a.mask0 = mask0; a.nmask = nmask; a.KS = KS; a.nitems = P * KS; a.out = out; a.out16 = out16; a.blocked = blocked; a.range = range;
    switch (inst) {                                                      // every instantiation msam_upscale_fused_range can launch (up_gelu16 <= 1)
    case 0: launch_grid(grid, 1, [=] { up_fused_kernel<1, 0>(a); }); break;
    case 1: launch_grid(grid, 1, [=] { up_fused_kernel<1, 1>(a); }); break;
    case 2: launch_grid(grid, 1, [=] { up_fused_kernel<0, 0>(a); }); break;
    case 3: launch_grid(grid, 1, [=] { up_fused_kernel<0, 1>(a); }); break;
    case 4: launch_grid(grid, 1, [=] { up_fused_kernel<1, 0, 1>(a); }); break;
    case 5: launch_grid(grid, 1, [=] { up_fused_kernel<1, 1, 1>(a); }); break;
    case 6: launch_grid(grid, 1, [=] { up_fused_kernel<1, 0, 0, 1>(a); }); break;
    case 7: launch_grid(grid, 1, [=] { up_fused_kernel<1, 1, 0, 1>(a); }); break;
    case 8: launch_grid(grid, 1, [=] { up_fused_kernel<1, 0, 0, 2>(a); }); break;
    case 9: launch_grid(grid, 1, [=] { up_fused_kernel<1, 1, 0, 2>(a); }); break;
    case 10: launch_grid(grid, 1, [=] { up_fused_kernel<1, 0, 0, 3>(a); }); break;
    default: launch_grid(grid, 1, [=] { up_fused_kernel<1, 1, 0, 3>(a); }); break;
    }
}
"""
# instantiation -> (LayerNorm form, packed-fp16 GELUs, range map)
INST = {0: ("one_pass", False, False), 1: ("one_pass", True, False), 2: ("one_pass", False, False), 3: ("one_pass", True, False),
        4: ("two_pass", False, False), 5: ("two_pass", True, False), 6: ("cen", False, False), 7: ("cen", True, False),
        8: ("one_pass", False, True), 9: ("one_pass", True, True), 10: ("cen", False, True), 11: ("cen", True, True)}
# (instantiation, generator, P, KS, grid, blocked, out16, hyper_ld, mask0, nmask)
EMU_CASES = [
    (7, "diffuse", 1, 1, 1, 0, 0, 128, 1, 3),           # one workgroup walks the 256 tiles of a prompt
    (11, "diffuse", 3, 1, 2, 0, 0, 36, 0, 3),           # KS = 1, uneven shares: workgroup 0 changes prompt, output base and hyper weights
    (6, "wide", 3, 1, 5, 1, 0, 32, 2, 2),               # KS = 1, a grid larger than the item count: two workgroups with nothing to do; blocked stream
    (1, "flat", 2, 2, 3, 0, 0, 128, 1, 3),              # KS = 2, uneven shares
    (10, "flat", 1, 2, 2, 0, 0, 128, 0, 1),
    (9, "diffuse", 1, 4, 4, 1, 0, 128, 3, 1),           # KS = 4, a grid equal to the item count
    (0, "large_mean", 1, 4, 3, 0, 0, 128, 0, 2),
    (5, "large_mean", 1, 8, 11, 0, 0, 128, 1, 2),       # KS = 8, a grid larger than the item count
    (8, "wide", 1, 8, 3, 0, 0, 32, 0, 3),               # KS = 8, uneven shares (3, 3, 2)
    (4, "large_mean", 1, 16, 5, 0, 1, 128, 1, 3),       # KS = 16, a grid smaller than the item count, fp16 output
    (3, "wide", 1, 16, 16, 0, 1, 36, 2, 1),             # priority 0
    (2, "diffuse", 1, 16, 7, 1, 0, 128, 0, 3),
    (7, "wide", 2, 1, 1, 0, 1, 128, 1, 3),              # the shipped instantiation, one workgroup, two prompts, fp16 output
]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    common = open(os.path.join(ROOT, "micro_sam_amd", "csrc", "common.h")).read()
    a = common.index("MSAM_DEVINL float relu1(float x)")
    gelu = common[a:common.index("// round-to-nearest-even fp32 -> packed fp16", a)]
    text = open(os.path.join(ROOT, "micro_sam_amd", "csrc", "upfused.hip")).read()
    s0 = text.index("constexpr int SUB_BYTES = TK * 64 + 64")
    s1 = text.index("// erf-GELU of two values in PACKED fp16 arithmetic")
    k0 = text.index("template <int UF_PRIO, int G16, int LN2P = 0, int CEN = 0>")
    k1 = text.index("}  // namespace", k0)
    lib = build(str(tmp_path_factory.mktemp("emu_up_geo")), "upgeo", DEC + gelu + text[s0:s1] + text[k0:k1], ENTRY)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_up_fused_geo.argtypes = [i, vp, i, i, i, i, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, i, i, i, vp, i, vp]
    return lib


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _f32(t):
    return t.numpy().astype(np.float32).copy()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _launch(lib, inst, inp, ks, grid, blocked, out16, want_range):
    P, nmask = inp["keys"].shape[0], inp["nmask"]
    keys = R.to_blocked(inp["keys"]) if blocked else inp["keys"]
    arrs = [_bits(keys), _bits(inp["w1"]), _f32(inp["b1"]), _f32(inp["ln_w"]), _f32(inp["ln_b"]), _bits(inp["w2"]), _f32(inp["b2"]), _f32(inp["hyper"])]
    guard, n = 4096, P * nmask * 65536
    SENT = -12345.5
    if out16:
        buf = np.full(guard + n + guard, 0x7e00, np.uint16)                              # fp16 NaN: prefill and guard zones
    else:
        buf = np.full(guard + n + guard, np.nan, np.float32)
        buf[:guard] = SENT
        buf[-guard:] = SENT
    rbuf = np.full(64 + n // 32 + 64, SENT, np.float32)
    out, rng = buf[guard:guard + n], rbuf[64:-64]
    lib.emu_up_fused_geo(inst, _ptr(arrs[0]), blocked, P, ks, grid, _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]), _ptr(arrs[4]), inp["eps"], _ptr(arrs[5]),
                         _ptr(arrs[6]), _ptr(arrs[7]), inp["hyper"].shape[-1], inp["mask0"], nmask, _ptr(out), out16, _ptr(rng) if want_range else None)
    if out16:
        assert (buf[:guard] == 0x7e00).all() and (buf[-guard:] == 0x7e00).all(), "a store outside the output"
        got = torch.from_numpy(out.view(np.float16).astype(np.float64))
    else:
        assert (buf[:guard] == SENT).all() and (buf[-guard:] == SENT).all(), "a store outside the output"
        got = torch.from_numpy(out.astype(np.float64))
    assert (rbuf[:64] == SENT).all() and (rbuf[-64:] == SENT).all(), "a store outside the range map"
    if not want_range:
        assert (rng == SENT).all()
    return got.reshape(P, nmask, 256, 256), torch.from_numpy(rng.copy()).reshape(P, nmask, 256, 4, 2)


@pytest.mark.parametrize("case", EMU_CASES, ids=lambda c: f"inst{c[0]}-{c[1]}-P{c[2]}-KS{c[3]}-grid{c[4]}-{'blocked' if c[5] else 'rows'}-{'f16' if c[6] else 'f32'}-ld{c[7]}-m{c[8]}+{c[9]}")
def test_kernel_source_on_the_cpu_is_inside_the_bound_and_the_mean_criterion(emu, case):
    inst, gen, P, ks, grid, blocked, out16, ld, mask0, nmask = case
    ln, g16, want_range = INST[inst]
    inp = R.make(gen, torch.float16, P, centred=(ln == "cen"), hyper_ld=ld, mask0=mask0, nmask=nmask, seed=2)
    rt = R.route(ln, g16, bool(out16))
    got, rng = _launch(emu, inst, inp, ks, grid, blocked, out16, want_range)
    assert bool(torch.isfinite(got).all()), "pixels never stored (the NaN prefill) or a non-finite result"
    ref, bound = R.ref(inp, rt)
    ratio = _ratio((got - ref).abs(), bound)
    base = R.plane_means(R.restate(inp, rt) - ref)
    means = R.plane_means(got - ref) / base
    print(f"\nkernel source on the host, instantiation {inst} ({ln}, gelu16={g16}), {gen} P={P} KS={ks} grid={grid}: max |got - ref| / bound = {ratio:.3f}, "
          f"mean ratio {float(means.min()):.3f} .. {float(means.max()):.3f}")
    assert ratio <= 1.0, ratio
    assert float(means.max()) <= R.MEAN_MARGIN, means
    if want_range:
        seg = got.float().reshape(P, nmask, 256, 4, 64)
        assert torch.equal(rng, torch.stack([seg.amin(-1), seg.amax(-1)], -1)), "the range map is not the segments' {min, max}"
    if out16:                                            # the fp16 output is the rounding of the fp32 output of the same launch
        got32, _ = _launch(emu, inst, inp, ks, grid, blocked, 0, False)
        assert torch.equal(got32.to(torch.float16).double(), got)


def test_kernel_source_on_the_cpu_does_not_depend_on_the_launch_geometry(emu):
    """Per-token arithmetic: the same bits whatever KS and the grid are, and for a prompt launched alone."""
    inp = R.make("diffuse", torch.float16, 2, centred=True, seed=4)
    a, _ = _launch(emu, 7, inp, 1, 2, 0, 0, False)
    b, _ = _launch(emu, 7, inp, 4, 3, 0, 0, False)
    c, _ = _launch(emu, 7, R.first_prompts(inp, slice(1, 2)), 16, 16, 0, 0, False)
    assert torch.equal(a, b) and torch.equal(a[1:2], c)


# --------------------------------------------------------------------------------------------------------------- 5. generator domains
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_generators_keep_their_promises(dtype):
    for gen in R.GENERATORS:
        inp = R.make(gen, dtype, 2, centred=(gen != "large_mean"), seed=1)
        st = R._first_stages(inp, 0, 2)
        assert float(inp["hyper"].abs().max()) < 60000 and float(st["g2"].abs().max()) < 60000 and float(st["g1"].abs().max()) < 60000
        x1, y = st["x1"], st["y"]
        if gen == "wide":
            for x in (x1, y):
                assert float(x.min()) < -9 and float(x.max()) > 9 and float((x.abs() < 0.5).double().mean()) > 0.05
                assert float((x < -5.5).double().mean()) > 0.01                          # the packed-fp16 exponential's flushed tail (q < -25)
        if gen == "flat":
            var = st["sig"] ** 2 - R.f32(inp["eps"])
            t = torch.arange(R.T)
            assert float(var[:, t % 8 == 0].abs().max()) == 0.0 and float(var[:, t % 8 == 1].abs().max()) <= 1e-20
            assert float(st["u"][:, t % 8 == 0].abs().max()) <= 0.125
            mid = var[:, t % 8 == 2]
            assert 1e-8 < float(mid.median()) < 1e-4 and float(var[:, t % 8 == 3].median()) > 0.1
            assert bool(torch.isfinite(R.ref(inp, R.route("one_pass", dtype == torch.float16))[1]).all())      # sig - E2 > 0
        if gen == "large_mean":
            assert float((st["mu"].abs() / st["sig"]).min()) > 30
        if gen == "hyper_pair":
            a, d = inp["hyper"], inp["hyper_d"] - inp["hyper"]
            assert torch.equal(a.to(torch.float16).float(), a) and torch.equal(d.to(torch.float16).float(), d) and float(d.abs().min()) > 0
            assert torch.equal(inp["hyper_d"].to(torch.float16).float(), a)              # below half an ulp: hi = a, lo = d
            assert torch.equal((inp["hyper_d"].double() - a.double()).float(), d)        # a + d is exact in fp32
