"""up_fused_kernel (csrc/upfused.hip) on the device at every launch route and edge, called through ops.upscale_fused and - where ops has no
parameter (guard zones, fp16 output, the range map) - through msam_upscale_fused_out / _range, against the fp64 formulation of
tests/upscale_fused_ref.py computed on the device in chunks of prompts.  EVERY element of every prompt is compared.

Prompt axis (the shipped route: centred weights, default knobs, fp32 output, generator "diffuse"), from the CU count the device reports
(printed): the launcher's key split is the smallest power of two with P * KS >= 2 x CUs (at most 16) and its grid min(P * KS, 2 x CUs), so
the axis holds P = 1, 2, 3, both sides of 2 x CUs / 16 (where the grid fills up), / 8, / 4, / 2 and / 1 (where KS drops to 8, 4, 2, 1),
2 x CUs / 16 + 1 (uneven shares: one workgroup in 32 runs a second item) and max(2 x CUs + 1, 513): KS = 1, the persistent loop in which a
workgroup walks the 256 tiles of a prompt and then changes prompt, output base and hyper weights.  "wide" and "flat" run at one P for each of
KS = 16, 4 and 1.  Route axis, each at P = 3 and at 2 x CUs / 16 + 1: up_gelu16 0 / 1 with centred and plain weights, up_centred = 0,
up_ln_two_pass = 1 on "large_mean", priority 0, the blocked stream, fp16 output, hyper_ld 32 / 36 / 128, all nine (mask0, nmask).

Criteria per case: the output is finite after a NaN prefill; sentinel guard zones around the output and the range map are untouched;
|got - ref| <= bound elementwise (derivation: upscale_fused_ref's docstring); mean |got - ref| <= 1.5 x mean |restate - ref| per (prompt,
mask) plane - the margin is for what the restatement does not model: v_exp_f16 at up to one ulp instead of correct rounding (one of about
three comparable rounding contributions per GELU: its doubling moves the rms by at most sqrt(2)) and the fp32 summation order; the range
map equals amin / amax of every 64-pixel segment; and the exact invariants - per-token arithmetic does not depend on the launch geometry, so
a second call, the first P - 1 prompts alone, single-prompt launches (first, last, the first prompt of a workgroup's second item), the
blocked stream, priority 0 and a launch with the range map give the same bits, and the fp16 output is the fp16 rounding of the fp32 one.
The differential check: out(a + d) - out(a) for hyper weights a + d that differ from a only in the lo half of the kernel's fp16 pair.

tests/test_upscale_fused_ref_host.py proves on the CPU that each defect this kernel is prone to lands outside one of these criteria (or
names it as invisible), and runs the kernel source on the host shim through the same reference.

MEASURED on an MI355X (256 CUs), the shipped fp16 build, over the 87 comparisons of this file (profiles/r15_upscale_fused_err.md holds the
table; every case prints its figures, pytest -s): max |got - ref| / bound 0.016 - 0.069 with the packed-fp16 GELUs (the shipped form) and
0.023 - 0.178 with the packed-fp32 GELUs; largest plane-mean ratio 1.000 - 1.004 and 1.000 - 1.006 (the criterion: 1.5); the differential
check 0.025 - 0.031 of its bound.  The packed-fp16 mean ratio of 1.00 says that v_exp_f16 behaves like the restatement's correctly rounded
exponential; the bound assumes one ulp for it.  On the CPU emulation only (the host test): 0.002 - 0.10 of the bound, mean ratio 1.000
(1.45 for the one-pass statistics on "large_mean", which the device runs through the two-pass form only).  The bf16 ablation build is
covered by the bf16 leg of the host test only."""
import pytest
import torch

import upscale_fused_ref as R

pytestmark = pytest.mark.gpu

SENT = -12345.5
KNOBS = {"up_gelu16": 1, "up_centred": 1, "up_ln_two_pass": 0}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import _lib, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"\nthe device reports {cus} CUs: launch grids of at most {2 * cus} workgroups; library build: decoder type {_lib.decoder_dtype()}")
    return ops, _lib, torch.device("cuda"), cus


def _resolve(P, cus):
    """The prompt axis in terms of the CU count: ("below", d) = 2 cus / d - 1, ("at", d) = 2 cus / d, "uneven", "persistent"."""
    if isinstance(P, int):
        return P
    if P == "uneven":
        return 2 * cus // 16 + 1
    if P == "persistent":
        return max(2 * cus + 1, 513)
    side, d = P
    return max(1, 2 * cus // d - (1 if side == "below" else 0))


def _pid(P):
    return f"P{P}" if isinstance(P, int) else P if isinstance(P, str) else f"{P[0]}-2cus/{P[1]}"


class _Knobs:
    """Sets tuning knobs and the priority; restores every one of them on exit."""

    def __init__(self, _lib, prio=1, **knobs):
        self.lib, self.prio, self.knobs = _lib.load(), prio, knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            self.lib.msam_tune_set(k.encode(), v)
        self.lib.msam_upscale_set_prio(self.prio)

    def __exit__(self, *exc):
        for k, v in KNOBS.items():
            self.lib.msam_tune_set(k.encode(), v)
        self.lib.msam_upscale_set_prio(1)


def _via_ops(ops, inp, blocked=False):
    keys = ops.to_blocked(inp["keys"]) if blocked else inp["keys"]
    return ops.upscale_fused(keys, inp["w1"], inp["b1"], inp["ln_w"], inp["ln_b"], inp["w2"], inp["b2"], inp["hyper"], inp["mask0"], inp["nmask"],
                             ln_eps=inp["eps"], blocked=blocked, centred=inp["centred"])


def _direct(_lib, inp, out16=False, want_range=False):
    """msam_upscale_fused_range into a NaN-prefilled output between sentinel guard zones (and a range map between its own): checks the guard
    zones, returns (logits, map or None)."""
    lib, dev = _lib.load(), inp["keys"].device
    P, nmask = inp["keys"].shape[0], inp["nmask"]
    n, guard = P * nmask * 65536, 65536
    if out16:
        buf = torch.full((guard + n + guard,), float("nan"), dtype=torch.float16, device=dev)
        buf[:guard] = SENT
        buf[-guard:] = SENT
    else:
        buf = torch.full((guard + n + guard,), float("nan"), dtype=torch.float32, device=dev)
        buf[:guard] = SENT
        buf[-guard:] = SENT
    rbuf = torch.full((1024 + n // 32 + 1024,), SENT, dtype=torch.float32, device=dev)
    out, rng = buf[guard:guard + n], rbuf[1024:1024 + n // 32]
    _lib.check(lib.msam_upscale_fused_range(inp["keys"].data_ptr(), 2 if inp["centred"] else 0, P, inp["w1"].data_ptr(), inp["b1"].data_ptr(),
                                            inp["ln_w"].data_ptr(), inp["ln_b"].data_ptr(), inp["eps"], inp["w2"].data_ptr(), inp["b2"].data_ptr(),
                                            inp["hyper"].data_ptr(), inp["hyper"].shape[-1], inp["mask0"], nmask, out.data_ptr(),
                                            _lib.F16 if out16 else _lib.F32, rng.data_ptr() if want_range else None, _lib.stream_ptr()),
               "msam_upscale_fused_range")
    torch.cuda.synchronize()
    sent = torch.tensor(SENT, dtype=buf.dtype, device=dev)
    assert bool((buf[:guard] == sent).all()) and bool((buf[-guard:] == sent).all()), "a store outside the output"
    assert bool((rbuf[:1024] == SENT).all()) and bool((rbuf[-1024:] == SENT).all()), "a store outside the range map"
    if not want_range:
        assert bool((rng == SENT).all()), "a launch without a range map wrote one"
    return out.reshape(P, nmask, 256, 256), (rng.reshape(P, nmask, 256, 4, 2) if want_range else None)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                                                                     b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


def _within(what, got, inp, rt, chunk=8, check=True):
    """|got - ref| <= bound elementwise and the mean criterion per (prompt, mask) plane, in one pass over the reference, chunk by chunk of
    prompts; prints the largest ratios and names the worst element.  ``check=False`` only measures: (max ratio, largest mean ratio)."""
    assert bool(torch.isfinite(got).all()), f"{what}: pixels never stored (the NaN prefill) or a non-finite result"
    worst, where, nbad, mean_worst, mean_where = -1.0, None, 0, -1.0, None
    for lo, hi, ref, bound in R.ref_chunks(inp, rt, chunk):
        diff = got[lo:hi].double() - ref
        err = diff.abs()
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.inf, 0.0))
        nbad += int((err > bound).sum())
        i = int(ratio.argmax())
        if float(ratio.reshape(-1)[i]) > worst:
            worst = float(ratio.reshape(-1)[i])
            p, m, y, x = (int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
            where = (lo + p, m, y, x, float(err[p, m, y, x]), float(bound[p, m, y, x]))
        base = R.plane_means(R.restate(R.first_prompts(inp, slice(lo, hi)), rt, chunk=hi - lo) - ref)
        means = R.plane_means(diff) / base
        j = int(means.argmax())
        if float(means.reshape(-1)[j]) > mean_worst:
            mean_worst, mean_where = float(means.reshape(-1)[j]), (lo + j // means.shape[1], j % means.shape[1])
    print(f"\n{what}: max |got - ref| / bound = {worst:.3f}; largest mean |got - ref| / mean |restate - ref| of a plane = {mean_worst:.3f}")
    if not check:
        return worst, mean_worst
    assert nbad == 0, (f"{what}: {nbad} elements outside the bound; worst |got - ref| / bound = {worst:.3g} at prompt {where[0]} mask {where[1]} "
                       f"pixel ({where[2]}, {where[3]}): err {where[4]:.3g}, bound {where[5]:.3g}")
    assert mean_worst <= R.MEAN_MARGIN, f"{what}: plane (prompt {mean_where[0]}, mask {mean_where[1]}) has {mean_worst:.3f} x the restatement's mean error"
    return worst, mean_worst


def _range_is_exact(out, rng):
    seg = out.reshape(*out.shape[:2], 256, 4, 64)
    assert torch.equal(rng, torch.stack([seg.amin(-1), seg.amax(-1)], -1)), "the range map is not {amin, amax} of every 64-pixel segment"


def _geometry_invariants(ops, inp, got, cus):
    """The same bits for the first P - 1 prompts alone and for single-prompt launches, whatever their key splits."""
    P = inp["keys"].shape[0]
    ks, grid = R.key_splits(P, cus)
    if P > 1:
        assert _same_bits(_via_ops(ops, R.first_prompts(inp, slice(0, P - 1))), got[:P - 1]), "the first P - 1 prompts alone differ"
    singles = {0, P - 1}
    if P * ks > grid:
        singles.add(grid // ks)                                                            # the prompt of work item `grid`: workgroup 0's second item
    for p in sorted(singles):
        assert _same_bits(_via_ops(ops, R.first_prompts(inp, slice(p, p + 1))), got[p:p + 1]), f"prompt {p} alone differs"


# ---------------------------------------------------------------------------------------------------------------------- prompt axis
PROMPT_AXIS = [1, 2, 3, ("below", 16), ("at", 16), "uneven", ("below", 8), ("at", 8), ("below", 4), ("at", 4), ("below", 2), ("at", 2),
               ("below", 1), ("at", 1), "persistent"]


@pytest.mark.parametrize("P", PROMPT_AXIS, ids=_pid)
def test_shipped_route_at_every_key_split(env, P):
    ops, _lib, dev, cus = env
    P = _resolve(P, cus)
    d16 = _lib.decoder_dtype()
    ks, grid = R.key_splits(P, cus)
    inp = R.make("diffuse", d16, P, dev, centred=True, seed=5)
    rt = R.route("cen", d16 == torch.float16)
    got = _via_ops(ops, inp)
    assert got.shape == (P, 3, 256, 256) and got.dtype == torch.float32
    assert _same_bits(_via_ops(ops, inp), got), "a second call differs"
    out, rng = _direct(_lib, inp, want_range=True)
    assert _same_bits(out, got), "the launch with the range map changed the logits"
    _range_is_exact(out, rng)
    plain, _ = _direct(_lib, inp)
    assert _same_bits(plain, got)
    _geometry_invariants(ops, inp, got, cus)
    _within(f"shipped route, diffuse P={P} KS={ks} items={P * ks} grid={grid} ({cus} CUs)", out, inp, rt)


@pytest.mark.parametrize("P", [3, ("at", 4), ("at", 1)], ids=_pid)
@pytest.mark.parametrize("gen", ["wide", "flat"])
def test_shipped_route_on_wide_and_flat_arguments(env, gen, P):
    ops, _lib, dev, cus = env
    P = _resolve(P, cus)
    d16 = _lib.decoder_dtype()
    ks, grid = R.key_splits(P, cus)
    inp = R.make(gen, d16, P, dev, centred=True, seed=6)
    out, rng = _direct(_lib, inp, want_range=True)
    assert _same_bits(_via_ops(ops, inp), out)
    _range_is_exact(out, rng)
    _within(f"shipped route, {gen} P={P} KS={ks} grid={grid}", out, inp, R.route("cen", d16 == torch.float16))


# ---------------------------------------------------------------------------------------------------------------------- route axis
ROUTE_P = [3, "uneven"]
# (name, generator, centred weights, knobs, priority)
ROUTES = [
    ("gelu16-centred", "wide", True, {"up_gelu16": 1}, 1),
    ("gelu32-centred", "wide", True, {"up_gelu16": 0}, 1),
    ("gelu16-plain", "diffuse", False, {"up_gelu16": 1}, 1),
    ("gelu32-plain", "flat", False, {"up_gelu16": 0}, 1),
    ("gelu16-up_centred0", "diffuse", True, {"up_gelu16": 1, "up_centred": 0}, 1),
    ("gelu32-up_centred0", "flat", True, {"up_gelu16": 0, "up_centred": 0}, 1),
    ("gelu16-two_pass", "large_mean", False, {"up_gelu16": 1, "up_ln_two_pass": 1}, 1),
    ("gelu32-two_pass", "large_mean", False, {"up_gelu16": 0, "up_ln_two_pass": 1}, 1),
    ("gelu16-prio0", "diffuse", False, {"up_gelu16": 1}, 0),
    ("gelu32-prio0", "wide", False, {"up_gelu16": 0}, 0),
]


def _route_of(centred, knobs, prio, d16, out16=False):
    g16 = bool(knobs.get("up_gelu16", 1)) and d16 == torch.float16
    if knobs.get("up_ln_two_pass", 0):
        return R.route("two_pass", g16, out16)
    return R.route("cen" if centred and knobs.get("up_centred", 1) and prio else "one_pass", g16, out16)


@pytest.mark.parametrize("P", ROUTE_P, ids=_pid)
@pytest.mark.parametrize("name,gen,centred,knobs,prio", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_instantiation_the_launcher_reaches(env, name, gen, centred, knobs, prio, P):
    """Each knob route on the row-major and the blocked stream, with fp32 and fp16 output, and (where the launcher builds one) the range map."""
    ops, _lib, dev, cus = env
    d16 = _lib.decoder_dtype()
    if knobs.get("up_gelu16", 1) and d16 != torch.float16:
        pytest.skip("the packed-fp16 GELUs exist in the fp16 decoder build only")
    P = _resolve(P, cus)
    ks, grid = R.key_splits(P, cus)
    inp = R.make(gen, d16, P, dev, centred=centred, seed=7)
    has_map = prio == 1 and not knobs.get("up_ln_two_pass", 0)
    with _Knobs(_lib, prio, **knobs):
        got, _ = _direct(_lib, inp)
        assert _same_bits(_via_ops(ops, inp), got), "a second call (through ops) differs"
        assert _same_bits(_via_ops(ops, inp, blocked=True), got), "the blocked stream differs from the row-major one"
        got16, _ = _direct(_lib, inp, out16=True)
        assert bool(torch.isfinite(got16).all()) and _same_bits(got16, got.to(torch.float16)), "the fp16 output is not the rounding of the fp32 output"
        if has_map:
            out, rng = _direct(_lib, inp, want_range=True)
            assert _same_bits(out, got), "the launch with the range map changed the logits"
            _range_is_exact(out, rng)
        if prio == 0:                                    # priority 0 against priority 1: the same kernel body
            _lib.load().msam_upscale_set_prio(1)
            assert _same_bits(_via_ops(ops, inp), got), "priority 0 differs from priority 1"
        _geometry_invariants(ops, inp, got, cus)
    what = f"{name}, {gen} P={P} KS={ks} grid={grid}"
    _within(what, got, inp, _route_of(centred, knobs, prio, d16))
    _within(what + ", fp16 output", got16, inp, _route_of(centred, knobs, prio, d16, out16=True))


def test_the_criteria_reject_a_wrong_result(env):
    """The control - a comparison that passed these would be vacuous.  (a) The last tile of the last prompt not stored: 4 rows of 64 pixels left at
    zero in an otherwise correct output.  (b) msam_tune_set("up_gelu16", 2) launches the timing experiment whose GELUs have no exponential (wrong
    by design, and for that reason not on the route axis): its output is non-finite or far outside both criteria."""
    ops, _lib, dev, cus = env
    d16 = _lib.decoder_dtype()
    inp = R.make("diffuse", d16, 3, dev, centred=True, seed=5)
    rt = R.route("cen", d16 == torch.float16)
    got = _via_ops(ops, inp)
    holed = got.clone()
    holed[2, :, 252:256, 192:256] = 0.0
    worst, _ = _within("the last tile of prompt 2 not stored", holed, inp, rt, check=False)
    assert worst > 4.0, worst
    if d16 != torch.float16:
        return
    with _Knobs(_lib, 1, up_gelu16=2):
        wrong = _via_ops(ops, inp)
    if bool(torch.isfinite(wrong).all()):
        worst, mean_worst = _within("up_gelu16 = 2 (no exponential)", wrong, inp, R.route("one_pass", True), check=False)
        assert worst > 4.0 and mean_worst > 4 * R.MEAN_MARGIN, (worst, mean_worst)
    else:
        print("\nup_gelu16 = 2 (no exponential): a non-finite output")
    assert _same_bits(_via_ops(ops, inp), got)                                             # (the knob is back)


MASKS = [(m0, nm) for nm in (1, 2, 3) for m0 in range(0, 5 - nm)]
LD_MASKS = [(128, m0, nm) for m0, nm in MASKS] + [(32, 1, 3), (36, 1, 3), (36, 0, 1)]


@pytest.mark.parametrize("P", ROUTE_P, ids=_pid)
@pytest.mark.parametrize("ld,mask0,nmask", LD_MASKS, ids=[f"ld{c[0]}-mask{c[1]}+{c[2]}" for c in LD_MASKS])
def test_every_mask_slice_and_hyper_stride(env, ld, mask0, nmask, P):
    """All nine legal (mask0, nmask) and hyper_ld 32 / 36 / 128 on the shipped route: the lanes of a mask >= nmask are dropped by the output
    descriptor's range, so the guard zones behind a 1- or 2-mask output are what an unwanted store would hit."""
    ops, _lib, dev, cus = env
    assert len(MASKS) == 9
    P = _resolve(P, cus)
    d16 = _lib.decoder_dtype()
    inp = R.make("diffuse", d16, P, dev, centred=True, hyper_ld=ld, mask0=mask0, nmask=nmask, seed=8)
    out, rng = _direct(_lib, inp, want_range=True)
    assert _same_bits(_via_ops(ops, inp), out)
    _range_is_exact(out, rng)
    full = R.make("diffuse", d16, P, dev, centred=True, hyper_ld=128, mask0=0, nmask=3, seed=8)
    if ld == 128 and (mask0, nmask) != (0, 3) and mask0 + nmask <= 3:                      # a slice of the 3-mask launch, bit for bit
        assert _same_bits(_via_ops(ops, full)[:, mask0:mask0 + nmask].contiguous(), out)
    _within(f"hyper_ld={ld} masks [{mask0}, {mask0 + nmask}) P={P}", out, inp, R.route("cen", d16 == torch.float16))


@pytest.mark.parametrize("P", ROUTE_P, ids=_pid)
def test_the_lo_half_of_the_hyper_pair_reaches_the_output(env, P):
    """hyper = a and a + d, d below half an fp16 ulp of a: the hi halves are equal, so out(a + d) - out(a) is what the lo half carries."""
    ops, _lib, dev, cus = env
    P = _resolve(P, cus)
    d16 = _lib.decoder_dtype()
    inp = R.make("hyper_pair", d16, P, dev, centred=True, seed=9)
    rt = R.route("cen", d16 == torch.float16)
    out_a = _via_ops(ops, inp)
    out_d = _via_ops(ops, dict(inp, hyper=inp["hyper_d"]))
    worst = 0.0
    for lo, hi, want, bound in R.diff_bound_chunks(inp, inp["hyper_d"], rt):
        err = ((out_d[lo:hi].double() - out_a[lo:hi].double()) - want).abs()
        worst = max(worst, float((err / bound).max()))
    print(f"\ndifferential check P={P}: max |(out(a + d) - out(a)) - d.G2| / bound = {worst:.3f}")
    assert worst <= 1.0, worst
    _within(f"hyper_pair P={P}", out_a, inp, rt)
