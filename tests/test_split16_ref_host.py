"""tests/split16_ref.py on the CPU, no GPU: (1) the host build of csrc/strict.hip (tests/hip_host_shim.py: the emulated MFMA lane
layouts, transposing LDS read and v_exp_f32) stays within the module's elementwise bounds on a small subset of every family - a check
of the DERIVATION, not of the hardware, which tests/test_gpu_split16_kernels.py repeats on the device over every route; (2) every named
mutation of the references lies at least 4 bounds from the unmutated reference at some element of some generator - the condition that
keeps the bounds from being slack: a kernel with that defect fails the device test; (3) the generators stay inside the documented
domain (they assert it when they build their operands).  The mutation tables are printed (pytest -s)."""
import os

import pytest
import torch

import split16_calls as K
import split16_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 4.0


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from micro_sam_amd import _lib
    lib = build_library(str(tmp_path_factory.mktemp("host_split16")), ROOT)
    for name, (res, args) in _lib._PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    os.environ["MSAM_EMU_CUS"] = "4"
    try:
        yield lib, _lib
    finally:
        os.environ.pop("MSAM_EMU_CUS", None)


def _far(ref, bound, mutated):
    return float(((mutated - ref).abs() / bound).max())


# ------------------------------------------------------------------------------------------------------------------ the mutations
def test_every_product_mutation_is_far_outside_the_bound():
    print()
    for mutation in R.PRODUCT_MUTATIONS:
        name, M, N, Kk, opt = R.PRODUCT_MUTATION_CASE[mutation]
        inp = R.make_product(name, M, N, Kk, seed=1, **opt)
        ref, bound = R.product_ref(inp)
        far = _far(ref, bound, R.product_ref(inp, mutation)[0])
        print(f"product {mutation:22s} on {R.product_case_id((name, M, N, Kk, opt)):60s}: {far:10.3g} bounds")
        assert far >= FAR, (mutation, far)


@pytest.fixture(scope="module")
def t2i_sets():
    sets = {}
    for gen in R.T2I_GENERATORS:
        inp = R.make_t2i(gen, 2, 7, seed=1)
        sets[gen] = (inp,) + R.t2i_ref(inp)
    return sets


def test_every_t2i_mutation_is_far_outside_the_bound(t2i_sets):
    print()
    for mutation in R.T2I_MUTATIONS:
        far = {gen: _far(ref, bound, R.t2i_ref(inp, mutation)[0]) for gen, (inp, ref, bound) in t2i_sets.items()}
        best = max(far, key=far.get)
        print(f"t2i {mutation:18s}: " + " ".join(f"{g} {v:9.3g}" for g, v in far.items()))
        assert far[best] >= FAR, (mutation, far)


@pytest.fixture(scope="module")
def i2t_sets():
    sets = {}
    for gen in R.I2T_GENERATORS:
        inp = R.make_i2t(gen, 2, 5, gen in ("distinct", "flat"), seed=1)
        ref, bounds = zip(*[(p[2], p[3]) for p in R.i2t_ref_chunks(inp)])
        sets[gen] = (inp, torch.cat(ref), [torch.cat([b[i] for b in bounds]) for i in range(2)])
    return sets


def test_every_i2t_mutation_is_far_outside_both_bounds(i2t_sets):
    print()
    for mutation in R.I2T_MUTATIONS:
        far = {}
        for gen, (inp, ref, bounds) in i2t_sets.items():
            mut = R.i2t_ref(inp, mutation=mutation)[0]
            far[gen] = min(_far(ref, b, mut) for b in bounds)                             # the wider of the two forms' bounds decides
        print(f"i2t {mutation:22s}: " + " ".join(f"{g} {v:9.3g}" for g, v in far.items()))
        assert max(far.values()) >= FAR, (mutation, far)


def test_every_up2_mutation_is_far_outside_the_bound():
    print()
    sets = [R.make_up2(gen, 1, m0, nm, ld, seed=1) for gen, (m0, nm, ld) in zip(R.UP2_GENERATORS, ((1, 3, 40), (3, 1, 40)))]
    refs = [R.up2_ref(inp) for inp in sets]
    for mutation in R.UP2_MUTATIONS:
        far = [_far(ref, bound, R.up2_ref(inp, mutation)[0]) for inp, (ref, bound) in zip(sets, refs)]
        print(f"up2 {mutation:22s}: " + " ".join(f"{g} {v:9.3g}" for g, v in zip(R.UP2_GENERATORS, far)))
        assert max(far) >= FAR, (mutation, far)


def test_every_relpos_mutation_is_far_outside_the_bound():
    print()
    sets = {gen: R.make_relpos(gen, 2, 2, 64, 20, 14, seed=1) for gen in R.RELPOS_GENERATORS}
    refs = {gen: R.relpos_ref(inp) for gen, inp in sets.items()}
    for mutation in R.RELPOS_MUTATIONS:
        far = {gen: _far(*refs[gen], R.relpos_ref(inp, mutation)[0]) for gen, inp in sets.items()}
        print(f"relpos {mutation:22s}: " + " ".join(f"{g} {v:9.3g}" for g, v in far.items()))
        assert max(far.values()) >= FAR, (mutation, far)


def test_generators_refuse_operands_outside_the_domain():
    """The domain assertions fire: a stream beyond 2^15, scores beyond 30 / log2 e, a weight scale that overflows fp16."""
    inp = R.make_t2i("diffuse", 1, 2, seed=2)
    R.check_t2i_domain(inp)
    with pytest.raises(AssertionError):
        R.check_t2i_domain(dict(inp, keys=inp["keys"] * 2.0 ** 14))
    with pytest.raises(AssertionError):
        R.check_t2i_domain(dict(inp, q=inp["q"] * 8))
    inp = R.make_i2t("diffuse", 1, 2, False, seed=2)
    with pytest.raises(AssertionError):
        R.check_i2t_domain(dict(inp, tok_k=inp["tok_k"] * 8))
    with pytest.raises(AssertionError):
        R.check_i2t_domain(dict(inp, tok_v=inp["tok_v"] * 4096))
    inp = R.make_relpos("diffuse", 1, 1, 64, 14, 14, seed=2)
    R.relpos_ref(inp)
    with pytest.raises(AssertionError):
        R.relpos_ref(dict(inp, qkv=inp["qkv"] * 4))
    inp = R.make_product("diffuse", 8, 8, 8, seed=2)
    with pytest.raises(AssertionError):
        R.check_product_domain(dict(inp, w_scale=inp["w_scale"] * 16))
    with pytest.raises(AssertionError):
        R.check_product_domain(dict(inp, a=inp["a"] * 1e5))


def test_pairs_ref_is_the_documented_layout():
    w = torch.arange(2 * 64, dtype=torch.float32).reshape(2, 64) + 0.0001
    out = R.pairs_ref(w, 1.0, False)
    assert torch.equal(out[1, 64:96], w[1, 32:].half()) and torch.equal(out[0, 32:64], (w[0, :32] - w[0, :32].half().float()).half())
    perm = R.pairs_ref(w, 1.0, True)
    assert torch.equal(perm[0, 8:12], w[0, 4:8].half()) and torch.equal(perm[0, 4:8], w[0, 8:12].half()) and \
        torch.equal(perm[0, 16:20], w[0, 16:20].half())


# --------------------------------------------------------------------------------------------------------------- the host build
HOST_PRODUCT = [R.PRODUCT_CASES[i] for i in (0, 3, 5, 9, 11, 13, 15, 16, 18)]


@pytest.mark.parametrize("case", HOST_PRODUCT, ids=R.product_case_id)
def test_host_product_within_the_bound(host, case):
    lib, L = host
    name, M, N, Kk, opt = case
    inp = R.make_product(name, M, N, Kk, seed=3, **opt)
    outs = {}
    for split in (True, False):
        ref, bound = R.product_ref(inp, split=split)
        for route, knobs in K.ROUTES.items():
            with K.tuned(lib, **knobs):
                outs[split, route] = got = K.gemm(lib, L, inp, split=split)
            r = K.ratio(got, ref, bound)
            print(f"\nhost product {R.product_case_id(case)} split16={int(split)} {route}: max |got - ref| / bound = {r:.3f}")
            assert r <= 1.0
        assert torch.equal(outs[split, "tile64"], outs[split, "tile128_nbuf1"]) and \
            torch.equal(outs[split, "tile64"], outs[split, "tile128_nbuf2"])


@pytest.mark.parametrize("N,Kk,permute", [(5, 32, 0), (128, 256, 1), (3, 128, 1)])
def test_host_prepared_pairs_are_bit_exact(host, N, Kk, permute):
    lib, L = host
    w = R.make_product("diffuse", 1, N, Kk, seed=4, w_range=20)["w"]
    got, guard = K.prepare_pairs(lib, w, R.weight_scale(w), permute)
    assert torch.equal(got.view(torch.int16), R.pairs_ref(w, R.weight_scale(w), permute).view(torch.int16))
    assert K.guard_untouched(guard)


@pytest.mark.parametrize("gen,Tk", [("diffuse", 7), ("needle", 8), ("plateau", 3), ("rising", 1), ("duel", 2)])
def test_host_t2i_within_the_bound(host, gen, Tk):
    lib, L = host
    inp = R.make_t2i(gen, 1, Tk, seed=3)
    got, guard = K.t2i(lib, L, inp, ldq=132, ldo=136)
    ref, bound = R.t2i_ref(inp)
    r = K.ratio(got, ref, bound)
    print(f"\nhost t2i {gen} Tk={Tk}: max |got - ref| / bound = {r:.3f}")
    assert r <= 1.0 and K.guard_untouched(guard)


@pytest.mark.parametrize("gen,Tk,shared", [("diffuse", 7, False), ("flat", 1, True), ("magnitudes", 8, False), ("duel", 2, True)])
def test_host_i2t_within_the_bounds(host, gen, Tk, shared):
    lib, L = host
    inp = R.make_i2t(gen, 1, Tk, shared, seed=3)
    folded, guard = K.i2t_folded(lib, L, inp)
    unfolded = K.i2t_unfolded(lib, L, inp)
    pairs = (K.prepare_pairs(lib, inp["wq"], inp["wq_scale"], 0)[0], K.prepare_pairs(lib, inp["wo"], inp["wo_scale"], 1)[0])
    assert torch.equal(K.i2t_unfolded(lib, L, inp, pairs=pairs), unfolded)
    for lo, hi, ref, bounds in R.i2t_ref_chunks(inp):
        for what, got, bound in (("folded", folded, bounds[0]), ("unfolded", unfolded, bounds[1])):
            r = K.ratio(got[lo:hi], ref, bound)
            print(f"\nhost i2t {what} {gen} Tk={Tk} {'shared' if shared else 'own'}: max |got - ref| / bound = {r:.3f}")
            assert r <= 1.0
    assert K.guard_untouched(guard)
    if not shared:
        own = dict(inp, keys=inp["keys"].clone())
        assert torch.equal(K.i2t_folded(lib, L, own, in_place=True)[0], folded)


@pytest.mark.parametrize("gen,mask0,nmask,ld", [("diffuse", 1, 3, 40), ("magnitudes", 0, 1, 32)])
def test_host_up2_within_the_bound(host, gen, mask0, nmask, ld):
    lib, L = host
    inp = R.make_up2(gen, 1, mask0, nmask, ld, seed=3)
    got, guard = K.up2(lib, L, inp)
    ref, bound = R.up2_ref(inp)
    r = K.ratio(got, ref, bound)
    print(f"\nhost up2 {gen} mask0={mask0} nmask={nmask} hyper_ld={ld}: max |got - ref| / bound = {r:.3f}")
    assert r <= 1.0 and K.guard_untouched(guard)


@pytest.mark.parametrize("gen,B,heads,hd,G,window", [("diffuse", 2, 2, 64, 20, 14), ("needle", 1, 1, 80, 20, 14), ("distinct", 1, 2, 64, 14, 14)])
def test_host_relpos_within_the_bound(host, gen, B, heads, hd, G, window):
    lib, L = host
    inp = R.make_relpos(gen, B, heads, hd, G, window, seed=3)
    got, guard = K.relpos(lib, inp)
    ref, bound = R.relpos_ref(inp)
    r = K.ratio(got, ref, bound)
    print(f"\nhost relpos {gen} B={B} heads={heads} hd={hd} grid={G} window={window}: max |got - ref| / bound = {r:.3f}")
    assert r <= 1.0 and K.guard_untouched(guard)
