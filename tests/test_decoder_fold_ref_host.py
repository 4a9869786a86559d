"""The proof behind tests/test_gpu_decoder_fold.py, on the CPU.

1. Every defect of decoder_fold_ref.T2I_MUTATIONS / I2T_MUTATIONS, written as a variant of the fp64 reference, is at least 4 of the
   module's elementwise bounds from the reference on the generator meant for it, for both 16-bit types.  A kernel within one bound of
   the truth is then at least 3 bounds from the mutant, so a kernel WITH that defect fails the device test on these inputs.  This is a
   condition on the generators, not a measurement of a kernel.
2. The bound is not too tight for an honest kernel: the folded arithmetic restated in fp64 with 16-bit roundings at exactly the
   kernels' rounding points lies within ONE bound of the reference on every generator.
3. The kernel source compiled for the host (tests/host_product.py; the fp16 build) stays within the bound at the smallest cases.

Every test prints its figure (pytest -s); profiles/r10_decoder_fold_err_over_bound.md records them."""
import functools

import pytest
import torch

import decoder_fold_ref as R
from host_product import product_on_host

DTYPES = [torch.bfloat16, torch.float16]
DIDS = ["bf16", "fp16"]

# mutation -> (generator, P, Nt, shared); P = 3 -> 16 key splits
T2I_CASES = {
    "drop_last_tile": ("needle", 3, 7, False),
    "drop_split": ("needle", 3, 7, False),
    "merge_no_rescale": ("split_skew", 3, 7, False),
    "no_tabk": ("needle", 3, 7, False),
    "no_bv": ("diffuse", 3, 7, False),
    "swap_heads": ("distinct", 3, 7, False),
    "prompt_from_next": ("distinct", 3, 7, False),
    "swap_v_rows": ("needle", 3, 7, False),
}
I2T_CASES = {
    "pad_unmasked": ("short", 2, 5, False),
    "no_bo": ("diffuse", 2, 7, False),
    "bo_over_nt": ("short", 2, 5, False),
    "no_residual": ("diffuse", 2, 7, False),
    "no_tabq": ("table", 2, 7, False),
    "swap_heads": ("distinct", 2, 7, False),
    "neighbour_tokens": ("distinct", 2, 7, False),
    "shared_reads_own_stream": ("distinct", 2, 7, True),
    "last_tile_unchanged": ("diffuse", 2, 7, False),
}


def _ratio(err, bound):
    return float((err / bound).max())


@functools.lru_cache(maxsize=None)
def _t2i_truth(gen, P, Nt, shared, dtype):
    inp = R.make_t2i(gen, dtype, P, Nt, shared, seed=0)
    return inp, R.t2i_ref(inp)


@functools.lru_cache(maxsize=None)
def _i2t_truth(gen, P, Nt, shared, dtype, variant):
    inp = R.make_i2t(gen, dtype, P, Nt, shared, seed=0)
    return inp, R.i2t_ref(inp, variant)


def test_every_mutation_has_a_case():
    assert set(T2I_CASES) == set(R.T2I_MUTATIONS) and set(I2T_CASES) == set(R.I2T_MUTATIONS)


def test_key_splits_thresholds():
    """Both sides of every threshold of the kernels' key_splits (63 | 64, 127 | 128, 255 | 256, 511 | 512)."""
    assert [R.key_splits(P) for P in (1, 63, 64, 127, 128, 255, 256, 511, 512, 513)] == [16, 16, 8, 8, 4, 4, 2, 2, 1, 1]


# ------------------------------------------------------------------------------------------------------------- 1. mutations
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("mutation", R.T2I_MUTATIONS)
def test_t2i_mutation_is_four_bounds_from_the_reference(mutation, dtype):
    gen, P, Nt, shared = T2I_CASES[mutation]
    inp, (ref, bound) = _t2i_truth(gen, P, Nt, shared, dtype)
    mut, _ = R.t2i_ref(inp, mutation)
    ratio = _ratio((mut - ref).abs(), bound)
    print(f"\nt2i {mutation} / {gen} / {DIDS[DTYPES.index(dtype)]}: max |mutant - ref| / bound = {ratio:.1f}")
    assert ratio >= 4.0, ratio


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("mutation", R.I2T_MUTATIONS)
def test_i2t_mutation_is_four_bounds_from_the_reference(mutation, dtype, variant):
    gen, P, Nt, shared = I2T_CASES[mutation]
    inp, (ref, bound) = _i2t_truth(gen, P, Nt, shared, dtype, variant)
    mut, _ = R.i2t_ref(inp, variant, mutation)
    ratio = _ratio((mut - ref).abs(), bound)
    print(f"\ni2t variant {variant} {mutation} / {gen} / {DIDS[DTYPES.index(dtype)]}: max |mutant - ref| / bound = {ratio:.1f}")
    assert ratio >= 4.0, ratio


# ------------------------------------------------------------------------------------------- 2. the bound is honest from below
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("gen", R.T2I_GENERATORS)
def test_t2i_rounded_restatement_is_within_one_bound(gen, dtype):
    inp, (ref, bound) = _t2i_truth(gen, 3, 7, False, dtype)
    ratio = _ratio((R.restate_t2i(inp) - ref).abs(), bound)
    print(f"\nt2i restatement / {gen} / {DIDS[DTYPES.index(dtype)]}: max |restated - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("gen", R.I2T_GENERATORS)
def test_i2t_rounded_restatement_is_within_one_bound(gen, dtype, variant):
    Nt = 5 if gen == "short" else 7
    inp, (ref, bound) = _i2t_truth(gen, 2, Nt, False, dtype, variant)
    ratio = _ratio((R.restate_i2t(inp, variant) - ref).abs(), bound)
    print(f"\ni2t variant {variant} restatement / {gen} / {DIDS[DTYPES.index(dtype)]}: max |restated - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------- what the generators promise
def test_needle_puts_its_weight_on_one_key_of_the_promised_tiles():
    """>= 0.9999 of every row's weight on ONE key; the keys cover every tile of needle_tiles(KS); key 4095 is among them; the reference
    output is V of that key to 2e-4 max |V|."""
    P, Nt = 3, 7
    inp, (ref, _) = _t2i_truth("needle", P, Nt, False, torch.float16)
    ks = R.key_splits(P)
    X, q = inp["keys"].double(), R._heads(inp["qtok"].double())
    K = R._heads(X @ inp["wk"].double().t() + inp["tabk"].double())                       # [P, T, 8, 16]
    V = R._heads(X @ inp["wv"].double().t() + inp["bv"].double())
    w = torch.softmax(torch.einsum("pthd,pjhd->pthj", q, K) / 4.0, dim=-1)
    top, arg = w.max(dim=-1)
    assert float(top.min()) >= 0.9999
    want = torch.tensor([[[R.needle_key(R.needle_code(p, t, h, Nt), h, ks) for h in range(8)] for t in range(Nt)] for p in range(P)])
    assert torch.equal(arg, want)
    assert {int(k) // 32 * 32 for k in arg.reshape(-1)} == set(R.needle_tiles(ks)) and int(arg[0, 0, 0]) == R.T - 1
    got = torch.stack([V[p, arg[p], torch.arange(8)] for p in range(P)])                  # [P, Nt, 8, 16]
    assert float((R._heads(ref) - got).abs().max()) <= 2e-4 * float(V.abs().max())


def test_split_skew_maxima_differ_by_tens_between_key_splits():
    inp, _ = _t2i_truth("split_skew", 3, 7, False, torch.float16)
    X, q = inp["keys"].double(), R._heads(inp["qtok"].double())
    K = R._heads(X @ inp["wk"].double().t() + inp["tabk"].double())
    s = torch.einsum("pthd,pjhd->pthj", q, K) / 4.0
    for ks in (2, 4, 8, 16):
        m = s.reshape(*s.shape[:-1], ks, R.T // ks).amax(dim=-1)
        spread = m.amax(dim=-1) - m.amin(dim=-1)
        assert float(spread.min()) >= 10.0, (ks, float(spread.min()))
        first = m.argmax(dim=-1)                                                          # ascending rows and descending rows
        assert bool((first == 0).any()) and bool((first == ks - 1).any())


def test_scores_stay_below_60_and_the_prenorm_row_has_sigma_of_order_1():
    for gen in R.T2I_GENERATORS:
        inp = R.make_t2i(gen, torch.bfloat16, 3, 7, False, seed=0)
        K = R._heads(inp["keys"].double() @ inp["wk"].double().t() + inp["tabk"].double())
        s = torch.einsum("pthd,pjhd->pthj", R._heads(inp["qtok"].double()), K) / 4.0
        assert float(s.abs().max()) < 60.0, (gen, float(s.abs().max()))
    for gen in R.I2T_GENERATORS:
        inp = R.make_i2t(gen, torch.bfloat16, 2, 5, False, seed=0)
        q = R._heads(inp["x"].double() @ inp["wq"].double().t() + inp["tabq"].double())
        s = torch.einsum("pjhd,pthd->pjht", q, R._heads(inp["ktok"].double())) / 4.0
        assert float(s.abs().max()) < 60.0, (gen, float(s.abs().max()))
        a = torch.softmax(s, dim=-1)
        U = torch.einsum("chd,pthd->phtc", inp["wo"].double().reshape(256, 8, 16), R._heads(inp["vtok"].double()))
        r = a.reshape(2, R.T, -1) @ U.reshape(2, -1, 256) + inp["x"].double() + inp["bo"].double()
        sig = r.std(dim=-1)
        assert 0.5 < float(sig.min()) and float(sig.max()) < 4.0, (gen, float(sig.min()), float(sig.max()))


# ------------------------------------------------------------------------------------- 3. the host-compiled product
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    with product_on_host(str(tmp_path_factory.mktemp("host_decoder_fold"))):
        from micro_sam_amd import _lib, ops
        yield ops, _lib


def _within(what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = err / bound
    i = int(ratio.argmax())
    print(f"\n{what}: max |got - ref| / bound = {float(ratio.reshape(-1)[i]):.3f}")
    bad = err > bound
    if bool(bad.any()):
        idx = [int(x) for x in torch.unravel_index(torch.tensor(i), err.shape)]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst |got - ref| / bound = "
                    f"{float(ratio.reshape(-1)[i]):.3g} at (prompt, row, channel) {idx}: err {float(err.reshape(-1)[i]):.3g}, "
                    f"bound {float(bound.reshape(-1)[i]):.3g}")


HOST_T2I = [("diffuse", 1, 3), ("diffuse", 1, 8), ("diffuse", 3, 3), ("diffuse", 3, 8), ("needle", 3, 3), ("split_skew", 3, 8),
            ("distinct", 3, 3)]
HOST_I2T = [("diffuse", 1, 3), ("diffuse", 1, 8), ("diffuse", 3, 3), ("diffuse", 3, 8), ("short", 3, 3), ("distinct", 3, 8)]


@pytest.mark.parametrize("gen,P,Nt", HOST_T2I)
def test_host_compiled_t2i_fold_attention_is_within_the_bound(host, gen, P, Nt):
    ops, _lib = host
    inp = R.make_t2i(gen, _lib.decoder_dtype(), P, Nt, False, seed=3)
    got = ops.t2i_fold_attention(inp["keys"], inp["qtok"], inp["wk"], inp["tabk"], inp["wv"], inp["bv"])
    ref, bound = R.t2i_ref(inp)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    _within(f"host t2i {gen} P={P} Nt={Nt}", got, ref, bound)


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("gen,P,Nt", HOST_I2T)
def test_host_compiled_i2t_fold_layer_is_within_the_bound(host, gen, P, Nt, variant):
    ops, _lib = host
    inp = R.make_i2t(gen, _lib.decoder_dtype(), P, Nt, False, seed=3)
    _lib.load().msam_tune_set(b"i2t_variant", variant)
    try:
        got = ops.i2t_fold_layer(inp["x"], inp["ktok"], inp["vtok"], inp["wq"], inp["tabq"], inp["wo"], inp["bo"], inp["ln_w"],
                                 inp["ln_b"])
    finally:
        _lib.load().msam_tune_set(b"i2t_variant", 1)
    ref, bound = R.i2t_ref(inp, variant)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    _within(f"host i2t variant {variant} {gen} P={P} Nt={Nt}", got, ref, bound)
