"""The proof behind tests/test_gpu_attention.py: every defect listed in attention_ref.MUTATIONS, written as a variant of the fp64
reference, is at least 4 of attention_ref's elementwise bounds away from the reference on the generator meant for it.  A kernel output
within one bound of the truth is then at least 3 bounds from the mutant, so a kernel WITH that defect (which is within one bound of the
mutant) fails the device test on these inputs.  This is a condition on the generators, not a measurement of a kernel: where a generator
does not reach 4, the generator is what changes.

Both 16-bit types (the bound and the operands' rounding differ); B = 1 and heads = 1 unless the defect needs a second head or image."""
import functools

import pytest
import torch

import attention_ref as R

# mutation -> (kinds, generator, stored head_dim, B, heads)
CASES = {
    "rel_h_plus1": (("window", "global"), "rel_only", 64, 1, 1),
    "rel_w_plus1": (("window", "global"), "rel_only", 64, 1, 1),
    "rel_swap_hw": (("window", "global"), "rel_only", 64, 1, 1),
    "rel_sign": (("window", "global"), "rel_only", 64, 1, 1),
    "drop_last32": (("global",), "needle", 64, 1, 1),
    "drop_192": (("window",), "needle", 64, 1, 1),
    "swap_v_rows": (("window", "global"), "needle", 64, 1, 1),
    "pad_zero": (("window",), "padding_aligned", 64, 1, 1),
    "pad_masked": (("window",), "padding_aligned", 64, 1, 1),
    "swap_heads": (("window", "global"), "peaked", 64, 1, 2),
    "image1_from_image0": (("window", "global"), "peaked", 64, 2, 1),
    "scale_96": (("window", "global"), "peaked", 96, 1, 1),
}
PARAMS = [(m, kind) for m, c in CASES.items() for kind in c[0]]


@functools.lru_cache(maxsize=None)
def _truth(kind, gen, hs, B, heads, dtype=torch.bfloat16):
    inp = R.make_inputs(kind, gen, dtype, hs, B, heads, seed=0)
    return inp, R.attention_ref(kind, inp)


def test_every_mutation_has_a_case():
    assert set(CASES) == set(R.MUTATIONS)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mutation,kind", PARAMS)
def test_mutation_is_four_bounds_from_the_reference(mutation, kind, dtype):
    _, gen, hs, B, heads = CASES[mutation]
    inp, (ref, bound) = _truth(kind, gen, hs, B, heads, dtype)
    # (image 0 of "image1_from_image0" is right by construction: only image 1 is recomputed and compared)
    only_image1 = mutation == "image1_from_image0"
    mut, _ = R.attention_ref(kind, inp, mutation, pairs=[(1, 0)] if only_image1 else None)
    rows = slice(R.TOK, None) if only_image1 else slice(None)
    ref, bound, mut = ref[rows], bound[rows], mut[rows]
    live = bound > 0                                                        # (zero-padded channels: reference 0, bound 0)
    ratio = ((mut - ref).abs()[live] / bound[live]).max().item()
    print(f"{mutation} / {kind} / {gen}: max |mutant - ref| / bound = {ratio:.1f}")
    assert ratio >= 4.0, ratio


@pytest.mark.parametrize("kind", ["window", "global"])
@pytest.mark.parametrize("hs", [64, 96])
def test_needle_puts_its_weight_on_one_key(kind, hs):
    """What the needle generator promises, for both head dims: exactly one key matches each query and it takes >= 0.9999 of the weight,
    so the reference output is v[pi(i)] to 2e-4 max |v| (a whole wrong row is off by the order of |v|)."""
    inp, (ref, bound) = _truth(kind, "needle", hs, 1, 1)
    q, k, v = (inp[n][0, 0].double() for n in "qkv")
    match = (q @ k.t() == 4.0 * inp["head_dim"])                           # q_i = 4 k_pi(i): the dot product is 4 head_dim at pi(i) only
    assert bool((match.sum(dim=1) == 1).all())
    want = v[match.double().argmax(dim=1)]
    assert float((ref - want).abs().max()) <= 2e-4 * float(v.abs().max())


def test_padding_aligned_output_is_the_value_bias_in_the_edge_windows():
    inp, (ref, _) = _truth("window", "padding_aligned", 64, 1, 1)
    bv = R.round16(inp["qkv_bias"].reshape(3, 64)[2], torch.bfloat16)
    edge = ref.reshape(64, 64, 64)[56:, 56:]                                # the corner window: 132 of 196 keys are bias-only
    assert float((edge - bv).abs().max()) <= 0.02 * float(bv.abs().max())


def test_scores_stay_where_the_bound_holds():
    """The bound's fp32 term assumes |s| well below 60."""
    for kind in ("window", "global"):
        for gen in R.GENERATORS[kind]:
            inp = R.make_inputs(kind, gen, torch.bfloat16, 96, 1, 1, seed=0)
            q, k = inp["q"][0, 0].double(), inp["k"][0, 0].double()
            rows = torch.arange(0, R.TOK, 37)
            s = inp["scale"] * q[rows] @ k.t()
            t = q[rows] @ torch.cat([inp["rel_h"], inp["rel_w"]]).double().t()
            assert float(s.abs().max() + 2 * t.abs().max()) < 60.0, (kind, gen)
