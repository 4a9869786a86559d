"""The kernels of the split16 precision mode (csrc/strict.hip) on the device, family by family through the C ABI, against the fp64
UNFUSED formulation of tests/split16_ref.py computed on the device, within its ELEMENTWISE rounding bound for every element of every
output (derivation: split16_ref's docstring; the bounds are derived from the kernels' arithmetic, not calibrated):

  msam_strict_gemm           split16 = 1 AND split16 = 0 (the fp32 product, its own bound) over one table of 20 cases x the three tile
                             routes (64 x 64; 128 x 128 NBUF 1; NBUF 2 - msam_tune_set sgemm_small_below / sgemm_bufs): tile edges in
                             M, N and K, every epilogue, A2 with fewer rows than M and for the first 128 columns only, a wrapped
                             residual, col_scale / col_shift, the 2 x 2 transposed-convolution store, the implicit 3 x 3 form, a weight
                             with a 2^20 dynamic range; the three routes give equal bits
  msam_split16_prepare_pairs bit for bit, both k orders, K = 32 / 128 / 256, N K / 4 not a multiple of the 256-thread block
  msam_split16_t2i_attention Tk = 1..8 at B = 3, every generator at Tk 7 and 8, B = 1 and B = CUs + 1 (a second dispatch round on a
                             CU's LDS), ldq / ldo > 128
  msam_split16_i2t_block     Tk = 1..8, shared and per-prompt stream, in place = out of place, B = 1, 3, CUs + 1
  msam_strict_i2t_block      split16 = 1: Tk in {1, 8, 9, 15, 16}, shared / own stream, with and without prepared pairs (equal bits)
  msam_strict_upscale2       P = 1, 2, 3; (mask0, nmask) in {(0, 1), (1, 3), (0, 4), (3, 1)}; hyper_ld 32 and 40; scaled rows of u1
  msam_split16_relpos_attention  global: grid 64, head dim 64 / 80, 1 / 2 heads; windows: grid 14 (exact), 20 (one padded window per
                             axis), 64 (the ViT's own), head dim 64 / 80, two images of two heads; diffuse, a needle on the padded keys
                             of the last window row, a signature per image and head

Every output is pre-filled with NaN; workspaces have exactly the documented size and a NaN guard behind them that must stay untouched;
a second call returns the same bits; a prompt's bits do not depend on its neighbours (the same prompts in a launch of B - 1).
tests/test_split16_ref_host.py proves every named defect of these kernels at least 4 bounds from the reference on one of the
generators used here.  Every case prints its max |got - ref| / bound (pytest -s); a value above 1 fails.  Measured on an MI355X
(256 CUs): 0.000 - 0.466 over the 112 tests, the whole file in 6 s (profiles/r16_split16_err_over_bound.md holds the table)."""
import pytest
import torch

import split16_calls as K
import split16_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"\nthe device reports {cus} CUs")
    return _lib.load(), _lib, torch.device("cuda"), cus


def _report(what, r):
    print(f"\n{what}: max |got - ref| / bound = {r:.3f}")
    return r


# --------------------------------------------------------------------------------------------------------------------- the product
@pytest.mark.parametrize("case", R.PRODUCT_CASES, ids=R.product_case_id)
def test_product_every_route_within_the_bound(env, case):
    lib, L, dev, _ = env
    name, M, N, Kk, opt = case
    inp = R.to_device(R.make_product(name, M, N, Kk, seed=5, **opt), dev)
    worst = 0.0
    for split in (True, False):
        ref, bound = R.product_ref(inp, split=split)
        outs = {}
        for route, knobs in K.ROUTES.items():
            with K.tuned(lib, **knobs):
                outs[route] = K.gemm(lib, L, inp, split=split, stream=L.stream_ptr())
                again = K.gemm(lib, L, inp, split=split, stream=L.stream_ptr())
            assert torch.equal(outs[route], again)
            worst = max(worst, _report(f"product {R.product_case_id(case)} split16={int(split)} {route}", K.ratio(outs[route], ref, bound)))
        assert torch.equal(outs["tile64"], outs["tile128_nbuf1"]) and torch.equal(outs["tile64"], outs["tile128_nbuf2"])
    assert worst <= 1.0


@pytest.mark.parametrize("N,Kk,permute", [(5, 32, 0), (5, 32, 1), (3, 128, 0), (129, 128, 1), (128, 256, 0), (7, 256, 1)])
def test_prepared_pairs_are_bit_exact(env, N, Kk, permute):
    lib, L, dev, _ = env
    assert (N * Kk // 4) % 256 or N == 128
    w = R.make_product("diffuse", 1, N, Kk, seed=6, w_range=20)["w"].to(dev)
    scale = R.weight_scale(w)
    got, guard = K.prepare_pairs(lib, w, scale, permute, stream=L.stream_ptr())
    assert torch.equal(got.view(torch.int16), R.pairs_ref(w, scale, permute).view(torch.int16))
    assert K.guard_untouched(guard)


# ----------------------------------------------------------------------------------------------------------------------------- t2i
def _t2i_within(what, got, inp):
    worst = 0.0
    for lo, hi, ref, bound in R.t2i_ref_chunks(inp, chunk=4):
        worst = max(worst, K.ratio(got[lo:hi], ref, bound))
    return _report(what, worst)


T2I_CASES = [("diffuse", 3, Tk) for Tk in range(1, 9)] + [(g, 2, Tk) for g in R.T2I_GENERATORS for Tk in (7, 8)] + \
    [("diffuse", 1, 7), ("needle", 1, 8), ("distinct", -1, 7)]


@pytest.mark.parametrize("gen,B,Tk", T2I_CASES, ids=lambda v: str(v) if not isinstance(v, int) or v >= 0 else "CUs+1")
def test_t2i_attention_within_the_bound(env, gen, B, Tk):
    lib, L, dev, cus = env
    if B < 0:
        B = cus + 1
        inp = R.widen_t2i(R.to_device(R.make_t2i(gen, 4, Tk, seed=5), dev), B)
        R.check_t2i_domain(inp)
    else:
        inp = R.to_device(R.make_t2i(gen, B, Tk, seed=5), dev)
    ld = (128, 128) if (B, Tk) == (3, 4) else (132, 136)
    got, guard = K.t2i(lib, L, inp, *ld, stream=L.stream_ptr())
    again, _ = K.t2i(lib, L, inp, *ld, stream=L.stream_ptr())
    r = _t2i_within(f"t2i {gen} B={B} Tk={Tk} ldq={ld[0]} ldo={ld[1]}", got, inp)
    assert K.guard_untouched(guard)
    assert torch.equal(got, again)
    if B > 1:                                                                              # the first B - 1 prompts alone
        fewer = dict(inp, keys=inp["keys"][:B - 1].contiguous(), q=inp["q"][:B - 1].contiguous())
        assert torch.equal(K.t2i(lib, L, fewer, *ld, stream=L.stream_ptr())[0], got[:B - 1])
    assert r <= 1.0


# ----------------------------------------------------------------------------------------------------------------------------- i2t
def _i2t_within(outputs, inp, forms):
    """outputs: [(label, tensor, index into forms)]"""
    worst = [0.0] * len(outputs)
    for lo, hi, ref, bounds in R.i2t_ref_chunks(inp, forms, chunk=4):
        for i, (_, got, which) in enumerate(outputs):
            worst[i] = max(worst[i], K.ratio(got[lo:hi], ref, bounds[which]))
    return [_report(what, w) for (what, _, _), w in zip(outputs, worst)]


def _fewer_i2t(inp, n):
    out = dict(inp, tok_k=inp["tok_k"][:n].contiguous(), tok_v=inp["tok_v"][:n].contiguous())
    if not inp["shared"]:
        out["keys"] = inp["keys"][:n].contiguous()
    return out


I2T_FOLDED_CASES = [("diffuse", 3, Tk, Tk % 2 == 0) for Tk in range(1, 9)] + \
    [(g, 2, 5, shared) for g in R.I2T_GENERATORS[1:] for shared in (False, True)] + \
    [("diffuse", 1, 7, False), ("flat", 1, 1, True), ("distinct", -1, 7, True)]


@pytest.mark.parametrize("gen,B,Tk,shared", I2T_FOLDED_CASES, ids=lambda v: str(v) if not isinstance(v, int) or v >= 0 else "CUs+1")
def test_i2t_folded_block_within_the_bound(env, gen, B, Tk, shared):
    lib, L, dev, cus = env
    if B < 0:
        B = cus + 1
        inp = R.widen_i2t(R.to_device(R.make_i2t(gen, 4, Tk, True, seed=5), dev), B)
        R.check_i2t_domain(inp)
    else:
        inp = R.to_device(R.make_i2t(gen, B, Tk, shared, seed=5), dev)
    got, guard = K.i2t_folded(lib, L, inp, stream=L.stream_ptr())
    again, _ = K.i2t_folded(lib, L, inp, stream=L.stream_ptr())
    r, = _i2t_within([(f"i2t folded {gen} B={B} Tk={Tk} {'shared' if shared else 'own'}", got, 0)], inp, ("folded",))
    assert K.guard_untouched(guard)
    assert torch.equal(got, again)
    if B > 1:
        assert torch.equal(K.i2t_folded(lib, L, _fewer_i2t(inp, B - 1), stream=L.stream_ptr())[0], got[:B - 1])
    if not shared:
        own = dict(inp, keys=inp["keys"].clone())
        assert torch.equal(K.i2t_folded(lib, L, own, in_place=True, stream=L.stream_ptr())[0], got)
    assert r <= 1.0


I2T_UNFOLDED_CASES = [("diffuse", 3, Tk, Tk % 2 == 1) for Tk in (1, 8, 9, 15, 16)] + \
    [("diffuse", 1, 9, False), ("distinct", 1, 16, True), ("flat", 3, 8, True), ("magnitudes", 3, 15, False), ("duel", 3, 9, False),
     ("duel", 1, 8, True)]


@pytest.mark.parametrize("gen,B,Tk,shared", I2T_UNFOLDED_CASES)
def test_i2t_unfolded_block_within_the_bound(env, gen, B, Tk, shared):
    lib, L, dev, _ = env
    inp = R.to_device(R.make_i2t(gen, B, Tk, shared, seed=7), dev)
    got = K.i2t_unfolded(lib, L, inp, stream=L.stream_ptr())
    assert torch.equal(K.i2t_unfolded(lib, L, inp, stream=L.stream_ptr()), got)
    pairs = (K.prepare_pairs(lib, inp["wq"], inp["wq_scale"], 0, stream=L.stream_ptr())[0],
             K.prepare_pairs(lib, inp["wo"], inp["wo_scale"], 1, stream=L.stream_ptr())[0])
    prepared = K.i2t_unfolded(lib, L, inp, pairs=pairs, stream=L.stream_ptr())
    what = f"{gen} B={B} Tk={Tk} {'shared' if shared else 'own'}"
    outputs = [(f"i2t unfolded {what}", got, 0), (f"i2t unfolded, prepared pairs {what}", prepared, 0)]
    forms = ("unfolded",)
    if Tk <= 8:                                                                            # the folded kernel on the same operands
        outputs.append((f"i2t folded {what}", K.i2t_folded(lib, L, inp, stream=L.stream_ptr())[0], 1))
        forms = ("unfolded", "folded")
    ratios = _i2t_within(outputs, inp, forms)
    assert torch.equal(prepared, got)                                                      # the same halves at the same LDS places
    if B > 1:
        assert torch.equal(K.i2t_unfolded(lib, L, _fewer_i2t(inp, B - 1), stream=L.stream_ptr()), got[:B - 1])
    if not shared:
        own = dict(inp, keys=inp["keys"].clone())
        assert torch.equal(K.i2t_unfolded(lib, L, own, in_place=True, stream=L.stream_ptr()), got)
    assert max(ratios) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------------- up2
UP2_CASES = [("diffuse", P, m0, nm, ld) for P, (m0, nm), ld in ((1, (0, 1), 32), (2, (1, 3), 40), (3, (0, 4), 32), (1, (3, 1), 40),
                                                                 (2, (0, 4), 40), (3, (1, 3), 32))] + \
    [("magnitudes", 2, 1, 3, 40), ("magnitudes", 1, 0, 4, 32)]


@pytest.mark.parametrize("gen,P,mask0,nmask,ld", UP2_CASES)
def test_upscale2_within_the_bound(env, gen, P, mask0, nmask, ld):
    lib, L, dev, _ = env
    inp = R.to_device(R.make_up2(gen, P, mask0, nmask, ld, seed=5), dev)
    got, guard = K.up2(lib, L, inp, stream=L.stream_ptr())
    again, _ = K.up2(lib, L, inp, stream=L.stream_ptr())
    worst = 0.0
    for p, ref, bound in R.up2_ref_chunks(inp):
        worst = max(worst, K.ratio(got[p], ref, bound))
    _report(f"up2 {gen} P={P} mask0={mask0} nmask={nmask} hyper_ld={ld}", worst)
    assert K.guard_untouched(guard) and torch.equal(got, again)
    if P > 1:                                                                              # the first P - 1 prompts alone
        fewer = dict(inp, P=P - 1, u1=inp["u1"][:(P - 1) * 16384].contiguous(), hyper=inp["hyper"][:P - 1].contiguous())
        assert torch.equal(K.up2(lib, L, fewer, stream=L.stream_ptr())[0], got[:P - 1])
    assert worst <= 1.0


# -------------------------------------------------------------------------------------------------------------------------- relpos
RELPOS_CASES = [(gen, 1, heads, hd, 64, 0) for gen, heads, hd in (("diffuse", 1, 64), ("diffuse", 2, 80), ("needle", 2, 64), ("distinct", 1, 80),
                                                                   ("distinct", 2, 64))] + \
    [(gen, 2, 2, hd, G, 14) for gen in R.RELPOS_GENERATORS for hd, G in ((64, 14), (80, 20), (64, 64), (80, 14), (64, 20))] + \
    [("diffuse", 2, 2, 80, 64, 14)]


@pytest.mark.parametrize("gen,B,heads,hd,G,window", RELPOS_CASES)
def test_relpos_attention_within_the_bound(env, gen, B, heads, hd, G, window):
    lib, L, dev, _ = env
    inp = R.to_device(R.make_relpos(gen, B, heads, hd, G, window, seed=5), dev)
    got, guard = K.relpos(lib, inp, stream=L.stream_ptr())
    again, _ = K.relpos(lib, inp, stream=L.stream_ptr())
    ref, bound = R.relpos_ref(inp)
    r = _report(f"relpos {gen} B={B} heads={heads} hd={hd} grid={G} window={window}", K.ratio(got, ref, bound))
    assert K.guard_untouched(guard) and torch.equal(got, again)
    if B > 1:                                                                              # the first image alone
        fewer = dict(inp, B=B - 1, qkv=inp["qkv"][:(B - 1) * G * G].contiguous())
        assert torch.equal(K.relpos(lib, fewer, stream=L.stream_ptr())[0], got[:(B - 1) * G * G])
    assert r <= 1.0
