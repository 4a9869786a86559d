"""msam_t2i_fold_attention (fold_q_kernel, fold_attn_kernel, fold_finish_kernel of csrc/decfold.hip) and msam_i2t_fold_layer (variant 1:
the token-owner kernel of csrc/decfold_tok.hip; variant 0: fold_q_kernel, fold_v_kernel, fold_i2t_kernel of csrc/decfold.hip) on the
device, called through ops.t2i_fold_attention / ops.i2t_fold_layer in the library's 16-bit type (``_lib.decoder_dtype()``: fp16 in the
shipped build), against the fp64 UNFOLDED formulation of tests/decoder_fold_ref.py computed on the device in chunks of prompts, and
within its ELEMENTWISE rounding bound for every element of every prompt (derivation: decoder_fold_ref's docstring).

Prompt counts: the kernels' key_splits is the smallest power of two with P * KS >= 512 (at most 16), i.e. 16 up to P = 63, 8 up to 127,
4 up to 255, 2 up to 511, 1 from 512.  The axis holds 1, 32, 33, 64, 65, 128, 129, 255, 256, 513 and both sides of every threshold of
that function (63 | 64, 127 | 128, 255 | 256, 511 | 512).  The launch grid is min(P * KS, 2 x CUs): with 256 CUs the persistent loop of
fold_attn_kernel / fold_i2t_kernel / i2t_tok_kernel runs from P = 33 (528 work items of 16 key splits) and for one key split at P = 513;
the "persistent" case takes max(513, 2 x CUs + 1) prompts from the CU count the device reports, and prints that count.  Per-prompt
streams below 64 prompts (and once at 129), the shared stream from 64.  Token counts 1..8 at P = 3, 256 and - for the fused
value-projection epilogue of one key split - 512.

tests/test_decoder_fold_ref_host.py proves that each defect these kernels are prone to (a dropped key tile or key split, splits merged
without rescaling, a missing table or bias term, crossed heads / prompts / value rows, unmasked padding tokens, bo shared as bo / Nt, a
missing residual, a shared stream read per prompt, an untouched last tile) is at least 4 bounds from the reference on one of these
generators, so a kernel with such a defect fails here.  Every case also checks: a second call returns the same bits; a prompt's result
does not depend on its neighbours (the same prompts in a launch of P - 1 are bit-identical: for t2i where P - 1 has the same key splits,
for i2t always - its split only divides the tokens among workgroups); i2t in place (out = x) equals out of place; t2i on the blocked
stream layout equals the row-major result (one case per key-split count).

Every case prints its max |got - ref| / bound (pytest -s); a value above 1 fails.  Measured on an MI355X (256 CUs), fp16 build:
t2i 0.056 - 0.728; i2t variant 1 0.045 - 0.465; i2t variant 0 0.056 - 0.492 of the bound over the 85 cases
(profiles/r10_decoder_fold_err_over_bound.md holds the table).  The bf16 ablation build is covered by the bf16 leg of the host
reference test only."""
import pytest
import torch

import decoder_fold_ref as R

pytestmark = pytest.mark.gpu

PERSISTENT = -1                                      # stands for 513; resolved on the device: max(513, 2 x CUs + 1) prompts


def _cases(generators, nt_ps):
    """(generator, P, Nt, shared) of both kernels; ``nt_ps``: the prompt counts of the token-count axis."""
    cases = [("diffuse", P, 7, False) for P in (1, 32, 33, 63)]
    cases += [("diffuse", P, 7, True) for P in (64, 65, 127, 128, 129, 255, 256, 511, 512, PERSISTENT)]
    cases += [("diffuse", 129, 7, False)]
    cases += [("diffuse", P, Nt, P >= 64) for P in nt_ps for Nt in range(1, 9)]
    for gen in generators:
        Nt = 5 if gen == "short" else 7
        cases += [(gen, 3, Nt, False), (gen, 128, Nt, True)]
    if "needle" in generators:                       # one P for each of 16 (persistent at 33), 8, 4, 2 key splits
        cases += [(gen, P, 7, P >= 64) for gen in ("needle", "split_skew") for P in (33, 64, 256)]
    return list(dict.fromkeys(cases))


def _id(case):
    gen, P, Nt, shared = case
    return f"{gen}-P{'persistent' if P == PERSISTENT else P}-Nt{Nt}-{'shared' if shared else 'own'}"


T2I_CASES = _cases(R.T2I_GENERATORS[1:], (3, 256, 512))
I2T_CASES = _cases(R.I2T_GENERATORS[1:], (3, 256))
BLOCKED_AT = {3, 64, 128, 256, 512}                  # one prompt count per key-split count: 16, 8, 4, 2, 1


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import _lib, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"\nthe device reports {cus} CUs: launch grids of at most {2 * cus} workgroups")
    return ops, _lib, torch.device("cuda"), cus


def _within(outputs, chunks):
    """``outputs``: [(label, kernel output, index of its bound in a chunk's bounds or None)]; ``chunks`` yields (lo, hi, ref, bound(s)).
    |got - ref| <= bound for every element, in ONE pass over the reference, chunk by chunk of prompts; prints each output's largest
    ratio and names its worst element."""
    state = [[-1.0, None, 0, 0] for _ in outputs]
    for lo, hi, ref, bounds in chunks:
        for st, (_, got, which) in zip(state, outputs):
            bound = bounds if which is None else bounds[which]
            err = (got[lo:hi].double() - ref).abs()
            ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.inf, 0.0))
            st[2] += int((err > bound).sum())
            st[3] += err.numel()
            i = int(ratio.argmax())
            if float(ratio.reshape(-1)[i]) > st[0]:
                st[0] = float(ratio.reshape(-1)[i])
                p, row, ch = (int(x) for x in torch.unravel_index(torch.tensor(i), err.shape))
                st[1] = (lo + p, row, ch, float(err[p, row, ch]), float(bound[p, row, ch]))
    failures = []
    for (what, _, _), (worst, where, nbad, total) in zip(outputs, state):
        print(f"\n{what}: max |got - ref| / bound = {worst:.3f}")
        if nbad:
            failures.append(f"{what}: {nbad} of {total} elements outside the bound; worst |got - ref| / bound = {worst:.3g} at prompt "
                            f"{where[0]} row {where[1]} channel {where[2]}: err {where[3]:.3g}, bound {where[4]:.3g}")
    if failures:
        pytest.fail("\n".join(failures))


def _first(inp, n, names, stream, shared):
    """The operands of the first ``n`` prompts alone."""
    out = dict(inp)
    for name in names:
        out[name] = inp[name][:n].contiguous()
    if not shared:
        out[stream] = inp[stream][:n].contiguous()
    return out


def _twice(inp, names):
    """One prompt twice (P = 1 has no smaller launch to be compared with)."""
    out = dict(inp)
    for name in names:
        out[name] = inp[name].repeat(2, 1, 1)
    return out


def _t2i(ops, inp, **kw):
    return ops.t2i_fold_attention(inp["keys"], inp["qtok"], inp["wk"], inp["tabk"], inp["wv"], inp["bv"], kv_shared=inp["kv_shared"], **kw)


def _i2t(ops, inp, **kw):
    return ops.i2t_fold_layer(inp["x"], inp["ktok"], inp["vtok"], inp["wq"], inp["tabq"], inp["wo"], inp["bo"], inp["ln_w"],
                              inp["ln_b"], x_shared=inp["x_shared"], **kw)


@pytest.mark.parametrize("case", T2I_CASES, ids=_id)
def test_t2i_fold_attention_within_the_rounding_bound(env, case):
    ops, _lib, dev, cus = env
    gen, P, Nt, shared = case
    if P == PERSISTENT:
        P = max(513, 2 * cus + 1)
    ks = R.key_splits(P)
    inp = R.to_device(R.make_t2i(gen, _lib.decoder_dtype(), P, Nt, shared, seed=5), dev)
    got = _t2i(ops, inp)
    again = _t2i(ops, inp)
    assert got.shape == (P, Nt, 128) and got.dtype == _lib.decoder_dtype()
    assert bool(torch.isfinite(got).all())
    what = f"t2i {gen} P={P} Nt={Nt} {'shared' if shared else 'own'} KS={ks} items={P * ks} grid={min(P * ks, 2 * cus)}"
    _within([(what, got, None)], R.t2i_ref_chunks(inp, chunk=8))
    assert torch.equal(got, again)                                                         # no atomics: run to run identical
    if P == 1:
        both = _t2i(ops, dict(_twice(inp, ("qtok",)), kv_shared=True))
        assert torch.equal(both[0:1], got) and torch.equal(both[1:2], got)
    elif R.key_splits(P - 1) == ks:                                                        # the first P - 1 prompts alone
        assert torch.equal(_t2i(ops, _first(inp, P - 1, ("qtok",), "keys", shared)), got[:P - 1])
    if P in BLOCKED_AT and gen in ("diffuse", "needle"):                                   # (blocked streams are per prompt)
        own = inp["keys"].expand(P, -1, -1) if shared else inp["keys"]
        blocked = dict(inp, keys=ops.to_blocked(own), kv_shared=False)
        assert torch.equal(_t2i(ops, blocked, blocked=True), got)


@pytest.mark.parametrize("case", I2T_CASES, ids=_id)
def test_i2t_fold_layer_within_the_rounding_bound(env, case):
    """Both variants in one case: they share the fp64 reference, each has its own bound."""
    ops, _lib, dev, cus = env
    gen, P, Nt, shared = case
    if P == PERSISTENT:
        P = max(513, 2 * cus + 1)
    ks = R.key_splits(P)
    inp = R.to_device(R.make_i2t(gen, _lib.decoder_dtype(), P, Nt, shared, seed=5), dev)
    got = {}
    try:
        for variant in (1, 0):
            _lib.load().msam_tune_set(b"i2t_variant", variant)
            got[variant] = y = _i2t(ops, inp)
            assert y.shape == (P, R.T, 256) and y.dtype == _lib.decoder_dtype()
            assert bool(torch.isfinite(y).all())
            assert torch.equal(_i2t(ops, inp), y)                                          # run to run identical
            if P == 1:
                both = _i2t(ops, dict(_twice(inp, ("ktok", "vtok")), x_shared=True))
                assert torch.equal(both[0:1], y) and torch.equal(both[1:2], y)
            else:                                                                          # the first P - 1 prompts alone
                assert torch.equal(_i2t(ops, _first(inp, P - 1, ("ktok", "vtok"), "x", shared)), y[:P - 1])
            if not shared:                                                                 # in place
                x2 = inp["x"].clone()
                _i2t(ops, dict(inp, x=x2), out=x2)
                assert torch.equal(x2, y)
    finally:
        _lib.load().msam_tune_set(b"i2t_variant", 1)
    what = f"{gen} P={P} Nt={Nt} {'shared' if shared else 'own'} KS={ks} items={P * ks} grid={min(P * ks, 2 * cus)}"
    _within([(f"i2t variant {v} {what}", got[v], i) for i, v in enumerate((1, 0))], R.i2t_ref_chunks(inp, (1, 0), chunk=8))
