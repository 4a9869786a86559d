"""Device pin of the weights-stationary decoder GEMM (csrc/wsgemm.hip, ``msam_wsgemm_bf16``) - harness, generators and references in
tests/wsgemm_ref.py.

* Exact cases: integer operands, so every output element must EQUAL the round-to-nearest-even 16-bit cast of the exact result, bit for bit,
  in every layout (plain, head-major, k | vT), for all four (N, K) - both ``EPI`` instantiations of each.  The shapes are the smallest that
  reach the code: M = 64 ... 384 (2 ... 12 tiles of 32 rows), wrap lengths that end inside a tile (table_rows 7, resid_rows 40, tokens 48)
  and across tiles (resid_rows 96), ``table_ld`` = table_cols + 4, ``ldr`` = N + 8, ``ldc`` = N + 4.
* The persistent loop: a launch starts min(M / 32, 512) workgroups, so only M > 16384 makes a workgroup take a second tile.  M = 16384,
  16448, 32768, 34880, 49280 are 512, 514, 1024, 1090 and 1540 tiles: one pass; 1 and 2 iterations mixed; two; 2 and 3 mixed; 3 and 4
  mixed (both register sets reused, the clamped prefetch, the guarded LDS store and the buffer flip all run).  Bit for bit again; rows of A
  are distinct across the whole M, so a stale, repeated or misplaced tile shows.
* LayerNorm epilogues and one Gaussian case per (N, K) against float64, with derived bounds (``wsgemm_ref.ln_bound`` / ``gauss_bound``).
* Refusals: status != 0, nothing launched, every output untouched.

Every call checks the NaN sentinels around all buffers and that the outputs its mode does not write stay untouched.  The bodies take a
``dev`` fixture: tests/test_wsgemm_host.py runs them against the host-compiled library.  Lines starting with "FIG" carry the figures
recorded in profiles/wsgemm_device.md (pytest -s)."""
import pytest
import torch

import wsgemm_ref as R

pytestmark = pytest.mark.gpu

NK = [(128, 128), (128, 256), (256, 128), (256, 256)]
LOOP_M = [16384, 16448, 32768, 34880, 49280]
# name -> (N, K, generator keywords, launch keywords); 'hm' is the launch of decoder.hip's wsgemm_kv (tokens = 4096 where it divides M)
LOOP_KINDS = {
    "k128-plain": (128, 128, {}, {}),
    "k256-plain": (256, 256, {}, {}),
    "k128-resid": (256, 128, dict(resid=True), {}),
    "k256-resid-table": (256, 256, dict(resid=True, table=64), {}),
    "kv-split": (256, 128, dict(table=128), dict(kv_split=1, tokens=64)),
    "head-major": (128, 256, dict(table=128, table_rows=4096), dict(head_major=1)),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _fig(case, **kv):
    print("FIG wsgemm", case, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def run_exact(dev, c, name, **launch):
    """One launch of an integer case: exactly one kernel launch recorded, every output bit-equal to the exact reference."""
    lay = {k: launch[k] for k in ("kv_split", "tokens", "head_major") if k in launch}
    r, n = R.launches(lambda: R.call(dev, c, **launch))
    assert n == 1, f"{name}: {n} launches recorded"
    exp = R.expected(c, dev, **lay)
    assert set(exp) <= set(r), (name, sorted(r))
    R.assert_bits(r, exp, name)
    return r


# ---- exact cases at the smallest shapes

@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("N,K", NK)
def test_plain(dev, N, K, M):
    run_exact(dev, R.exact_case(M, N, K, 100 + M + N + 3 * K, dev=dev), f"plain M{M} N{N} K{K}")


@pytest.mark.parametrize("tc", [4, 64, "N"])
@pytest.mark.parametrize("N,K", NK)
def test_table(dev, N, K, tc):
    """table_rows = 7 wraps in the middle of every tile; table_ld = table_cols + 4, so a read beyond table_cols meets a NaN."""
    tc = N if tc == "N" else tc
    run_exact(dev, R.exact_case(128, N, K, 200 + N + 3 * K + tc, table=tc, dev=dev), f"table{tc} N{N} K{K}")


@pytest.mark.parametrize("rr", [0, 40, 96])
@pytest.mark.parametrize("N,K", NK)
def test_residual(dev, N, K, rr):
    """resid_rows 40 wraps inside the second tile, 96 at a tile boundary, 0 reads row for row."""
    run_exact(dev, R.exact_case(192, N, K, 300 + N + 3 * K + rr, resid=True, resid_rows=rr, dev=dev), f"resid{rr} N{N} K{K}")


@pytest.mark.parametrize("N,K", NK)
def test_residual_in_place(dev, N, K):
    """``out`` aliases ``resid`` (resid_rows = 0): the decoder's in-place stream update."""
    run_exact(dev, R.exact_case(192, N, K, 400 + N + 3 * K, resid=True, table=64, dev=dev), f"in place N{N} K{K}", inplace=True)


@pytest.mark.parametrize("table", [None, 128])
@pytest.mark.parametrize("tokens", [64, 48])
@pytest.mark.parametrize("N,K", NK)
def test_head_major(dev, N, K, tokens, table):
    """[M / tokens][N / 16][tokens][16] with 8 (N = 128) or 16 heads; tokens = 48 puts an image boundary inside every other tile."""
    c = R.exact_case(192, N, K, 500 + N + 3 * K + tokens + (table or 0), table=table, dev=dev)
    run_exact(dev, c, f"head-major N{N} K{K} tokens{tokens} table{table}", head_major=1, tokens=tokens)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("tokens", [64, 128])
@pytest.mark.parametrize("N,K", NK)
def test_kv_split(dev, N, K, tokens, table):
    """M = 384: 6 or 3 images per launch.  N = 256: k_out <- columns 0..127 (the table lies on this half), vT_out <- the rest transposed;
    N = 128: everything transposed into vT_out and k_out - handed over as a sentinel buffer - stays untouched (``call`` asserts it)."""
    c = R.exact_case(384, N, K, 600 + N + 3 * K + tokens + table, table=((128 if N == 256 else 64) if table else None), dev=dev)
    r = run_exact(dev, c, f"kv-split N{N} K{K} tokens{tokens} table{table}", kv_split=1, tokens=tokens)
    assert ("k" in r) == (N == 256)


# ---- the persistent loop

def run_persistent(dev, M, kind):
    N, K, gen, launch = LOOP_KINDS[kind]
    launch = dict(launch)
    if launch.get("head_major"):
        launch["tokens"] = 4096 if M % 4096 == 0 else 64
    c = R.exact_case(M, N, K, 700 + M % 1000 + N + 3 * K, dev=dev, **gen)
    run_exact(dev, c, f"persistent M{M} {kind}", **launch)


@pytest.mark.parametrize("kind", list(LOOP_KINDS))
@pytest.mark.parametrize("M", LOOP_M)
def test_persistent_loop(dev, M, kind):
    run_persistent(dev, M, kind)


# ---- LayerNorm epilogues against float64

LN_CASES = [(1, 256, 256, 0, True), (1, 256, 128, 40, False), (1, 256, 256, 0, False), (2, 128, 256, 0, True), (2, 128, 128, 40, False),
            (2, 256, 128, 0, True), (2, 256, 256, 96, False)]


@pytest.mark.parametrize("mode,N,K,rr,inplace", LN_CASES)
def test_layernorm_epilogues(dev, mode, N, K, rr, inplace):
    """ln_mode 1 (LayerNorm over the 256-wide row) and ln_mode 2 (LayerNorm over groups of 64 columns + GELU) on exact integer
    pre-activations, residual included, also in place.  Bound: ``wsgemm_ref.ln_bound``.  The row of variance 0 must give round16(ln_b) bit for
    bit (mode 1: 0 * rstd * w + b) and round16(gelu_erf(ln_b)) within the bound (mode 2)."""
    d = R.d16()
    eps = 1e-5 if mode == 1 else 1e-6
    c = R.ln_case(192, N, K, 800 + mode + N + 3 * K + rr, mode, resid_rows=rr, dev=dev)
    r, n = R.launches(lambda: R.call(dev, c, ln_mode=mode, ln_eps=eps, inplace=inplace))
    assert n == 1
    ref = R.result64(c, dev, ln_mode=mode, ln_eps=eps)
    ratio = R.max_ratio(r["out"], ref, R.ln_bound(ref, mode, d))
    row = c["const_row"]
    lb = c["ln_b"].repeat(N // c["ln_b"].numel()).to(dev)
    if mode == 1:
        R.assert_bits({"out": r["out"][row]}, {"out": lb.to(d)}, f"ln_mode 1 N{N} K{K}: the row of variance 0")
        const_ratio = 0.0
    else:
        want = R.G.gelu64(lb.double())
        const_ratio = R.max_ratio(r["out"][row], want, R.ln_bound(want, 2, d))
    _fig(f"ln_mode{mode}-N{N}-K{K}-resid_rows{rr}{'-inplace' if inplace else ''}", err_over_bound=ratio, const_row_err_over_bound=const_ratio,
         not_rne_of_ref=R.share_off(r["out"], ref))
    assert ratio <= 1.0 and const_ratio <= 1.0, (ratio, const_ratio)


# ---- Gaussian operands against float64

@pytest.mark.parametrize("N,K", NK)
def test_gaussian(dev, N, K):
    """Bias + table + wrapped residual on Gaussian operands against the float64 product of the same 16-bit operands; the bound is
    ``wsgemm_ref.gauss_bound``: fp32 arithmetic in any order plus the output cast, nothing measured."""
    d = R.d16()
    c = R.random_case(192, N, K, 900 + N + 3 * K, table=64, resid=True, resid_rows=40, dev=dev)
    r, n = R.launches(lambda: R.call(dev, c))
    assert n == 1
    ref = c["ref"].to(dev)
    ratio = R.max_ratio(r["out"], ref, R.gauss_bound(c, dev, d))
    _fig(f"gaussian-N{N}-K{K}", err_over_bound=ratio, not_rne_of_ref=R.share_off(r["out"], ref))
    assert ratio <= 1.0, ratio


# ---- refusals

def refusal_cases():
    kv, hm = dict(kv_split=1, tokens=64), dict(head_major=1, tokens=64)
    cases = [(f"M={m}", dict(M=m)) for m in (0, 32, 96)]
    cases += [(f"N={n}", dict(N=n)) for n in (64, 192)] + [(f"K={k}", dict(K=k)) for k in (64, 192)]
    cases += [("kv-split tokens=96", dict(kv_split=1, tokens=96)), ("kv-split tokens=0", dict(kv_split=1, tokens=0)),
              ("kv-split tokens=-64", dict(kv_split=1, tokens=-64)), ("kv-split tokens=128 not dividing M", dict(kv_split=1, tokens=128)),
              ("kv-split with ln_mode", dict(kv, ln_mode=2)), ("kv-split N=256 without k_out", dict(kv, null=("k_out",))),
              ("kv-split without vT_out", dict(kv, null=("vT_out",))), ("head_major with kv-split", dict(hm, kv_split=1)),
              ("head_major tokens=80", dict(head_major=1, tokens=80)), ("head_major tokens=0", dict(head_major=1, tokens=0)),
              ("ln_mode 1 with N=128", dict(ln_mode=1, N=128)), ("ln_mode 3", dict(ln_mode=3)), ("ln_mode -1", dict(ln_mode=-1)),
              ("ln_mode 2 without ln_w", dict(ln_mode=2, null=("ln_w",))), ("ln_mode 1 without ln_b", dict(ln_mode=1, null=("ln_b",))),
              ("null out", dict(null=("out",))), ("table_cols=2", dict(table_cols=2)), ("table_cols=6", dict(table_cols=6)),
              ("table_cols=-4", dict(table_cols=-4))]
    return cases


def test_refusals(dev):
    """Each refusal returns a non-zero status, launches nothing and leaves out, k_out and vT_out untouched (``call`` asserts the latter
    for every non-zero status).  table_cols that is no multiple of 4 used to be accepted: the kernel then added the table up to the next
    multiple of 4 and read past the end of each table row."""
    c = dict(R.exact_case(192, 256, 256, 1000, table=8, resid=True, dev=dev))
    c["ln_w"], c["ln_b"] = torch.ones(256), torch.zeros(256)
    for name, launch in refusal_cases():
        r, n = R.launches(lambda: R.call(dev, c, expect_ok=False, **launch))
        assert r["status"] != 0, f"{name}: accepted"
        assert n == 0, f"{name}: refused with status {r['status']} after a launch"
        assert r["error"].startswith("msam_wsgemm_bf16"), (name, r["error"])
        if name.startswith("table_cols"):
            assert "table_cols" in r["error"] and "multiple of 4" in r["error"], r["error"]
    run_exact(dev, c, "the refusals' case as it stands")            # the same case, unmodified, is accepted


def test_refusal_by_the_wrapper(dev):
    """``ops.wsgemm`` refuses table_cols = 6 itself, before anything is handed to the library, and leaves ``out`` untouched."""
    from micro_sam_amd import ops
    d = R.d16()
    a, w = torch.ones(64, 128, dtype=d, device=dev), torch.ones(128, 128, dtype=d, device=dev)
    table = torch.ones(7, 6, device=dev)
    out = R.Padded(64, 128, 128, d, dev)
    with pytest.raises(ValueError, match="table_cols = 6 must be a multiple of 4"):
        R.launches(lambda: ops.wsgemm(a, w, table=table, table_cols=6, out=out.view))
    assert out.unchanged()
    got, n = R.launches(lambda: ops.wsgemm(a, w, table=torch.ones(7, 8, device=dev), table_cols=4, out=out.view))
    assert n == 1 and got is out.view and out.padding_intact()
    exp = torch.full((64, 128), 128.0)
    exp[:, :4] += 1
    assert torch.equal(got.float().cpu(), exp)
