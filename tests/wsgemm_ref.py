"""Harness, operand generators and references for the device pin of the weights-stationary decoder GEMM (csrc/wsgemm.hip:
``msam_wsgemm_bf16``).  Pure Python / torch, built on tests/gemm_ref.py: the same code drives the GPU library (tests/test_gpu_wsgemm.py) and
the host-compiled one (tests/test_wsgemm_host.py), with the decoder's 16-bit type being fp16 (the default build) or bf16 (``--dec-bf16``).

* ``call`` fills ``_lib.WsGemmParams`` directly, so every field of the ABI is reachable: ``table_ld`` wider than the table, ``ldr``, ``ldc``,
  ``resid_rows``, ``tokens``, an ``out`` that aliases ``resid``, overridden M / N / K, missing pointers.  Every buffer is a ``gemm_ref.Padded``
  allocation with NaN sentinels in its row padding and guard elements.  ALL THREE outputs (out, k_out, vT_out) are always allocated and handed
  over: after a successful call the inputs are unchanged bit for bit, the outputs the mode writes have their padding intact and the outputs
  it does not write (k_out for a kv-split with N = 128, out for any kv-split, k_out / vT_out otherwise) are untouched altogether; after a
  refused call every output is untouched.
* ``exact_case``: ``gemm_ref.exact_case`` in the decoder's type - integer operands in [-3, 3], integer bias / table / residual, every partial
  sum an exact integer in any accumulation order, bias magnitudes that put the results above ``THRESH16`` so that >= 25 % of them are inexact
  in the 16-bit type and >= 1 % exact ties (asserted by the generator on its own reference), and rows of A that are pairwise distinct
  across the whole M (asserted), so a swapped, stale or repeated tile changes the result.
* ``ln_case``: exact integer pre-activations of moderate size for the LayerNorm epilogues, with one row whose pre-activation is the same
  integer in every column (variance 0) and pairwise distinct ``ln_w`` / ``ln_b`` entries.
* ``expected`` turns a case into the outputs of its launch (out / k / vT / the head-major layout).  Its ``defect`` argument gives what a
  subtly wrong kernel would write - tests/test_wsgemm_host.py shows that each one breaks bit equality on the generators' cases:
    tile_stride_off       tile t computed from the rows of A of tile t + grid (the persistent loop's stride applied once too often)
    stale_tile            tile t computed from the rows of A of tile t - grid (the LDS buffer not flipped / the pending set not stored)
    last_tile_clamped     the prefetch index clamped one tile early: tile ntiles - 2 computed from the rows of A of tile ntiles - 1
    table_row_off         table row (row + 1) % table_rows
    table_col_le4         the table added up to the next multiple of 4 above table_cols, read past the end of each table row (what the
                          kernel did before table_cols % 4 != 0 was refused; past the allocation the model reads +inf)
    resid_nowrap          ``row % resid_rows`` ignored (clamped to the last residual row)
    vt_untransposed       the vT block written [tokens, 128]
    head_batch_per_tile   head-major: the image index taken from the tile's first row instead of per row
    ln64_index_unwrapped  ln_mode 2: ``ln_w[c]`` instead of ``ln_w[c & 63]`` (columns from 64 on read the guard NaNs behind the vector)
    truncate, double_round  ``gemm_ref.rne16``'s rounding defects"""
import ctypes as C
import functools

import torch

import gemm_ref as G
from gemm_ref import THRESH16, Padded, assert_bits, bits, rne16, same_bits  # noqa: F401  (re-exported for the test files)

WM = 32                  # csrc/wsgemm.hip: rows per tile
GRID = 512               # ... and the most workgroups a launch starts: M / 32 tiles above it make the persistent loop iterate
TILE_DEFECTS = ("tile_stride_off", "stale_tile", "last_tile_clamped")
DEFECTS = TILE_DEFECTS + ("table_row_off", "table_col_le4", "resid_nowrap", "vt_untransposed", "head_batch_per_tile", "ln64_index_unwrapped",
                          "truncate", "double_round")


def d16():
    from micro_sam_amd import _lib
    return _lib.decoder_dtype()


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch

def call(dev, c, *, expect_ok=True, table_cols=None, table_ld=None, table_rows=None, ldr=None, ldc=None, inplace=False, kv_split=0, tokens=0,
         head_major=0, ln_mode=0, ln_eps=1e-5, null=(), M=None, N=None, K=None):
    """One ``msam_wsgemm_bf16`` launch of case ``c`` (A, W and whichever of bias / table / resid / ln_w / ln_b it holds).  ``M`` / ``N`` /
    ``K`` override what is handed over (the buffers keep the case's sizes), ``null`` names pointer fields to leave NULL.  Returns a dict:
    status, error, and clones of the logical outputs - out ([M, N], or [M / tokens, N / 16, tokens, 16] head-major), k [M, 128],
    vT [M / tokens, 128, tokens]."""
    from micro_sam_amd import _lib
    d = d16()
    Mc, Nc, Kc = c["M"], c["N"], c["K"]
    assert c["A"].dtype == d and c["W"].dtype == d, "the case was generated for another decoder type"
    p = _lib.WsGemmParams()
    inputs, outputs = [], {}

    def keep(buf):
        inputs.append(buf)
        return buf.ptr()

    def vec(name):
        return keep(Padded(1, c[name].numel(), c[name].numel(), c[name].dtype, dev, c[name].reshape(1, -1))) if name in c and name not in null else None
    p.A, p.W = keep(Padded(Mc, Kc, Kc, d, dev, c["A"])), keep(Padded(Nc, Kc, Kc, d, dev, c["W"]))
    p.M, p.N, p.K = (Mc if M is None else M), (Nc if N is None else N), (Kc if K is None else K)
    p.bias = vec("bias")
    if "table" in c:
        tr, tc = c["table"].shape
        ld = tc + 4 if table_ld is None else table_ld
        p.table, p.table_ld = keep(Padded(tr, tc, ld, torch.float32, dev, c["table"])), ld
        p.table_rows, p.table_cols = (tr if table_rows is None else table_rows), (tc if table_cols is None else table_cols)
    ldc = Nc + 4 if ldc is None else ldc
    if inplace:
        assert "resid" in c and not c.get("resid_rows") and not head_major and not kv_split
        out = Padded(Mc, Nc, ldc, d, dev, c["resid"])
        p.resid, p.resid_rows, p.ldr = out.ptr(), 0, ldc
    else:
        out = Padded(1, Mc * Nc, 0, d, dev) if head_major else Padded(Mc, Nc, ldc, d, dev)
        if "resid" in c:
            ldr = Nc + 8 if ldr is None else ldr
            p.resid = keep(Padded(c["resid"].shape[0], Nc, ldr, d, dev, c["resid"]))
            p.resid_rows, p.ldr = c.get("resid_rows", 0), ldr
    outputs = {"out": out, "k": Padded(Mc, 128, 128, d, dev), "vT": Padded(1, Mc * 128, 0, d, dev)}
    p.out, p.k_out, p.vT_out = (None if nm in null else outputs[o].ptr() for nm, o in (("out", "out"), ("k_out", "k"), ("vT_out", "vT")))
    p.ldc, p.kv_split, p.tokens, p.head_major = ldc, kv_split, tokens, head_major
    p.ln_mode, p.ln_eps, p.ln_w, p.ln_b = ln_mode, ln_eps, vec("ln_w"), vec("ln_b")

    status = _lib.load().msam_wsgemm_bf16(C.byref(p), _lib.stream_ptr())
    if dev.type == "cuda":
        torch.cuda.synchronize()
    res = {"status": status, "error": _lib.load().msam_last_error().decode("utf-8", "replace") if status else ""}
    what = f"msam_wsgemm_bf16 M={p.M} N={p.N} K={p.K}"
    for i, b in enumerate(inputs):
        assert b.unchanged(), f"{what}: input buffer {i} (or its padding) was written"
    written = set() if status else ({"vT"} | ({"k"} if p.N == 256 else set()) if kv_split else {"out"})
    for nm, o in outputs.items():
        if nm in written:
            assert o.padding_intact(), f"{what}: output {nm}: padding or guard elements were written"
        else:
            assert o.unchanged(), f"{what}: status {status}, but output {nm}, which this call does not write, was written"
    if expect_ok:
        assert status == 0, (status, res["error"])
    if status == 0:
        for nm in written:
            res[nm] = outputs[nm].logical()
        if head_major:
            res["out"] = res["out"].reshape(Mc // tokens, Nc // 16, tokens, 16)
        if kv_split:
            res["vT"] = res["vT"].reshape(Mc // tokens, 128, tokens)
    return res


def launches(fn):
    """(fn's result, number of launches the library's profile recorded while it ran: 0 or 1)."""
    out, fam = G.route_taken(fn)
    assert fam in (None, 1), f"family {fam} is not the decoder-stream family"
    return out, 0 if fam is None else 1


# ---------------------------------------------------------------------------------------------------------------------------------
# generators

@functools.lru_cache(maxsize=3)
def _exact(M, N, K, seed, table, table_rows, resid, resid_rows, d, devtype):
    c = G.exact_case(M, N, K, d, seed, out_dtype=d, table=table, table_rows=table_rows, resid=d if resid else None, resid_rows=resid_rows,
                     dev=torch.device(devtype))
    a = c["A"].float()
    assert torch.unique(a, dim=0).shape[0] == M, "exact_case: rows of A repeat somewhere in M - choose another seed"
    return c


def exact_case(M, N, K, seed, *, table=None, table_rows=7, resid=False, resid_rows=0, dev=None):
    """Integer case in the decoder's type (module docstring).  ``table`` = table_cols or None; ``resid``: a residual of ``resid_rows or M``
    rows.  A dict of CPU tensors plus 'ref', the exact float64 pre-activation [M, N] on ``dev``.  The last few cases are kept: the tests
    that share one compute it once - treat it as read-only."""
    return _exact(M, N, K, seed, table, table_rows, bool(resid), resid_rows, d16(), (dev or torch.device("cpu")).type)


def ln_case(M, N, K, seed, mode, *, resid_rows=0, const_row=37, dev=None):
    """LayerNorm input without error: integer operands and residual, an integer bias in [-50, 50] (|pre-activation| of a few hundred, so the
    normalised values spread over several binades of the 16-bit type).  Row ``const_row`` of A is zero and its residual row is 7 - bias:
    its pre-activation is 7 in every column, variance exactly 0.  ``ln_w`` in (0.25, 1.75] and ``ln_b`` in [-1, 1) have pairwise distinct
    entries (N of them for mode 1, 64 for mode 2)."""
    d = d16()
    c = dict(G.exact_case(M, N, K, d, seed, out_dtype=d, bias=False, resid=d, resid_rows=resid_rows, check_shares=False))
    g = torch.Generator().manual_seed(seed + 1)
    c["bias"] = torch.randint(-50, 51, (N,), generator=g).float()
    c["A"], c["resid"] = c["A"].clone(), c["resid"].clone()
    c["A"][const_row] = 0
    c["resid"][const_row % c["resid"].shape[0]] = (7 - c["bias"]).to(d)
    assert torch.unique(c["A"].float(), dim=0).shape[0] == M
    n = N if mode == 1 else 64
    c["ln_w"] = (0.25 + 1.5 * (torch.randperm(n, generator=g) + 1).float() / n)
    c["ln_b"] = ((torch.randperm(n, generator=g).float() - n / 2) * (2.0 / n))
    assert torch.unique(c["ln_w"]).numel() == n and torch.unique(c["ln_b"]).numel() == n
    c["ref"] = G.preact64(c, dev)
    assert bool((c["ref"] == c["ref"].round()).all()) and bool((c["ref"][const_row] == 7).all())
    c["const_row"] = const_row
    return c


def random_case(M, N, K, seed, *, table=None, table_rows=7, resid=False, resid_rows=0, dev=None):
    """``gemm_ref.random_case`` in the decoder's type: Gaussian operands, fp32 bias / table, 16-bit residual."""
    d = d16()
    return G.random_case(M, N, K, d, seed, table=table, table_rows=table_rows, resid=d if resid else None, resid_rows=resid_rows, out_dtype=d,
                         dev=dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# references

def _tile_source(M, defect, grid):
    """Row of A that each output row is computed from under a tile defect of the persistent loop."""
    nt = M // WM
    t = torch.arange(nt)
    if defect == "tile_stride_off":
        assert nt > grid, "no workgroup has a second tile at this M"
        s = torch.where(t + grid < nt, t + grid, t)
    elif defect == "stale_tile":
        assert nt > grid, "no workgroup has a second tile at this M"
        s = torch.where(t >= grid, t - grid, t)
    else:
        s = t.clone()
        s[nt - 2] = nt - 1
    return (s[:, None] * WM + torch.arange(WM)[None, :]).reshape(-1)


def preact64(c, dev=None, defect=None, grid=GRID):
    """float64 A W^T + bias + table + residual of a case (exact for the integer cases); ``defect``: module docstring."""
    if defect is None and "ref" in c:                          # the generator computed it already
        return c["ref"].to(dev or c["ref"].device).clone()
    if defect in TILE_DEFECTS:
        c = dict(c, A=c["A"][_tile_source(c["M"], defect, grid)])
    v = G.preact64(c, dev, defect if defect in ("table_row_off", "resid_nowrap") else None)
    if defect == "table_col_le4":
        t = c["table"].double()
        tr, tc = t.shape
        up = -(-tc // 4) * 4
        assert up > tc, "table_cols is a multiple of 4: the defect does not show"
        flat = torch.cat([t.reshape(-1), torch.full((up - tc,), float("inf"), dtype=torch.float64)]).to(v.device)
        rows = torch.arange(c["M"], device=v.device) % tr
        v[:, tc:up] += flat[rows[:, None] * tc + torch.arange(tc, up, device=v.device)[None, :]]
    return v


def layernorm64(pre, ln_w, ln_b, eps, mode, defect=None):
    """float64 LayerNorm over the row (mode 1) or over each group of 64 columns followed by the exact erf-GELU (mode 2)."""
    M, N = pre.shape
    n = N if mode == 1 else 64
    x = pre.reshape(M, N // n, n)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = ((x - mu) / torch.sqrt(var + eps) * ln_w.to(pre.device).double() + ln_b.to(pre.device).double()).reshape(M, N)
    if defect == "ln64_index_unwrapped":
        assert mode == 2
        y[:, 64:] = float("nan")
    return G.gelu64(y) if mode == 2 else y


def result64(c, dev=None, *, ln_mode=0, ln_eps=1e-5, defect=None, grid=GRID):
    """The float64 value of every output element before the 16-bit cast, [M, N]."""
    v = preact64(c, dev, defect, grid)
    return layernorm64(v, c["ln_w"], c["ln_b"], ln_eps, ln_mode, defect) if ln_mode else v


def expected(c, dev=None, *, kv_split=0, tokens=0, head_major=0, ln_mode=0, ln_eps=1e-5, defect=None, grid=GRID):
    """The outputs of a launch of case ``c`` as ``call`` returns them: {'out'} (plain or head-major), {'vT'} or {'k', 'vT'}."""
    d = d16()
    M, N = c["M"], c["N"]
    o = rne16(result64(c, dev, ln_mode=ln_mode, ln_eps=ln_eps, defect=defect, grid=grid).float(), d,
              defect if defect in ("truncate", "double_round") else None)
    if kv_split:
        B = M // tokens
        vv = (o[:, 128:] if N == 256 else o).reshape(B, tokens, 128)
        res = {"vT": (vv.reshape(B, 128, tokens) if defect == "vt_untransposed" else vv.permute(0, 2, 1)).contiguous()}
        if N == 256:
            res["k"] = o[:, :128].contiguous()
        return res
    if head_major:
        B, Hn = M // tokens, N // 16
        if defect != "head_batch_per_tile":
            return {"out": o.reshape(B, tokens, Hn, 16).permute(0, 2, 1, 3).contiguous()}
        rows, cols = torch.arange(M, device=o.device), torch.arange(N, device=o.device)
        b = (rows // WM * WM) // tokens
        t = rows - b * tokens                                   # reaches past `tokens` where an image ends inside a tile
        idx = ((b[:, None] * Hn + cols[None, :] // 16) * tokens + t[:, None]) * 16 + cols[None, :] % 16
        flat = torch.zeros(M * N, dtype=d, device=o.device)
        ok = idx < M * N
        flat[idx[ok]] = o[ok]
        return {"out": flat.reshape(B, Hn, tokens, 16)}
    return {"out": o}


def half_ulp(ref64, d):
    """Half a unit in the last place of the 16-bit type ``d`` at |ref| (subnormal spacing below the smallest normal number)."""
    mant, emin = (10, -14) if d == torch.float16 else (7, -126)
    e = torch.frexp(ref64.abs().clamp(min=2.0 ** emin))[1].double() - 1        # floor(log2 |ref|)
    return torch.exp2(e.clamp(min=emin) - mant - 1)


def ln_bound(ref64, mode, d):
    """The project's LayerNorm bound (tests/test_gpu_ops_boundary.py: 2e-5 + 1e-5 |ref|; through the GELU slope 1.13 plus the 5.5e-5 design
    error of ``gelu_erf``) plus half a unit in the last place of the decoder type, 2^-11 |ref| (fp16) or 2^-8 |ref| (bf16)."""
    h = 2.0 ** -11 if d == torch.float16 else 2.0 ** -8
    if mode == 2:
        return 1.13 * 2e-5 + 5.5e-5 + (1.13 * 1e-5 + h) * ref64.abs()
    return 2e-5 + (1e-5 + h) * ref64.abs()


def gauss_bound(c, dev, d):
    """(K + 3) 2^-24 (|A| |W|^T + |bias| + |table| + |resid|): K products' sums and three epilogue additions in fp32 in any order (the products
    of two 16-bit numbers are exact in fp32), plus half a unit in the last place of the decoder type at |ref|."""
    mags = dict(c)
    for k in ("A", "W", "bias", "table", "resid"):
        if k in c:
            mags[k] = c[k].abs()
    return (c["K"] + 3) * 2.0 ** -24 * G.preact64(mags, dev) + half_ulp(c["ref"].to(dev) if dev is not None else c["ref"], d)


def share_off(got, ref64):
    """Share of the elements that are NOT the round-to-nearest-even cast of the float64 reference (a figure, not a check: the half unit in
    the last place dominates every bound above, so err / bound alone says little about the fp32 arithmetic in front of the cast)."""
    return float((bits(got) != bits(rne16(ref64.float(), got.dtype))).float().mean())


def max_ratio(got, ref64, bound):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref64).abs() / bound).max())
