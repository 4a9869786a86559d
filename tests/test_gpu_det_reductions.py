"""The fixed-order reductions of fine-tuning's parameter gradients on the device (csrc/train.hip ``msam_det_reduce`` /
``msam_det_reduce_tree``): the ``msam_cast_transpose`` column sums (parts = ceil(M / 64)), the ``msam_layernorm_backward`` parameter
gradients (parts = min(ceil(rows / 4), 2048)) and split-K ``msam_gemm_bf16`` (parts = split_k).  The tree adds groups of 32 parts per
level, alternating between the two halves of a shared workspace, until at most 32 parts are left; the part counts here cross those
thresholds (1, 32, 33, 1024, 1025, 2048, 65 535 parts: up to three levels).

Exact where possible: with small integers every fp32 partial sum is exact in any order while the totals stay below 2^24, and a bf16 x bf16
product is exact in fp32.  So the column sums, ``dbias`` and the split-K product must EQUAL the float64 reference bit for bit: a part that
is dropped, counted twice or read from the wrong half cannot hide behind a tolerance.  Elsewhere (random data; ``dweight`` and ``dx``,
which have no exact form) the error is held to a rigorous bound: |got - ref64| <= gamma_d * sum |terms| for a sum of depth d, with
gamma_d = d u / (1 - d u), u = 2^-24, and first-order propagation of the per-row rounding errors for the LayerNorm quantities."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXACT = 2 ** 24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _gamma(d):
    return d * U / (1 - d * U)


def _tree(parts):
    """(levels, parts left for the final pass) of msam_det_reduce_tree."""
    levels = 0
    while parts > 32:
        parts, levels = (parts + 31) // 32, levels + 1
    return levels, parts


def _cast_transpose(x, colsum, want16=False, want_t=False):
    """msam_cast_transpose with the caller's column-sum buffer (ops.cast_transpose always starts from zeros): colsum += x.sum(0)."""
    from micro_sam_amd import _lib
    M, K = x.shape
    o16 = torch.empty((M, K), dtype=torch.bfloat16, device=x.device) if want16 else None
    oT = torch.empty((K, M), dtype=torch.bfloat16, device=x.device) if want_t else None
    _lib.check(_lib.load().msam_cast_transpose(x.data_ptr(), _lib.F32 if x.dtype == torch.float32 else _lib.BF16, M, K, x.stride(0),
                                               _lib.ptr(o16), _lib.ptr(oT), colsum.data_ptr(), _lib.stream_ptr()), "msam_cast_transpose")
    return o16, oT


def _ln_backward(x, w, dy, eps, dw, db):
    """msam_layernorm_backward: returns dx; dw / db += the parameter gradients."""
    from micro_sam_amd import _lib
    rows, dim = x.shape
    dx = torch.empty_like(x)
    _lib.check(_lib.load().msam_layernorm_backward(x.data_ptr(), w.data_ptr(), dy.data_ptr(), float(eps), rows, dim, dx.data_ptr(),
                                                   dw.data_ptr(), db.data_ptr(), _lib.stream_ptr()), "msam_layernorm_backward")
    return dx


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ---- msam_cast_transpose column sums

CT_M = [1, 2048, 2049, 65536, 65537, 4194240]       # 1, 32, 33, 1024, 1025, 65 535 parts


@pytest.mark.parametrize("src", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", CT_M)
def test_cast_transpose_column_sums_exact_on_integers(dev, M, src):
    K = 4 if M >= 65536 else 68                       # small K for the large M; 68: a partial second 64-column tile
    g = torch.Generator().manual_seed(M + K)
    x = torch.randint(-2, 3, (M, K), generator=g).to(src)
    init = torch.randint(-1000, 1001, (K,), generator=g).float()
    ref = init.double() + x.double().sum(0)
    assert float(init.abs().max()) + float(x.double().abs().sum(0).max()) < EXACT       # every partial sum is exact
    xd = x.to(dev)
    cs = init.to(dev)
    o16, oT = _cast_transpose(xd, cs, want16=True, want_t=True)
    assert torch.equal(cs.cpu().double(), ref), (M, src, _tree((M + 63) // 64))
    assert torch.equal(o16, xd.to(torch.bfloat16)) and torch.equal(oT, xd.to(torch.bfloat16).t().contiguous())
    cs2 = init.to(dev)
    _cast_transpose(xd, cs2)                          # the column sums alone: the same bits
    assert torch.equal(cs2, cs)


@pytest.mark.parametrize("M", CT_M)
def test_cast_transpose_column_sums_bounded_on_random_data(dev, M):
    K = 8 if M >= 65536 else 68
    g = torch.Generator().manual_seed(7 * M + 1)
    x = torch.randn(M, K, generator=g) * 3 + 1
    init = torch.randn(K, generator=g) * 100
    ref = init.double() + x.double().sum(0)
    levels, last = _tree((M + 63) // 64)
    depth = 4 + 16 + 32 * levels + last + 1           # 4 rows per thread, 16 row groups, 32 per tree level, init + the last parts
    bound = _gamma(depth) * (init.double().abs() + x.double().abs().sum(0))
    cs = init.to(dev)
    _cast_transpose(x.to(dev), cs)
    err = (cs.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), (M, float((err / bound).max()))


# ---- msam_layernorm_backward parameter gradients

def _ln_reference(x, w, dy, eps, dw0, db0):
    """float64 LayerNorm backward and first-order bounds of the kernel's fp32 evaluation (one wave per row: V = dim / 64 values per lane,
    then a 6-level butterfly; per-wave chains over the rows of a workgroup, 4 waves, the tree, the final pass onto dw0 / db0)."""
    rows, n = x.shape
    h = n // 64 + 6
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    xa = x64.abs().mean(1, keepdim=True)
    mu = x64.mean(1, keepdim=True)
    xc = x64 - mu
    var = (xc * xc).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xhat = xc * r
    g = dy64 * w64
    mg = g.mean(1, keepdim=True)
    gx = g * xhat
    mgx = gx.mean(1, keepdim=True)
    dx = r * (g - mg - xhat * mgx)
    dw = dw0.double() + (dy64 * xhat).sum(0)
    db = db0.double() + dy64.sum(0)
    # rounding of the row statistics: the sums (depth h), the products with the rounded 1 / dim, + eps, sqrt, division
    d_mu = _gamma(h + 2) * xa
    d_xc = d_mu + U * xc.abs()
    del xa
    d_var = _gamma(h + 2) * var + 2 * (xc.abs() * d_xc).mean(1, keepdim=True)
    eps_r = 0.5 * d_var / (var + eps) + _gamma(3)
    d_xhat = r * d_xc + xhat.abs() * (eps_r + U)
    del d_xc, xc
    grid = min((rows + 3) // 4, 2048)
    levels, last = _tree(grid)
    chain = (rows + 4 * grid - 1) // (4 * grid)       # rows per wave
    depth = chain + 1 + 3 + 32 * levels + last + 1    # the product, the per-wave chain, 4 waves, the tree, dw0 + the last parts
    b_dw = 2 * (_gamma(depth) * (dw0.double().abs() + (dy64 * xhat).abs().sum(0)) + (dy64.abs() * d_xhat).sum(0))
    d_g = U * g.abs()
    d_mg = _gamma(h + 2) * g.abs().mean(1, keepdim=True)
    d_mgx = _gamma(h + 3) * gx.abs().mean(1, keepdim=True) + ((g.abs() * d_xhat) + xhat.abs() * d_g).mean(1, keepdim=True)
    d_t = d_g + d_mg + xhat.abs() * d_mgx + mgx.abs() * d_xhat + _gamma(3) * (g.abs() + mg.abs() + (xhat * mgx).abs())
    b_dx = 2 * (r * d_t + dx.abs() * (eps_r + U))     # (x 2: room for the second-order terms)
    return dx, dw, db, b_dx, b_dw


LN_ROWS = [1, 4, 128, 129, 4096, 4097, 8192, 100000]     # 1, 1, 32, 33, 1024, 1025, 2048, 2048 parts
LN_DIMS = [64, 256, 768, 1280]


@pytest.mark.parametrize("dim", LN_DIMS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_backward_dbias_exact_dweight_dx_bounded(dev, rows, dim):
    """Integer dy: dbias (accumulated onto a non-zero integer start) equals the float64 sum bit for bit; dweight (onto a non-zero start)
    and dx hold the rigorous bound; through training.functional.layer_norm (zero start) the same bits as the raw call."""
    from micro_sam_amd.training import functional as HF
    g = torch.Generator().manual_seed(rows * 7 + dim)
    x = (torch.randn(rows, dim, generator=g) * 2 + 0.5).to(dev)
    w = (torch.randn(dim, generator=g) * 0.3 + 1).to(dev)
    dy = torch.randint(-4, 5, (rows, dim), generator=g).float().to(dev)
    dw0 = (torch.randn(dim, generator=g) * 10).to(dev)
    db0 = torch.randint(-500, 501, (dim,), generator=g).float().to(dev)
    eps = 1e-6
    dw, db = dw0.clone(), db0.clone()
    dx = _ln_backward(x, w, dy, eps, dw, db)
    ref_dx, ref_dw, ref_db, b_dx, b_dw = _ln_reference(x, w, dy, eps, dw0, db0)
    assert float(db0.abs().max()) + float(dy.abs().sum(0).max()) < EXACT
    assert torch.equal(db.double(), ref_db), (rows, dim, float((db.double() - ref_db).abs().max()))
    e_dw = (dw.double() - ref_dw).abs()
    assert bool((e_dw <= b_dw).all()), (rows, dim, float((e_dw / b_dw).max()))
    e_dx = (dx.double() - ref_dx).abs()
    assert bool((e_dx <= b_dx).all()), (rows, dim, float((e_dx / b_dx).max()))
    del ref_dx, b_dx, e_dx
    # the autograd function: zero start, the same reduction - the raw call from zeros gives the same bits
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    br = torch.zeros(dim, device=dev, requires_grad=True)
    HF.layer_norm(xr, wr, br, eps).backward(dy)
    dwz, dbz = torch.zeros(dim, device=dev), torch.zeros(dim, device=dev)
    dxz = _ln_backward(x, w, dy, eps, dwz, dbz)
    assert torch.equal(wr.grad, dwz) and torch.equal(br.grad, dbz) and torch.equal(xr.grad, dxz) and torch.equal(dxz, dx)


# ---- split-K msam_gemm_bf16

SPLITS = [2, 32, 33, 64]


@pytest.mark.parametrize("split", SPLITS)
def test_split_k_gemm_exact_on_integers(dev, split):
    from micro_sam_amd import ops
    M, N, K = 200, 256, 64 * split * 4
    g = torch.Generator().manual_seed(split)
    a = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    w = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16)
    ref = a.double() @ w.double().t()
    assert float((a.double().abs() @ w.double().abs().t()).max()) < EXACT
    ad, wd = a.to(dev), w.to(dev)
    out = torch.full((M, N), float("nan"), device=dev)          # split-K overwrites its output
    got = ops.gemm(ad, wd, None, out_dtype=torch.float32, split_k=split, out=out)
    assert torch.equal(got.cpu().double(), ref), (split, _tree(split), float((got.cpu().double() - ref).abs().max()))
    assert torch.equal(ops.gemm(ad, wd, None, out_dtype=torch.float32), got)        # the plain product: also exact
    assert torch.equal(ops.gemm(ad, wd, None, out_dtype=torch.float32, split_k=split), got)


# ---- results do not depend on earlier calls of other sizes (they grow the workspaces; all three share the tree's slot)

def test_results_do_not_depend_on_earlier_calls(dev):
    from micro_sam_amd import ops
    g = torch.Generator().manual_seed(99)
    ct_x = (torch.randn(65537, 8, generator=g) * 3).to(dev)
    ct_init = torch.randn(8, generator=g).to(dev)
    ln_x, ln_dy = torch.randn(4097, 256, generator=g).to(dev), torch.randn(4097, 256, generator=g).to(dev)
    ln_w = (torch.randn(256, generator=g) * 0.3 + 1).to(dev)
    gm_a = torch.randn(200, 64 * 33 * 2, generator=g).to(torch.bfloat16).to(dev)
    gm_w = torch.randn(256, 64 * 33 * 2, generator=g).to(torch.bfloat16).to(dev)

    def ct():
        cs = ct_init.clone()
        _cast_transpose(ct_x, cs)
        return [cs]

    def ln():
        dw, db = torch.ones(256, device=dev), torch.ones(256, device=dev)
        return [_ln_backward(ln_x, ln_w, ln_dy, 1e-6, dw, db), dw, db]

    def gm():
        return [ops.gemm(gm_a, gm_w, None, out_dtype=torch.float32, split_k=33)]

    def big_ct():
        cs = torch.zeros(8, device=dev)
        _cast_transpose(torch.randn(4194240, 8, device=dev), cs)

    def big_ln():
        _ln_backward(torch.randn(100000, 1280, device=dev), torch.ones(1280, device=dev), torch.randn(100000, 1280, device=dev), 1e-6,
                     torch.zeros(1280, device=dev), torch.zeros(1280, device=dev))

    def big_gm():
        ops.gemm(torch.randn(512, 64 * 64 * 4, device=dev).to(torch.bfloat16), torch.randn(512, 64 * 64 * 4, device=dev).to(torch.bfloat16),
                 None, out_dtype=torch.float32, split_k=64)

    def small_ct():                                    # a call without the tree after the large ones
        cs = torch.zeros(8, device=dev)
        _cast_transpose(torch.randn(100, 8, device=dev), cs)

    want = {"ct": [_bits(t) for t in ct()], "ln": [_bits(t) for t in ln()], "gm": [_bits(t) for t in gm()]}
    run = {"ct": ct, "ln": ln, "gm": gm}
    for grow, check in ((big_ct, "ln"), (big_gm, "ct"), (big_ln, "gm"), (small_ct, "ln"), (big_ln, "ct"), (big_ct, "gm"), (None, "ct"),
                        (None, "ln"), (None, "gm")):
        if grow is not None:
            grow()
        got = [_bits(t) for t in run[check]()]
        assert all(torch.equal(a, b) for a, b in zip(got, want[check])), (getattr(grow, "__name__", None), check)
