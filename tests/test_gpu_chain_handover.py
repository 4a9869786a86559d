"""Hand-over between the two chained decoder kernels (csrc/decfold_tok.hip, include/msam_hip.h msam_chain_handover_bytes).

Both kernels compute the same layer-0 image->token block for every (prompt, 16-token tile).  With the hand-over the attention kernel
(msam_i2t0_t2i_fused_v2_handover) stores the block's packed softmax probabilities and LayerNorm statistics per tile, and the stream
kernel (msam_i2t01_fused_handover) reads them instead of computing them again.  The values handed over are the registers the
producer holds anyway and the consumer's remaining arithmetic is unchanged, so everything is compared BIT FOR BIT with the pair
without hand-over:

  * kernel level, (P, Nt) in (3, 5), (129, 8), (300, 7): P = 300 exceeds the 256-workgroup grid (prompt-stride loop with unequal trip
    counts), Nt = 5 has padded token slots, P = 129 is an odd count just above the 128-prompt chain threshold; every ring depth of the
    stream kernel;
  * the contents of the buffer: probabilities of the used slots of a (token, head) sum to 1, padded slots are exactly 0;
  * a buffer poisoned with NaN patterns: every slot is written before it is read;
  * the decoder with msam_tune_set "chain_handover" 0 and 1;
  * without a GPU: the decoder workspace grows by exactly the buffer, and a workspace one byte short is refused before any launch.

The inputs are built the way tests/test_gpu_kernels.py::_chained_layer0_case builds them; each case is built once and shared."""
import ctypes as C
import math

import pytest
import torch

from test_gpu_decoder_routes import _decode, ctx  # noqa: F401  (ctx: the module fixture of the decoder-route tests, instantiated for this module)

T = 4096
HAND_TILE = 2 * 1024 + 16 * 8                     # per (prompt, tile): pk[0], pk[1] (64 lanes x 16 B each), 16 x (rstd, -mean rstd)
CASES = [(3, 5), (129, 8), (300, 7)]
RINGS = (3, 2)                                    # msam_tune_set "chain_handover_ring"
RING_DEFAULT = 3
_built = {}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import ops
    return ops, torch.device("cuda")


def _ddt():
    from micro_sam_amd import _lib
    return _lib.decoder_dtype()


def _case(env, P, Nt):
    """Operands of both chained kernels and the results of the pair WITHOUT hand-over (the reference; computed once, never changed)."""
    if (P, Nt) in _built:
        return _built[(P, Nt)]
    ops, dev = env
    d16 = _ddt()
    g = torch.Generator().manual_seed(300 + P)
    src = torch.randn(T, 256, generator=g).to(d16).to(dev)
    pe = torch.randn(T, 256, generator=g).to(dev)

    def layer():
        wq = (torch.randn(128, 256, generator=g) / 16).to(d16).to(dev); bq = torch.randn(128, generator=g).to(dev)
        wo = (torch.randn(256, 128, generator=g) / math.sqrt(128)).to(d16).to(dev); bo = torch.randn(256, generator=g).to(dev)
        lw = (torch.randn(256, generator=g) * 0.2 + 1).to(dev); lb = torch.randn(256, generator=g).to(dev)
        ktok = torch.randn(P, Nt, 128, generator=g).to(d16).to(dev); vtok = torch.randn(P, Nt, 128, generator=g).to(d16).to(dev)
        tabq = (pe @ wq.float().t() + bq).to(d16)
        return dict(wq=wq, wo=wo, bo=bo, lw=lw, lb=lb, ktok=ktok, vtok=vtok, tabq=tabq)

    L0, L1 = layer(), layer()
    q0 = (src.float() @ L0["wq"].float().t() + L0["tabq"].float()).to(d16)
    op0 = ops.i2t_fold_operands(L0["ktok"], L0["vtok"], L0["wq"], L0["wo"], L0["bo"], with_kfold=False)
    op1 = ops.i2t_fold_operands(L1["ktok"], L1["vtok"], L1["wq"], L1["wo"], L1["bo"])
    wk = (torch.randn(128, 256, generator=g) / 16).to(d16).to(dev); bk = torch.randn(128, generator=g).to(dev)
    tabk = (pe @ wk.float().t() + bk).to(d16)
    tables = ops.chain_prepare_tables(src, q0, tabk, L1["tabq"])
    wv = (torch.randn(128, 256, generator=g) / 16).to(d16).to(dev); bv = torch.randn(128, generator=g).to(dev)
    qtok = (torch.randn(P, Nt, 128, generator=g) * 1.5).to(d16).to(dev)
    t2 = ops.chain_prepare_tables2(src, wv, bv, wk, L0["lw"], L0["lb"], L0["wo"], L0["bo"])
    mf = ops.t2i_fold_values(L0["vtok"], t2)
    c = dict(P=P, Nt=Nt, L0=L0, L1=L1, op0=op0, op1=op1, tables=tables, t2=t2, mf=mf, qtok=qtok, wk=wk)
    c["att_ref"] = ops.i2t0_t2i_fused_v2(tables, t2, op0, mf, L0["lw"], qtok, wk)
    c["out_ref"] = ops.i2t01_fused(tables, op0, L0["lw"], L0["lb"], op1, L1["lw"], L1["lb"], P, Nt)
    _built[(P, Nt)] = c
    return c


def _produce(ops, c, hand):
    return ops._i2t0_t2i_fused_v2_handover(c["tables"], c["t2"], c["op0"], c["mf"], c["L0"]["lw"], c["qtok"], c["wk"], hand)


def _consume(ops, c, hand, ring=RING_DEFAULT):
    from micro_sam_amd import _lib
    lib = _lib.load()
    L0, L1 = c["L0"], c["L1"]
    assert lib.msam_tune_set(b"chain_handover_ring", ring) == 0
    try:
        return ops._i2t01_fused_handover(c["tables"], c["op0"], L0["lw"], L0["lb"], c["op1"], L1["lw"], L1["lb"], c["P"], c["Nt"], hand)
    finally:
        lib.msam_tune_set(b"chain_handover_ring", RING_DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("P,Nt", CASES)
def test_handover_pair_is_bit_identical(env, P, Nt):
    ops, dev = env
    c = _case(env, P, Nt)
    hand = ops._chain_handover_buffer(P, dev)
    assert hand.numel() == P * 256 * HAND_TILE
    att = _produce(ops, c, hand)
    assert torch.equal(att, c["att_ref"])
    for ring in RINGS:
        out = _consume(ops, c, hand, ring)
        assert torch.equal(out, c["out_ref"]), f"ring depth {ring}"
        del out


@pytest.mark.gpu
@pytest.mark.parametrize("P,Nt", CASES)
def test_handover_contents(env, P, Nt):
    """pk[a2], lane 16 fg + fr, 16-bit value i = the probability of prompt token i for image token fr of the tile and head 4 a2 + fg."""
    ops, dev = env
    c = _case(env, P, Nt)
    hand = ops._chain_handover_buffer(P, dev)
    _produce(ops, c, hand)
    sel = [0, P // 2, P - 1]
    h = hand.view(P, 256, HAND_TILE)[sel]
    pk = h[:, :, :2048].contiguous().view(_ddt()).view(len(sel), 256, 2, 64, 8)
    # used slots: 8 roundings to the 16-bit type of values <= 1, at most a quarter of its epsilon each (fp16: 2^-12 each, 2^-9 in all)
    bound = 8 * torch.finfo(_ddt()).eps / 4
    assert _ddt() != torch.float16 or bound == 2.0 ** -9
    total = pk[..., :Nt].double().sum(-1)
    worst = float((total - 1).abs().max())
    print(f"P={P} Nt={Nt}: max |sum of the used slots - 1| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
    assert bool((pk[..., Nt:].contiguous().view(torch.int16) == 0).all()), "a padded slot is not exactly 0"
    stat = h[:, :, 2048:].contiguous().view(torch.float32).view(len(sel), 256, 16, 2)
    assert bool(torch.isfinite(stat).all()) and bool((stat[..., 0] > 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("P,Nt", CASES)
def test_every_slot_is_written_before_it_is_read(env, P, Nt):
    ops, dev = env
    c = _case(env, P, Nt)
    hand = ops._chain_handover_buffer(P, dev)
    hand.fill_(0xFF)                                  # NaN as 16-bit values and as fp32
    assert bool(torch.isnan(hand[:HAND_TILE].view(_ddt())).all()) and bool(torch.isnan(hand[:HAND_TILE].view(torch.float32)).all())
    att = _produce(ops, c, hand)
    out = _consume(ops, c, hand)
    assert torch.equal(att, c["att_ref"])
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, c["out_ref"])


@pytest.mark.gpu
def test_decoder_route_with_and_without_handover(ctx):  # noqa: F811
    from micro_sam_amd import _lib
    lib = _lib.load()
    res = {}
    try:
        for on in (0, 1):
            assert lib.msam_tune_set(b"chain_handover", on) == 0
            res[on] = _decode(ctx, "two_points", 130)
    finally:
        lib.msam_tune_set(b"chain_handover", 1)
    (low0, iou0), (low1, iou1) = res[0], res[1]
    assert low1.shape == (130, 3, 256, 256) and bool(torch.isfinite(low1).all())
    assert torch.equal(low1, low0) and torch.equal(iou1, iou0)


# ---- without a GPU: the library's argument checks run before any launch

def _align256(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("P", [1, 3, 130, 1024])
def test_decoder_workspace_grows_by_the_handover_buffer(P):
    from micro_sam_amd import _lib
    lib = _lib.load()
    assert lib.msam_chain_handover_bytes(P) == P * 256 * HAND_TILE
    # the carvings of decoder_run's workspace before the hand-over (csrc/decoder.hip work_bytes, Nt = 16), each rounded to 256 bytes
    M, R, Cc, CI = P * 16, P * T, 256, 128
    before = (3 * _align256(M * Cc * 4) + 6 * _align256(M * Cc * 2) + _align256(M * 2048 * 2) + _align256(R * Cc * 2)
              + 4 * _align256(R * CI * 2) + _align256(R * Cc * 2) + _align256(R * Cc * 4) + 2 * _align256(5 * P * Cc * 2)
              + _align256(P * 4 * 128 * 4) + _align256(P * 128 * 4))
    assert lib.msam_decoder_workspace_bytes(P) == before + _align256(P * 256 * HAND_TILE)


def test_workspace_one_byte_short_is_refused_before_any_launch():
    """10 points per prompt = 16 tokens, the count msam_decoder_workspace_bytes is sized for.  The check precedes every launch (and every
    read of the arguments): without a device a launch would fail with another error, here the call returns the argument error."""
    from micro_sam_amd import _lib
    lib = _lib.load()
    P, Np = 3, 10
    need = lib.msam_decoder_workspace_bytes(P)
    dec = _lib.DecoderParams()
    blob = (C.c_char * 4096)()
    addr = C.addressof(blob)
    args = (C.byref(dec), addr, addr, addr, addr, Np, None, P, 1, addr, addr, addr)
    assert lib.msam_decoder_forward(*args, need - 1, None) == 1
    assert b"workspace too small" in lib.msam_last_error()
