"""micro_sam_amd.visualization on the device against sklearn's PCA in float64 (tests/embedding_pca_ref.py).

Float output: max |device - ref64| / ptp(ref64) <= 4 r, r being the same figure of sklearn run on the float32 input (computed here on the
same input); uint8 output: within 1 of the float64 reference's and at most 0.5 % of the values different.  Every numeric case asserts
lambda3 / lambda4 >= 2 on its input first.  Each check prints its figures (pytest -s); profiles/r07_embedding_pca.md records them."""
import numpy as np
import pytest
import torch

import embedding_pca_ref as REF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def VIS():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import visualization
    return visualization


@pytest.fixture(scope="module")
def predictor(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd import util
    return util.get_sam_model("vit_b", device="cuda:0", state_dict=vit_b_sd)


def _embedding(shape):
    c, h, w = shape
    return REF.synthetic_embedding(c + h, c, h, w)[None]


@pytest.mark.parametrize("shape", REF.SHAPES)
def test_float_and_rgb_match_sklearn(VIS, shape):
    emb = _embedding(shape)
    dev = torch.from_numpy(emb).cuda()
    vis = VIS.compute_pca(dev, as_rgb=False)
    assert vis.is_cuda and tuple(vis.shape) == (shape[1], shape[2], 3) and vis.dtype == torch.float32
    REF.check_float(vis.cpu().numpy(), emb)
    rgb = VIS.compute_pca(dev)
    assert rgb.is_cuda and tuple(rgb.shape) == (shape[1], shape[2], 3) and rgb.dtype == torch.uint8
    REF.check_rgb(rgb.cpu().numpy(), emb)
    # a second call, and numpy input, agree bit for bit
    assert torch.equal(VIS.compute_pca(dev, as_rgb=False), vis) and torch.equal(VIS.compute_pca(dev), rgb)
    from_numpy = VIS.compute_pca(emb)
    assert isinstance(from_numpy, np.ndarray) and np.array_equal(from_numpy, rgb.cpu().numpy())


def test_moments_against_float64():
    """The kernels one by one on a ragged unit (C = 45, N = 700: masked channels and positions, more than one split) in a batch of two."""
    from micro_sam_amd import ops
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((2, 45, 700)) * 3 + rng.standard_normal((2, 45, 1)) * 5).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    mean, gram = ops.pca_moments(xd)
    x64 = x.astype(np.float64)
    mean_h = mean.cpu().numpy()
    m64 = x64.mean(axis=2)
    assert (np.abs(mean_h - m64) <= 2.0 ** -24 * np.abs(m64) * (1 + 1e-6)).all()             # the fp64 mean rounded once
    xc = x64 - mean_h.astype(np.float64)[:, :, None]
    g64 = np.einsum("ucn,udn->ucd", xc, xc)
    g = gram.cpu().numpy()
    assert np.array_equal(g, g.transpose(0, 2, 1))
    # fp32 rounding of the centred data (2^-24 relative per factor) and an fp32 chain of 64 terms: 66 * 2^-24 of sum |a| |b|
    diag = np.einsum("ucc->uc", g64)
    assert (np.abs(g - g64) <= 66 * 2.0 ** -24 * np.sqrt(diag[:, :, None] * diag[:, None, :])).all()
    again = ops.pca_moments(xd)
    assert torch.equal(again[0], mean) and torch.equal(again[1], gram)
    alone = ops.pca_moments(xd[1:])
    assert torch.equal(alone[0], mean[1:]) and torch.equal(alone[1], gram[1:])
    comp = rng.standard_normal((2, 5, 45)).astype(np.float32)
    out, minmax = ops.pca_project(xd, torch.from_numpy(comp).cuda(), mean)
    out_h = out.cpu().numpy()
    want = np.einsum("ukc,ucn->ukn", comp.astype(np.float64), xc)
    scale = np.einsum("ukc,ucn->ukn", np.abs(comp).astype(np.float64), np.abs(xc))
    assert (np.abs(out_h - want) <= 47 * 2.0 ** -24 * scale).all()
    assert np.array_equal(minmax.cpu().numpy(), np.stack([out_h.min(axis=(1, 2)), out_h.max(axis=(1, 2))], axis=1))
    rgb = ops.pca_to_rgb(out[:, :3].contiguous(), minmax)
    o, mn, mx = out_h[:, :3], minmax.cpu().numpy()[:, 0], minmax.cpu().numpy()[:, 1]
    want8 = ((np.float32(255) * (o - mn[:, None, None])) / (mx - mn)[:, None, None]).astype(np.uint8).transpose(0, 2, 1)
    assert np.array_equal(rgb.cpu().numpy(), want8)


def test_stack_slices_are_fitted_on_their_own(VIS):
    stack = np.stack([REF.synthetic_embedding(3, 256, 16, 16, noise_seed=z)[None] * np.float32(10.0 ** (z - 1)) for z in range(3)])
    for z in range(3):
        REF.assert_separated(stack[z, 0])
    dev = torch.from_numpy(stack).cuda()
    for as_rgb in (True, False):
        vis = VIS.compute_pca(dev, as_rgb=as_rgb)
        assert vis.is_cuda and tuple(vis.shape) == (3, 16, 16, 3) and vis.dtype == (torch.uint8 if as_rgb else torch.float32)
        for z in range(3):
            assert torch.equal(vis[z], VIS.compute_pca(dev[z], as_rgb=as_rgb))
    for z in range(3):
        REF.check_rgb(VIS.compute_pca(dev[z]).cpu().numpy(), stack[z], f"stack slice {z}")


def test_errors_and_degenerate_input(VIS):
    emb = torch.from_numpy(_embedding((20, 16, 24))).cuda()
    for bad in (emb[0], emb[None, None]):                               # ndim 3 and ndim 6
        with pytest.raises(ValueError):
            VIS.compute_pca(bad)
    with pytest.raises(ValueError):
        VIS.compute_pca(emb, n_components=2)
    with pytest.raises(ValueError):
        VIS.compute_pca(emb, n_components=9, as_rgb=False)
    with pytest.raises(ValueError):
        VIS.compute_pca(torch.zeros((1, 257, 4, 4), device="cuda"))
    with pytest.raises(ValueError):
        VIS.compute_pca(torch.zeros((1, 16, 2, 2), device="cuda"), n_components=5, as_rgb=False)
    with pytest.raises(TypeError):
        VIS.compute_pca(emb.to(torch.int32))
    with pytest.raises(TypeError):
        VIS.compute_pca(emb.cpu().numpy().astype(np.int64))
    const = VIS.compute_pca(torch.full((1, 20, 16, 24), 1.5, device="cuda"))
    assert const.dtype == torch.uint8 and tuple(const.shape) == (16, 24, 3) and not bool(const.any())
    assert tuple(VIS.compute_pca(emb, n_components=2, as_rgb=False).shape) == (16, 24, 2)
    assert tuple(VIS.compute_pca(emb, n_components=8, as_rgb=False).shape) == (16, 24, 8)


def test_ops_refuse_before_any_launch():
    from micro_sam_amd import ops
    x = torch.zeros((1, 20, 384), device="cuda")
    need = ops.pca_moments_workspace_bytes(1, 20, 384)
    assert need > 0
    with pytest.raises(ValueError, match="contiguous"):
        ops.pca_moments(torch.zeros((1, 384, 20), device="cuda").permute(0, 2, 1))
    with pytest.raises(TypeError):
        ops.pca_moments(x.double())
    with pytest.raises(ValueError, match="workspace"):
        ops.pca_moments(x, workspace=torch.zeros(need - 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.pca_moments(x.cpu())
    comp, mean = torch.zeros((1, 3, 20), device="cuda"), torch.zeros((1, 20), device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.pca_project(x, torch.zeros((1, 20, 3), device="cuda").permute(0, 2, 1), mean)
    with pytest.raises(TypeError):
        ops.pca_project(x, comp.double(), mean)
    with pytest.raises(ValueError):
        ops.pca_project(x, torch.zeros((1, 9, 20), device="cuda"), mean)
    proj, minmax = torch.zeros((1, 3, 384), device="cuda"), torch.zeros((1, 2), device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.pca_to_rgb(torch.zeros((1, 384, 3), device="cuda").permute(0, 2, 1), minmax)
    with pytest.raises(TypeError):
        ops.pca_to_rgb(proj.half(), minmax)
    with pytest.raises(ValueError):
        ops.pca_to_rgb(proj, minmax.cpu())


def _tiled_container(tiles, device):
    from micro_sam_amd.tiling import TileArray, TiledFeatures
    feats = TiledFeatures(REF.TILED["shape"], REF.TILED["tile_shape"], REF.TILED["halo"])
    for t, tile in enumerate(tiles):
        feats[t] = TileArray(torch.from_numpy(tile).to(device), (0, 0), (0, 0))
    return {"features": feats, "input_size": None, "original_size": None}


@pytest.mark.parametrize("n_slices", [None, 2])
def test_tiled_mosaic_and_pca(VIS, n_slices):
    from micro_sam_amd.tiling import Blocking
    tiles = REF.synthetic_tiles(7, n_slices=n_slices)
    mosaic = REF.tiled_mosaic(tiles, **REF.TILED)
    assert mosaic.shape[-2:] == (71, 111)
    tiling = Blocking([0, 0], REF.TILED["shape"], REF.TILED["tile_shape"])
    parts = [VIS._project_embeddings_to_tile(tiling.get_block_with_halo(t, list(REF.TILED["halo"])), torch.from_numpy(tiles[t]).cuda())
             for t in range(4)]
    assert [tuple(p.shape[-2:]) for p in parts] == [(57, 57), (57, 36), (9, 57), (14, 54)]
    got = VIS._resize_and_cocatenate([VIS._resize_and_cocatenate(parts[:2], axis=-1), VIS._resize_and_cocatenate(parts[2:], axis=-1)], axis=-2)
    assert got.is_cuda and tuple(got.shape) == mosaic.shape
    assert np.abs(got.cpu().numpy().astype(np.float64) - mosaic).max() <= 1e-6 * np.ptp(mosaic)
    emb = _tiled_container(tiles, "cuda")
    shape = REF.TILED["shape"]
    vis, scale = VIS.project_embeddings_for_visualization(emb)
    flt, scale_f = VIS.project_embeddings_for_visualization(emb, as_rgb=False)
    assert vis.is_cuda and flt.is_cuda
    vis, flt = vis.cpu().numpy(), flt.cpu().numpy()
    if n_slices is None:
        assert vis.shape == (71, 111, 3) and scale == scale_f == (shape[0] / 71, shape[1] / 111)
        REF.check_rgb(vis, mosaic, "tiled")
        REF.check_float(flt, mosaic, "tiled")
    else:
        assert vis.shape == (2, 71, 111, 3) and scale == scale_f == (1.0, shape[0] / 71, shape[1] / 111)
        for z in range(n_slices):
            REF.check_rgb(vis[z], mosaic[z], f"tiled slice {z}")
            REF.check_float(flt[z], mosaic[z], f"tiled slice {z}")
    host, _ = VIS.project_embeddings_for_visualization(_tiled_container(tiles, "cpu"))
    assert torch.is_tensor(host) and not host.is_cuda and np.array_equal(host.numpy(), vis)


def test_containers_of_the_encoder(VIS, predictor):
    """Plumbing equalities on real containers: no tolerance depends on the encoder's spectrum."""
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_tile
    image = synthetic_tile(4, (768, 1024))
    emb = util.precompute_image_embeddings(predictor, image, verbose=False)
    vis, scale = VIS.project_embeddings_for_visualization(emb)
    assert isinstance(vis, np.ndarray) and vis.dtype == np.uint8 and vis.shape == (48, 64, 3) and scale == (16.0, 16.0)
    assert np.array_equal(vis, VIS.compute_pca(emb["features"])[:48])
    emb_dev = util.precompute_image_embeddings(predictor, image, verbose=False, keep_on_device=True)
    assert emb_dev["features"].is_cuda
    vis_dev, scale_dev = VIS.project_embeddings_for_visualization(emb_dev)
    assert vis_dev.is_cuda and scale_dev == scale and np.array_equal(vis_dev.cpu().numpy(), vis)
    assert torch.equal(vis_dev, VIS.compute_pca(emb_dev["features"])[:48])
