"""CPU reference for micro_sam_amd.visualization (NOT a test): elf's ``embedding_pca`` restated on ``sklearn.decomposition.PCA`` (elf is
not available: restated from its published source), the reference's tiled mosaic restated with ``scipy.ndimage.zoom`` (skimage's
``resize``, enlarging only, is ``zoom(order=1, mode="mirror", grid_mode=True)``), a seeded generator of synthetic embeddings whose
third and fourth sample eigenvalues are well separated, and the checks tests/test_visualization_host.py and
tests/test_gpu_visualization.py share.  Written for the tests; nothing here is used by the product."""
import numpy as np
from scipy import ndimage as ndi
from sklearn.decomposition import PCA

AMPLITUDES = (8.0, 5.0, 3.0, 1.5)
NOISE_SIGMA, OFFSET_SIGMA = 0.3, 2.0
FLOAT_MARGIN = 4.0            # device error <= 4 x the error of sklearn run on the float32 input (both against the float64 reference)
MAX_DIFFERING = 0.005         # uint8: at most 0.5 % of the values differ from the float64 reference's, none by more than 1

# numeric shapes (C, H, W): the real shape; a ragged position chunk; C below one MFMA tile and no multiple of 32; fewer samples than channels
SHAPES = [(256, 64, 64), (256, 37, 29), (20, 16, 24), (256, 8, 8)]
TILED = {"shape": (300, 420), "tile_shape": (256, 256), "halo": (32, 32)}


# ---- the reference

def embedding_pca(embeddings, n_components=3, as_rgb=True, dtype=np.float64):
    """elf.segmentation.embeddings.embedding_pca on an embedding [C, H, W], computed in ``dtype``."""
    if as_rgb and n_components != 3:
        raise ValueError("as_rgb needs three components")
    emb = np.asarray(embeddings).astype(dtype)
    samples = emb.reshape(emb.shape[0], -1).T
    flat = PCA(n_components=n_components).fit_transform(samples).T
    out = flat.reshape((n_components,) + emb.shape[1:])
    if as_rgb:
        out = (255 * (out - out.min()) / np.ptp(out)).astype("uint8")
    return out


def eigenvalues(embedding):
    """Sample eigenvalues (descending) of an embedding [C, H, W] in float64."""
    emb = np.asarray(embedding, dtype=np.float64)
    return np.linalg.eigvalsh(np.cov(emb.reshape(emb.shape[0], -1)))[::-1]


def compute_pca(embeddings, n_components=3, as_rgb=True, dtype=np.float64):
    """[1, C, H, W] -> (H, W, k); [Z, 1, C, H, W] -> (Z, H, W, k), every slice on its own."""
    embeddings = np.asarray(embeddings)
    if embeddings.ndim == 4:
        return embedding_pca(embeddings[0], n_components, as_rgb, dtype).transpose(1, 2, 0)
    if embeddings.ndim == 5:
        return np.stack([embedding_pca(e[0], n_components, as_rgb, dtype).transpose(1, 2, 0) for e in embeddings])
    raise ValueError(f"ndim {embeddings.ndim}")


def _aspect_crop(grid, shape):
    """How much of a (gh, gw) embedding grid an image of ``shape`` padded to a square covers."""
    gh, gw = grid
    if shape[0] > shape[1]:
        gw = int(float(shape[1] / shape[0]) * gw)
    elif shape[1] > shape[0]:
        gh = int(float(shape[0] / shape[1]) * gh)
    return gh, gw


def tile_blocks(shape, tile_shape, halo):
    """Per tile in C order: (grid position, outer begin, outer end, inner begin relative to the outer block, inner end likewise)."""
    ny, nx = (-(-s // t) for s, t in zip(shape, tile_shape))
    out = []
    for i in range(ny):
        for j in range(nx):
            ib = (i * tile_shape[0], j * tile_shape[1])
            ie = tuple(min(b + t, s) for b, t, s in zip(ib, tile_shape, shape))
            ob = tuple(max(b - h, 0) for b, h in zip(ib, halo))
            oe = tuple(min(e + h, s) for e, h, s in zip(ie, halo, shape))
            out.append(((i, j), ob, oe, tuple(b - o for b, o in zip(ib, ob)), tuple(e - o for e, o in zip(ie, ob))))
    return out


def _enlarge(arr, axis, length):
    factors = [1.0] * arr.ndim
    factors[axis] = length / arr.shape[axis]
    out = ndi.zoom(arr, factors, order=1, mode="mirror", grid_mode=True)
    assert out.shape[axis] == length
    return out


def tiled_mosaic(tiles, shape, tile_shape, halo):
    """The reference's mosaic of per-tile embeddings ([1, C, h, w] or [Z, 1, C, h, w] each, in tile order)."""
    rows = {}
    for tile, ((i, j), ob, oe, lb, le) in zip(tiles, tile_blocks(shape, tile_shape, halo)):
        tile = np.asarray(tile)
        outer = tuple(e - b for b, e in zip(ob, oe))
        gh, gw = _aspect_crop(tile.shape[-2:], outer)
        part = tile[..., :gh, :gw]
        sy, sx = gh / float(outer[0]), gw / float(outer[1])
        part = part[..., int(np.round(lb[0] * sy)):int(np.round(le[0] * sy)), int(np.round(lb[1] * sx)):int(np.round(le[1] * sx))]
        rows.setdefault(i, []).append(part)
    strips = []
    for i in sorted(rows):
        height = max(p.shape[-2] for p in rows[i])
        strips.append(np.concatenate([_enlarge(p, p.ndim - 2, height) for p in rows[i]], axis=-1))
    width = max(s.shape[-1] for s in strips)
    return np.concatenate([_enlarge(s, s.ndim - 1, width) for s in strips], axis=-2)


# ---- synthetic embeddings

def _patterns(yy, xx):
    two_pi = 2.0 * np.pi
    return np.stack([np.sin(two_pi * yy), np.cos(two_pi * xx), np.sin(two_pi * (xx + yy)), np.cos(two_pi * (2.0 * xx - yy))])


def frame(seed, channels):
    """(four orthonormal directions [C, 4], per-channel offset [C]) shared by everything generated for one ``seed``."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((channels, channels)))
    return q[:, :4], OFFSET_SIGMA * rng.standard_normal(channels)


def synthetic_embedding(seed, channels, height, width, yy=None, xx=None, noise_seed=None):
    """float32 [C, H, W]: four smooth patterns of the normalised coordinates (``yy``, ``xx``: [H, W]; default pixel centres of the unit
    square) with amplitudes 8, 5, 3, 1.5 along four orthonormal directions, Gaussian noise of sigma 0.3, a per-channel offset of sigma 2."""
    basis, offset = frame(seed, channels)
    if yy is None:
        yy, xx = np.meshgrid((np.arange(height) + 0.5) / height, (np.arange(width) + 0.5) / width, indexing="ij")
    signal = np.einsum("ck,k,khw->chw", basis, np.asarray(AMPLITUDES), _patterns(yy, xx))
    rng = np.random.default_rng([seed, 1 if noise_seed is None else 2 + noise_seed])
    return (signal + NOISE_SIGMA * rng.standard_normal(signal.shape) + offset[:, None, None]).astype(np.float32)


def synthetic_tiles(seed, channels=256, grid=64, n_slices=None, shape=TILED["shape"], tile_shape=TILED["tile_shape"], halo=TILED["halo"]):
    """Per tile a float32 [1, C, grid, grid] (or [Z, 1, C, grid, grid]) embedding: the patterns at the GLOBAL image coordinates of the tile's
    outer block padded to a square, so that the mosaic has the structure of one image."""
    tiles = []
    for t, (_, ob, oe, _, _) in enumerate(tile_blocks(shape, tile_shape, halo)):
        side = max(e - b for b, e in zip(ob, oe))
        ys = (ob[0] + (np.arange(grid) + 0.5) * side / grid) / shape[0]
        xs = (ob[1] + (np.arange(grid) + 0.5) * side / grid) / shape[1]
        yy, xx = np.meshgrid(ys, xs, indexing="ij")
        if n_slices is None:
            tiles.append(synthetic_embedding(seed, channels, grid, grid, yy, xx, noise_seed=t)[None])
        else:
            tiles.append(np.stack([synthetic_embedding(seed, channels, grid, grid, yy + 0.13 * z, xx, noise_seed=100 * z + t)[None]
                                   for z in range(n_slices)]))
    return tiles


# ---- shared checks

def assert_separated(embedding):
    """Precondition of every numeric test on its input: the third component is well defined."""
    lam = eigenvalues(embedding)
    assert lam[2] / lam[3] >= 2.0, lam[:5]


def float_error(values, ref64):
    return float(np.abs(np.asarray(values, dtype=np.float64) - ref64).max() / np.ptp(ref64))


def check_float(got, embedding, label=""):
    """``got``: the product's float32 (H, W, 3) for the float32 ``embedding`` [1, C, H, W].  Returns (error, r)."""
    assert_separated(embedding[0])
    ref64 = compute_pca(embedding, 3, False, np.float64)
    r = float_error(compute_pca(embedding, 3, False, np.float32), ref64)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape
    err = float_error(got, ref64)
    print(f"embedding_pca float {label or tuple(embedding.shape)}: error {err:.3e}, r {r:.3e}, ratio {err / r:.3f}")
    assert err <= FLOAT_MARGIN * r, (err, r)
    return err, r


def check_rgb(got, embedding, label=""):
    """``got``: the product's uint8 (H, W, 3).  Returns the fraction of values that differ from the float64 reference's."""
    assert_separated(embedding[0])
    ref = compute_pca(embedding, 3, True, np.float64)
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    frac = float((diff != 0).mean())
    print(f"embedding_pca uint8 {label or tuple(embedding.shape)}: max difference {int(diff.max())}, differing {frac:.5f}")
    assert diff.max() <= 1 and frac <= MAX_DIFFERING, (int(diff.max()), frac)
    return frac
