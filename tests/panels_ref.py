"""The exact model of l2i_panels_u8 (csrc/l2i_panels.hip) in numpy: the reference's clip_ims (np.uint8(np.clip(((x + 1) / 2.0) * 255, 0, 255)) in
float32) per pixel, and its imgrid per grid (every tile padded on its bottom and right with the fill value, tiles row-major, the last gutter
cropped).  Integer output: the kernel is held to it bit for bit (tests/test_panels_gpu.py).  ``mistake`` seeds one wrong reading of either half;
tests/test_panels_ref_cpu.py shows that each of them changes bytes on the inputs the GPU tests use, so those inputs can tell them apart."""
import numpy as np

# (G, rows, cols, C, H, W, pad, N): N = G * rows * cols unless a case wants empty tiles
CASES = (
    (1, 1, 1, 3, 4, 4, 0, 1),
    (2, 1, 3, 3, 5, 5, 0, 6),          # 15-byte tile rows: neighbouring tiles share dwords, odd row pitch
    (1, 2, 3, 3, 8, 8, 1, 5),          # N = 5 for six tiles: one empty tile
    (3, 1, 7, 3, 32, 32, 1, 21),
    (1, 3, 3, 1, 7, 3, 2, 9),
    (1, 1, 2, 3, 2, 1024, 1, 2),
)
QUANT_MISTAKES = ('rint', 'float64', 'fused')
GRID_MISTAKES = ('no_crop', 'gutter_top_left', 'fill_in_tiles')


def quant_inputs():
    """The 256 thresholds float32(2k / 255 - 1), where clip_ims steps from k - 1 to k, each with its two float32 neighbours, and ten values
    beyond them: 778 in all."""
    t = (2.0 * np.arange(256, dtype=np.float64) / 255.0 - 1.0).astype(np.float32)
    lo, hi = np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
    extra = np.array([1.5, -1.5, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e38, -3e38], dtype=np.float32)
    return np.concatenate([np.stack([lo, t, hi], 1).reshape(-1), extra])


def clip_ims(x, mistake=None):
    """uint8 of float32 x; NaN inputs have no defined result in numpy (the kernel gives 0: asserted on its own)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        if mistake == 'float64':
            t = ((x.astype(np.float64) + 1) / 2.0) * 255
        elif mistake == 'fused':
            t = x * np.float32(127.5) + np.float32(127.5)                          # the constants folded: the roundings fall elsewhere
        else:
            t = ((x + np.float32(1)) / np.float32(2.0)) * np.float32(255)
            assert t.dtype == np.float32
        t = np.clip(t, 0, 255)
        if mistake == 'rint':
            t = np.rint(t)
        return np.uint8(t)


def grid_hw(rows, cols, H, W, pad):
    return rows * (H + pad) - pad, cols * (W + pad) - pad


def panels(x, tile_src, G, rows, cols, pad=0, fill=0, mistake=None):
    """out [G, GH, GW, C] uint8 of x [N, C, H, W] float32; tile_src [G * rows * cols], a value outside [0, N) = an empty tile."""
    x = np.asarray(x, dtype=np.float32)
    N, C, H, W = x.shape
    tile_src = np.asarray(tile_src).reshape(-1)
    assert tile_src.size == G * rows * cols
    q = clip_ims(x, mistake if mistake in QUANT_MISTAKES else None).transpose(0, 2, 3, 1)
    tiles = np.full((tile_src.size, H + pad, W + pad, C), fill, dtype=np.uint8)
    for t, s in enumerate(tile_src):
        if 0 <= s < N:
            if mistake == 'gutter_top_left':
                tiles[t, pad:, pad:] = q[s]
            else:
                tiles[t, :H, :W] = q[s]
            if mistake == 'fill_in_tiles' and pad:                     # the gutter drawn over the tile's own last rows and columns
                tiles[t, H - pad:H] = fill
                tiles[t, :, W - pad:W] = fill
    grid = tiles.reshape(G, rows, cols, H + pad, W + pad, C).transpose(0, 1, 3, 2, 4, 5).reshape(G, rows * (H + pad), cols * (W + pad), C)
    if pad and mistake != 'no_crop':
        grid = grid[:, :-pad, :-pad]
    return np.ascontiguousarray(grid)


def case_inputs(case, seed=0):
    """(x [N, C, H, W] float32 in about [-1.2, 1.2] with the thresholds sprinkled in, tile_src) of a case: tile t shows image t, tiles beyond N are
    empty."""
    G, rows, cols, C, H, W, pad, N = case
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.2, 1.2, size=(N, C, H, W)).astype(np.float32)
    qi = quant_inputs()
    flat = x.reshape(-1)
    pos = rs.permutation(flat.size)[:min(flat.size // 2, qi.size)]
    flat[pos] = qi[:pos.size]
    tile_src = np.arange(G * rows * cols, dtype=np.int32)
    return x, tile_src
