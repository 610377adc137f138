"""A synthetic image sequence for the tracker (System) that needs no interpolation, so it is exact and cheap.

The image is cut into horizontal bands; band b is a fronto-parallel textured plane at depth Z_b.  The camera looks
along +z and translates along +x by `step` per frame, so band b of frame k is the band's texture shifted left by
k * d_b pixels with d_b = fx * step / Z_b an integer: img_k[band b][:, u] = texture_b[:, u + k * d_b].  The ground
truth follows: camera centre C_k = (k * step, 0, 0), identity rotation, world = the first camera.

A patch across a band border sees two depths at once: those are the outliers that the RANSAC, the chi2 removal of the
bundle adjustment and the depth filter's no-match path must meet.
"""
import numpy as np

WIDTH, HEIGHT = 480, 160
FX = FY = 300.0
CX, CY = 240.0, 80.0
# px per frame of the bands, top to bottom.  Not monotone: inverse depth linear in the row would be one tilted plane,
# for which the essential matrix is degenerate.  Not smaller: at 2..5 px the two-view initialisation of this narrow
# scene is ill-conditioned (rotation about y trades against translation along x within the 1-px RANSAC threshold).
DISPARITY = (16, 8, 20, 12)
STEP = 0.1                 # camera translation per frame; Z_b = FX * STEP / d_b = 1.875, 3.75, 1.5, 2.5
CELL = 16
N_FRAMES = 8
MAX_FRAMES = 12            # the textures are cut for this many frames (longer sequences: wider textures, other images)
TEXTURE_SEED = 12

CAMERA = dict(fx=FX, fy=FY, cx=CX, cy=CY, width=WIDTH, height=HEIGHT)


def band_depths(disparity=DISPARITY, fx=FX, step=STEP):
    return [fx * step / d for d in disparity]


def _texture(rng, rows, cols):
    """Smooth random texture with strong gradients: 3-px blocks of uniform noise, box-blurred once (the detector's
    threshold is on the gradient magnitude; the KLT needs structure that survives three pyrDown levels)."""
    blk = 3
    coarse = rng.integers(0, 256, size=((rows + blk - 1) // blk + 1, (cols + blk - 1) // blk + 1)).astype(np.float64)
    t = np.kron(coarse, np.ones((blk, blk)))[:rows + 2, :cols + 2]
    s = sum(t[i:i + rows, j:j + cols] for i in range(3) for j in range(3)) / 9.0
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def make_sequence(n_frames=N_FRAMES, width=WIDTH, height=HEIGHT, disparity=DISPARITY, seed=TEXTURE_SEED):
    """(images (n_frames, height, width) uint8, ground-truth world->camera poses (n_frames, 7) in Sophus order)."""
    rng = np.random.default_rng(seed)
    nb = len(disparity)
    edges = [height * b // nb for b in range(nb + 1)]
    imgs = np.zeros((n_frames, height, width), np.uint8)
    for b, d in enumerate(disparity):
        rows = edges[b + 1] - edges[b]
        tex = _texture(rng, rows, width + d * (max(n_frames, MAX_FRAMES) - 1))
        for k in range(n_frames):
            imgs[k, edges[b]:edges[b + 1]] = tex[:, k * d:k * d + width]
    poses = np.zeros((n_frames, 7))
    poses[:, 3] = 1.0
    poses[:, 4] = -STEP * np.arange(n_frames)  # t = -R C
    return imgs, poses


def config_kwargs(**over):
    """The Config fields of the committed scene (svo_amd.Config and tests/system_ref.Config take the same names)."""
    kw = dict(img_width=WIDTH, img_height=HEIGHT, fx=FX, fy=FY, cx=CX, cy=CY, cell_pixel_size=CELL,
              min_level_image_pyramid=0, max_level_image_pyramid=3, disparity_threshold=5.0,
              desired_detected_points_for_initialization=400, ransac_seed=0,
              map_cell_seed=5)
    kw.update(over)
    return kw
