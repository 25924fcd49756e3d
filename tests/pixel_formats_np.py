"""The bilinear BGGR demosaic, stated in numpy from its definition, and a sampler that makes a mosaic of a colour picture.
Imports neither `oracle/` nor the HIP package; resize, grey, undistort and CLAHE come from tests/preproc_definitions_np.py.

Colour layout of the mosaic: even row, even column B; odd row, odd column R; every other site G.  An interior pixel keeps its own
sample for the colour of its site and interpolates the other two from its 3 x 3 neighbourhood:
  * at a B or R site: G is the average of the four edge neighbours (the cross), the opposite colour the average of the four corner
    neighbours (the diagonal), both (a + b + c + d + 2) >> 2;
  * at a G site: the two other colours are the averages of the horizontal pair and of the vertical pair, (a + b + 1) >> 1 -- in an even
    row the horizontal neighbours are B and the vertical ones R, in an odd row the other way round.
A border pixel takes the value of the nearest interior pixel (its coordinates clamped to 1 .. size - 2).  A mosaic with a side below
3 has no interior pixel: the picture is all zeros."""
import numpy as np


def mosaic(bgr):
    """The BGGR mosaic a sensor would deliver of the picture bgr [h, w, 3] (channels B, G, R): each site keeps its colour's sample."""
    h, w = bgr.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    ch = np.where((yy % 2 == 0) & (xx % 2 == 0), 0, np.where((yy % 2 == 1) & (xx % 2 == 1), 2, 1))
    return np.ascontiguousarray(np.take_along_axis(bgr, ch[..., None], axis=2)[..., 0])


def demosaic_bggr(m):
    """mosaic [h, w] uint8 -> picture [h, w, 3] uint8, channels B, G, R."""
    h, w = m.shape
    out = np.zeros((h, w, 3), np.uint8)
    if h < 3 or w < 3:
        return out
    v = m.astype(np.int64)
    c = v[1:-1, 1:-1]
    up, down, left, right = v[:-2, 1:-1], v[2:, 1:-1], v[1:-1, :-2], v[1:-1, 2:]
    cross = (up + down + left + right + 2) >> 2
    diag = (v[:-2, :-2] + v[:-2, 2:] + v[2:, :-2] + v[2:, 2:] + 2) >> 2
    horz = (left + right + 1) >> 1
    vert = (up + down + 1) >> 1
    yy, xx = np.mgrid[1:h - 1, 1:w - 1]
    ey, ex = yy % 2 == 0, xx % 2 == 0
    b_site, r_site = ey & ex, ~ey & ~ex
    B = np.where(b_site, c, np.where(r_site, diag, np.where(ey, horz, vert)))
    G = np.where(b_site | r_site, cross, c)
    R = np.where(r_site, c, np.where(b_site, diag, np.where(ey, vert, horz)))
    inner = np.stack([B, G, R], axis=2).astype(np.uint8)
    iy = np.clip(np.arange(h), 1, h - 2) - 1
    ix = np.clip(np.arange(w), 1, w - 2) - 1
    return np.ascontiguousarray(inner[iy][:, ix])
