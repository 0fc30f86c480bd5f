"""numpy restatement of the RGB network's upper-body crops, written from the stated semantics of the reference
rgb_network/roi_extraction.py:18-80 and OpenCV 3.3's BGR2GRAY / generic 8-bit INTER_CUBIC resize, independent of the product code:

  gray   Y = (1868 B + 9617 G + 4899 R + 8192) >> 14
  box    up = shcY - 120, down = hipY + 120, left = hipX - 180, right = hipX + 180 of skeleton row f; up <= 0 -> 1, down >= 480 -> 479,
         left <= 0 -> 1, right >= 640 -> 639; crop = gray[up:down, left:right] (a real numpy slice); gray[0:330, 0:640] when f has no
         skeleton row or the crop is empty
  resize per axis scale = 1 / (dst / src) in double; fx = float32((d + 0.5) scale - 0.5); sx = floor(fx); fx -= sx; float32 cubic
         weights (A = -0.75), the fourth 1 - c0 - c1 - c2; each rint(c * 2048) (half to even); taps sx-1..sx+2 clamped to the crop;
         horizontal int sums, vertical int sums, (v + 2^21) >> 22 clipped to 0..255
"""
import numpy as np


def gray(bgr):
    """(..., 3) uint8 BGR -> (...) uint8."""
    p = np.asarray(bgr).astype(np.int64)
    return ((1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14).astype(np.uint8)


def cubic_table(dst, src):
    """(sx int64 (dst,), weights int64 (dst, 4)) of one axis resized from src to dst samples."""
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx)
    fx = (fx - sx).astype(np.float32)
    A = np.float32(-0.75)
    one, two, three = np.float32(1), np.float32(2), np.float32(3)
    xp = fx + one
    c0 = ((A * xp - np.float32(5) * A) * xp + np.float32(8) * A) * xp - np.float32(4) * A
    c1 = ((A + two) * fx - (A + three)) * fx * fx + one
    xm = one - fx
    c2 = ((A + two) * xm - (A + three)) * xm * xm + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], 1).astype(np.float32)
    assert c.dtype == np.float32
    w = np.rint(c * np.float32(2048)).astype(np.int64)
    return sx.astype(np.int64), w


def resize(img, D):
    """(h, w) uint8 -> (D, D) uint8 by the fixed-point INTER_CUBIC path."""
    img = np.asarray(img)
    h, w = img.shape
    sx, wx = cubic_table(D, w)
    sy, wy = cubic_table(D, h)
    k = np.arange(4)
    ix = np.clip(sx[:, None] - 1 + k, 0, w - 1)                       # (D, 4)
    iy = np.clip(sy[:, None] - 1 + k, 0, h - 1)
    hor = (img.astype(np.int64)[:, ix] * wx[None]).sum(-1)             # (h, D)
    ver = (hor[iy] * wy[:, :, None]).sum(1)                            # (D, D)
    assert np.abs(hor).max() < 2 ** 31 and np.abs(ver).max() < 2 ** 31  # the int32 sums of the contract do not overflow
    return np.clip((ver + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def crop(gray_img, hipX, hipY, shcY, f):
    """The reference's crop of frame f (try / except IndexError and empty crops)."""
    try:
        up, down, left, right = shcY[f] - 120, hipY[f] + 120, hipX[f] - 180, hipX[f] + 180
        if up <= 0:
            up = 1
        if down >= 480:
            down = 479
        if left <= 0:
            left = 1
        if right >= 640:
            right = 639
        c = gray_img[int(up):int(down), int(left):int(right)]
        if c.size == 0:
            raise ValueError("empty crop")        # cv2.resize raises; the reference's bare except falls back
        return c
    except (IndexError, ValueError):
        return gray_img[0:330, 0:640]


def box(gray_img, hipX, hipY, shcY, f):
    """[y0, y1, x0, x1) of crop(), found through numpy's own slice objects."""
    H, W = gray_img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    c = crop(ys, hipX, hipY, shcY, f)
    cx = crop(xs, hipX, hipY, shcY, f)
    return [int(c[0, 0]), int(c[-1, 0]) + 1, int(cx[0, 0]), int(cx[0, -1]) + 1]


def roi(frame, box_, D):
    """(D, D) uint8 of one BGR frame and a box [y0, y1, x0, x1)."""
    y0, y1, x0, x1 = box_
    return resize(gray(frame[y0:y1, x0:x1]), D)


def extract(frames, hipX, hipY, shcY, D=60):
    """(n, D, D, 1) uint8: the reference's loop over frames."""
    out = np.zeros((len(frames), D, D, 1), np.uint8)
    for f, fr in enumerate(frames):
        out[f, :, :, 0] = resize(crop(gray(fr), hipX, hipY, shcY, f), D)
    return out
