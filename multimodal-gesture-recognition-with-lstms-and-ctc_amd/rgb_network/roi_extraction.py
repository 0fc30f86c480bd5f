"""The RGB network's upper-body frames from colour video: gray, crop around the skeleton's hip and shoulder centres, resize.

The reference (rgb_network/roi_extraction.py:18-80, OpenCV) decodes each colour video, converts every frame to gray, crops
``gray[shcY-120 : hipY+120, hipX-180 : hipX+180]`` after its one-sided clamps (``gray[0:330, 0:640]`` when the skeleton has no row
for the frame or the crop is empty) and resizes the crop to img_dim x img_dim with INTER_CUBIC.  Here the host builds the boxes
(``crop_boxes``) and reads the frames; one ``mgr_roi_crop`` launch per chunk of frames (csrc/roi.hip) does the gray conversion, the
crop and the resize with OpenCV's 8-bit fixed-point arithmetic, restated in DESIGN 9d.  That integer path is the contract, bit for
bit; parity with OpenCV itself (which may route through IPP, and whose vectorised vertical pass rounds in float) is not pinned.

Videos are uncompressed AVI (BI_RGB 24-bit, OpenDML continuations included) or ``.npy`` stacks (n, 480, 640, 3) of uint8 BGR; the
ChaLearn ``.mp4`` files are refused and must be converted first (INTEGRATION).
"""
import argparse
import os
import re
import struct

import numpy as np

from .. import _capi

#: the reference's frame size and its fallback crop gray[0:330, 0:640]
FRAME_H, FRAME_W = 480, 640
FALLBACK = (0, 330, 0, 640)
#: frames per upload: the device holds one chunk of frames (~59 MB at 640 x 480), whatever the video's length
CHUNK_FRAMES = 64
NAME_RE = re.compile(r'Sample(\d+)_')
VIDEO_EXTS = (".avi", ".npy")
COMPRESSED_EXTS = (".mp4", ".m4v", ".mov", ".mkv", ".webm", ".wmv", ".flv", ".mpg", ".mpeg")

_DEV = [None]


def _device():
    if _DEV[0] is None:
        _DEV[0] = _capi.Device(0)
    return _DEV[0]


# ---- boxes ----------------------------------------------------------------------------------------------------------------------
def _int_column(v, name):
    a = np.asarray(v)
    if a.dtype.kind not in "iu" and a.size:   # (an empty list is a file without skeleton rows)
        raise ValueError("skeletal column %s must be integer-typed, got %s (NaN or float joints would make the reference fall back "
                         "to gray[0:330, 0:640] on every frame)" % (name, a.dtype))
    return a.astype(np.int64).reshape(-1)


def _slice_bounds(a, b, n):
    """numpy's a:b on an axis of length n (step 1): negative bounds count from the end, then both are clipped to [0, n]."""
    a = np.where(a < 0, a + n, a).clip(0, n)
    b = np.where(b < 0, b + n, b).clip(0, n)
    return a, b


def crop_boxes(hipX, hipY, shcY, n_frames, H=FRAME_H, W=FRAME_W):
    """int32 (n_frames, 4) boxes [y0, y1, x0, x1) of frames 0..n_frames-1, the reference's rules: skeleton row f (file order) gives
    up = shcY - 120, down = hipY + 120, left = hipX - 180, right = hipX + 180; up <= 0 -> 1, down >= 480 -> 479, left <= 0 -> 1,
    right >= 640 -> 639 (the constants are the reference's, whatever H and W); numpy slice semantics; frames past the skeleton rows
    and empty crops take gray[0:330, 0:640] (sliced the same way)."""
    hx, hy, sy = _int_column(hipX, "hipX"), _int_column(hipY, "hipY"), _int_column(shcY, "shcY")
    if not hx.size == hy.size == sy.size:
        raise ValueError("hipX, hipY and shcY differ in length")
    n = int(n_frames)
    if n < 0:
        raise ValueError("n_frames must be >= 0")
    m = min(n, hx.size)
    hx, hy, sy = hx[:m], hy[:m], sy[:m]
    up, down, left, right = sy - 120, hy + 120, hx - 180, hx + 180
    up = np.where(up <= 0, 1, up)
    down = np.where(down >= 480, 479, down)
    left = np.where(left <= 0, 1, left)
    right = np.where(right >= 640, 639, right)
    y0, y1 = _slice_bounds(up, down, H)
    x0, x1 = _slice_bounds(left, right, W)
    fy0, fy1 = _slice_bounds(np.array([FALLBACK[0]]), np.array([FALLBACK[1]]), H)
    fx0, fx1 = _slice_bounds(np.array([FALLBACK[2]]), np.array([FALLBACK[3]]), W)
    boxes = np.empty((n, 4), np.int32)
    boxes[:] = (fy0[0], fy1[0], fx0[0], fx1[0])
    ok = (y1 > y0) & (x1 > x0)
    boxes[:m][ok] = np.stack([y0, y1, x0, x1], 1)[ok]
    return boxes


# ---- uncompressed AVI -----------------------------------------------------------------------------------------------------------
class _Avi:
    """Layout of an uncompressed AVI: the video stream's geometry and the (offset, size) of every frame chunk, in order, across the
    RIFF 'AVI ' part and its OpenDML RIFF 'AVIX' continuations."""

    def __init__(self, path):
        self.path = path
        self.width = self.height = None
        self.bottom_up = True
        self.stream = None
        self.frames = []
        with open(path, "rb") as f:
            f.seek(0, 2)
            end = f.tell()
            f.seek(0)
            pos, first = 0, True
            while pos + 12 <= end:
                f.seek(pos)
                tag, size, form = struct.unpack("<4sI4s", f.read(12))
                if tag != b"RIFF" or form != (b"AVI " if first else b"AVIX"):
                    if first:
                        raise ValueError("%s: not an AVI file (RIFF 'AVI ' expected, found %r %r)" % (path, tag, form))
                    break
                stop = min(pos + 8 + size, end)
                self._walk(f, pos + 12, stop, top=first)
                if first and self.stream is None:
                    raise ValueError("%s: no video stream header" % path)
                first = False
                pos = pos + 8 + size + (size & 1)

    def _chunks(self, f, pos, stop):
        while pos + 8 <= stop:
            f.seek(pos)
            tag, size = struct.unpack("<4sI", f.read(8))
            yield tag, pos + 8, size
            pos += 8 + size + (size & 1)   # RIFF chunks are padded to even sizes

    def _walk(self, f, pos, stop, top):
        for tag, data, size in self._chunks(f, pos, stop):
            if tag == b"LIST":
                f.seek(data)
                kind = f.read(4)
                if kind == b"hdrl" and top:
                    self._hdrl(f, data + 4, data + size)
                elif kind in (b"movi", b"rec "):
                    self._walk(f, data + 4, min(data + size, stop), top=False)
                continue
            if self.stream is None or len(tag) != 4 or not tag[:2].isdigit():
                continue        # JUNK, idx1, ix##, other streams' headers ...
            if int(tag[:2]) != self.stream or tag[2:] not in (b"db", b"dc"):
                continue        # other streams' data (audio 01wb ...)
            if size != self.frame_bytes:
                raise ValueError("%s: frame chunk of %d bytes, expected %d (dropped or compressed frames are not supported)"
                                 % (self.path, size, self.frame_bytes))
            self.frames.append(data)

    def _hdrl(self, f, pos, stop):
        idx = 0
        for tag, data, size in self._chunks(f, pos, stop):
            if tag != b"LIST":
                continue
            f.seek(data)
            if f.read(4) != b"strl":
                continue
            strh = strf = None
            for t2, d2, s2 in self._chunks(f, data + 4, data + size):
                f.seek(d2)
                if t2 == b"strh":
                    strh = f.read(s2)
                elif t2 == b"strf":
                    strf = f.read(s2)
            if strh is not None and strh[:4] == b"vids" and self.stream is None:
                if strf is None or len(strf) < 40:
                    raise ValueError("%s: video stream without a BITMAPINFOHEADER" % self.path)
                _, w, h, _, bits, comp = struct.unpack("<IiiHHI", strf[:20])
                if comp != 0 or bits != 24:
                    fourcc = struct.pack("<I", comp)
                    raise ValueError("%s: only uncompressed 24-bit BI_RGB video is read (found compression %r, %d bits per pixel); "
                                     "convert it to raw bgr24 AVI or a .npy frame stack" % (self.path, fourcc, bits))
                if w <= 0 or h == 0:
                    raise ValueError("%s: bad frame size %d x %d" % (self.path, w, h))
                self.stream, self.width, self.height, self.bottom_up = idx, w, abs(h), h > 0
                self.stride = (3 * w + 3) & ~3
                self.frame_bytes = self.stride * self.height
            idx += 1

    def read(self, start, count):
        out = np.empty((count, self.height, self.width, 3), np.uint8)
        with open(self.path, "rb") as f:
            for i in range(count):
                f.seek(self.frames[start + i])
                rows = np.frombuffer(f.read(self.frame_bytes), np.uint8).reshape(self.height, self.stride)
                img = rows[:, :3 * self.width].reshape(self.height, self.width, 3)
                out[i] = img[::-1] if self.bottom_up else img
        return out


def _refuse_compressed(path):
    raise ValueError("%s: compressed video is not decoded here; convert it to raw bgr24 AVI (ffmpeg -i %s -c:v rawvideo "
                     "-pix_fmt bgr24 NAME.avi) or to a .npy frame stack (n, 480, 640, 3) uint8 BGR" % (path, os.path.basename(path)))


def _open_video(path):
    """(n_frames, read(start, count) -> (count, H, W, 3) uint8 BGR) of an uncompressed AVI or a .npy stack."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path, mmap_mode="r")
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise ValueError("%s: a .npy video must be (n, H, W, 3) uint8 BGR, got %s %s" % (path, a.shape, a.dtype))
        return a.shape[0], lambda s, k: np.asarray(a[s:s + k])
    if ext == ".avi":
        avi = _Avi(path)
        return len(avi.frames), avi.read
    _refuse_compressed(path)


def iter_avi(path, chunk=CHUNK_FRAMES):
    """Frames of an uncompressed AVI (or a .npy stack) in chunks of at most `chunk`: (k, H, W, 3) uint8 BGR, top row first."""
    n, read = _open_video(path)
    for s in range(0, n, int(chunk)):
        yield read(s, min(int(chunk), n - s))


def read_avi(path):
    """All frames of an uncompressed AVI (or a .npy stack): (n, H, W, 3) uint8 BGR, top row first."""
    n, read = _open_video(path)
    return read(0, n)


# ---- the GPU path ---------------------------------------------------------------------------------------------------------------
def _check_frames(frames):
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[1:] != (FRAME_H, FRAME_W, 3):
        raise ValueError("frames must be (n, %d, %d, 3) uint8 BGR, got %s %s" % (FRAME_H, FRAME_W, frames.shape, frames.dtype))


class _Cropper:
    """Device buffers for one chunk of frames, reused across chunks and videos: peak device memory does not depend on the number
    of frames."""

    def __init__(self, dev, img_dim, H=FRAME_H, W=FRAME_W, chunk=CHUNK_FRAMES):
        if not 1 <= int(img_dim) <= 64:
            raise ValueError("img_dim must be in [1, 64]")
        self.dev, self.D, self.H, self.W, self.chunk = dev, int(img_dim), H, W, int(chunk)
        self.d_frames = dev.empty((self.chunk, H, W, 3), np.uint8)
        self.d_boxes = dev.empty((self.chunk, 4), np.int32)
        self.d_out = dev.empty((self.chunk, self.D, self.D), np.uint8)

    def run(self, frames, boxes):
        """(k, D, D, 1) uint8 of k <= chunk frames."""
        k = frames.shape[0]
        if k == 0:
            return np.zeros((0, self.D, self.D, 1), np.uint8)
        self.d_frames.view(0, (k, self.H, self.W, 3)).upload(frames)
        self.d_boxes.view(0, (k, 4)).upload(boxes)
        out = self.d_out.view(0, (k, self.D, self.D))
        self.dev.call("mgr_roi_crop", self.d_frames, k, self.H, self.W, self.d_boxes, self.D, out)
        return out.download().reshape(k, self.D, self.D, 1)

    def close(self):
        for a in (self.d_frames, self.d_boxes, self.d_out):
            a.free()
        self.dev._arrays = [a for a in self.dev._arrays if a.ptr]


def roi_frames(frames, boxes, img_dim=60, dev=None, chunk=CHUNK_FRAMES):
    """(n, img_dim, img_dim, 1) uint8 crops of (n, 480, 640, 3) uint8 BGR frames for int32 (n, 4) boxes [y0, y1, x0, x1) (from
    crop_boxes), uploaded and launched `chunk` frames at a time."""
    _check_frames(frames)
    boxes = np.ascontiguousarray(boxes, np.int32)
    if boxes.shape != (frames.shape[0], 4):
        raise ValueError("boxes must be (%d, 4), got %s" % (frames.shape[0], boxes.shape))
    y0, y1, x0, x1 = boxes.T
    if not ((y0 >= 0) & (y1 <= FRAME_H) & (y1 > y0) & (x0 >= 0) & (x1 <= FRAME_W) & (x1 > x0)).all():
        raise ValueError("boxes must be non-empty and inside the frame (crop_boxes applies the reference's rules)")
    cropper = _Cropper(dev or _device(), img_dim, chunk=chunk)
    try:
        parts = [cropper.run(frames[s:s + cropper.chunk], boxes[s:s + cropper.chunk]) for s in range(0, frames.shape[0], cropper.chunk)]
    finally:
        cropper.close()
    return np.concatenate(parts) if parts else np.zeros((0, cropper.D, cropper.D, 1), np.uint8)


def _skeleton_rows(df, file_num):
    vf = df[df['file_number'] == file_num]
    return vf['hipX'].values, vf['hipY'].values, vf['shcY'].values


def _read_skeletal(df):
    if isinstance(df, (str, os.PathLike)):
        import pandas as pd
        df = pd.read_csv(df)
    for col in ("file_number", "hipX", "hipY", "shcY"):
        if col not in df.columns:
            raise ValueError("skeletal table has no column %s" % col)
    for col in ("hipX", "hipY", "shcY"):
        _int_column(df[col].values, col)
    return df


def video_files(video_path):
    """The names in video_path that extract_body processes, sorted; a compressed video among them raises ValueError."""
    names = []
    for name in sorted(os.listdir(video_path)):
        if not NAME_RE.search(name):
            continue
        ext = os.path.splitext(name)[1].lower()
        if ext in COMPRESSED_EXTS:
            _refuse_compressed(os.path.join(video_path, name))
        if ext in VIDEO_EXTS:
            names.append(name)
    return names


def out_name(video_name):
    return os.path.splitext(video_name)[0] + ".npy"


def extract_video(df, path, img_dim=60, dev=None, cropper=None):
    """(frames, img_dim, img_dim, 1) uint8 crops of one video (.avi or .npy) with the skeleton rows of its file number in df."""
    file_num = int(NAME_RE.search(os.path.basename(path)).group(1))
    hx, hy, sy = _skeleton_rows(df, file_num)
    n, read = _open_video(path)
    own = cropper is None
    cropper = cropper or _Cropper(dev or _device(), img_dim)
    try:
        boxes = crop_boxes(hx, hy, sy, n)
        out = np.zeros((n, cropper.D, cropper.D, 1), np.uint8)
        for s in range(0, n, cropper.chunk):
            frames = read(s, min(cropper.chunk, n - s))
            _check_frames(frames)
            out[s:s + frames.shape[0]] = cropper.run(frames, boxes[s:s + frames.shape[0]])
    finally:
        if own:
            cropper.close()
    return out


def extract_body(df, video_path, out_path, img_dim=60, dev=None):
    """The reference's extract_body: for every video in video_path whose name matches Sample(\\d+)_ (sorted; .avi or .npy), write
    <name minus extension>.npy of shape (frames, img_dim, img_dim, 1) uint8 into out_path.  df: the skeletal DataFrame or the path of
    its CSV.  A video with no frames gives (0, img_dim, img_dim, 1) (the reference writes np.array([])).  Returns the written paths."""
    df = _read_skeletal(df)
    names = video_files(video_path)
    os.makedirs(out_path, exist_ok=True)
    cropper = _Cropper(dev or _device(), img_dim)
    written = []
    try:
        for name in names:
            dst = os.path.join(out_path, out_name(name))
            src = os.path.join(video_path, name)
            if os.path.abspath(dst) == os.path.abspath(src):
                raise ValueError("%s: the output would overwrite the input stack; choose another out_path" % src)
            np.save(dst, extract_video(df, src, cropper=cropper))
            written.append(dst)
    finally:
        cropper.close()
    return written


class RoiStore:
    """The crops extract_body would write for video_dir, computed on first request and kept (uint8): names() lists the .npy names,
    frames(name) returns (frames, img_dim, img_dim, 1) uint8.  rgb_network.DataGenerator(store=...) reads from it."""

    def __init__(self, video_dir, skeletal_csv, img_dim=60, dev=None):
        self.video_dir = video_dir
        self.img_dim = int(img_dim)
        self.df = _read_skeletal(skeletal_csv)
        self.dev = dev
        self._src = {out_name(n): n for n in video_files(video_dir)}
        self._cache = {}

    def names(self):
        return sorted(self._src)

    def frames(self, name):
        hit = self._cache.get(name)
        if hit is None:
            if name not in self._src:
                raise KeyError(name)
            hit = extract_video(self.df, os.path.join(self.video_dir, self._src[name]), self.img_dim, self.dev)
            self._cache[name] = hit
        return hit


def main(argv=None):
    """Replaces the reference's raw_input('Choose train or validation') prompt with explicit paths."""
    ap = argparse.ArgumentParser(description="upper-body crops of colour videos for the RGB network")
    ap.add_argument("--skeletal-csv", required=True, help="Training_set_skeletal.csv / Validation_set_skeletal.csv")
    ap.add_argument("--video-dir", required=True, help="SampleNNNNN_*.avi (raw bgr24) or .npy frame stacks")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--img-dim", type=int, default=60)
    a = ap.parse_args(argv)
    for p in extract_body(a.skeletal_csv, a.video_dir, a.out_dir, a.img_dim):
        print(p)


if __name__ == '__main__':
    main()
