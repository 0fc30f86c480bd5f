"""A minimal uncompressed AVI writer for the tests of rgb_network/roi_extraction.py's reader: BI_RGB frames in '00db' / '00dc' chunks,
optional odd-sized JUNK, 'ix00' and LIST 'rec ' chunks inside 'movi', an idx1 index and OpenDML RIFF 'AVIX' continuations."""
import struct

import numpy as np


def _chunk(tag, data):
    return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _list(kind, body):
    return _chunk(b"LIST", kind + body)


def write_avi(path, frames, bottom_up=True, tag=b"00db", junk=b"odd", ix=True, rec=False, avix_at=None, bits=24, compression=0,
              audio=False):
    """frames (n, h, w, 3) uint8 BGR, top row first.  bits / compression other than 24 / 0 write a header only a refusing reader
    accepts (the frame bytes are then whatever fits the header).  avix_at=k puts frames k.. into a RIFF 'AVIX' continuation.
    audio=True declares a second stream and puts '01wb' chunks between the frames."""
    frames = np.asarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    bpp = bits // 8
    stride = (bpp * w + 3) & ~3
    size_image = stride * h

    def frame_bytes(img):
        rows = np.zeros((h, stride), np.uint8)
        if bpp == 3:
            rows[:, :3 * w] = img.reshape(h, 3 * w)
        else:
            px = np.zeros((h, w, bpp), np.uint8)
            px[:, :, :3] = img
            rows[:, :bpp * w] = px.reshape(h, bpp * w)
        return (rows[::-1] if bottom_up else rows).tobytes()

    avih = struct.pack("<14I", 40000, 0, 0, 0x10, n, 0, 2 if audio else 1, size_image, w, h, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"DIB ", 0, 0, 0, 0, 1, 25, 0, n, size_image, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHHIIiiII", 40, w, h if bottom_up else -h, 1, bits, compression, size_image, 0, 0, 0, 0)
    strls = _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf))
    if audio:
        ash = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 0, 4096, 0xFFFFFFFF, 2, 0, 0, 0, 0)
        strls += _list(b"strl", _chunk(b"strh", ash) + _chunk(b"strf", struct.pack("<HHIIHH", 1, 1, 8000, 16000, 2, 16)))
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + strls)

    def movi(idx):
        body = b""
        for i in idx:
            c = _chunk(tag, frame_bytes(frames[i]))
            body += _list(b"rec ", c) if rec else c
            if audio:
                body += _chunk(b"01wb", b"\1\2\3")
        if ix:
            body += _chunk(b"ix00", b"\0" * 24)
        return _list(b"movi", body)

    split = n if avix_at is None else avix_at
    junk_chunk = _chunk(b"JUNK", b"\0" * (7 if junk == b"odd" else 8)) if junk else b""
    first = b"AVI " + hdrl + junk_chunk + movi(range(split)) + _chunk(b"idx1", b"\0" * 16 * split)
    data = _chunk(b"RIFF", first)
    if avix_at is not None:
        data += _chunk(b"RIFF", b"AVIX" + movi(range(split, n)))
    with open(path, "wb") as f:
        f.write(data)
    return path
