"""PNG files without scikit-image or Pillow: the forms the `visualize` task and ``save_mip`` write, and a
reader for the tests.

The reference saves its pictures with ``skimage.io.imsave`` (PatchPerPix/visualize/patches.py:191-195,
visualize/instances.py:79, vote_instances/stitch_patch_graph.py:823-847): uint8 arrays, (H, W) grey or
(H, W, 3) RGB.  ``write`` produces exactly those two: the 8-byte signature, IHDR (bit depth 8, colour type 0
or 2, no interlace), ONE IDAT chunk holding one zlib stream of the scanlines, each with filter type 0, and
IEND, every chunk with its CRC-32.  Byte equality with scikit-image's files (its compression level, its
ancillary chunks) is not a goal and cannot be checked here; the pixels any PNG reader decodes are.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def write(path, array, level=6):
    """``array``: uint8, (H, W) -> greyscale, (H, W, 3) -> RGB.  Any other dtype or shape raises: the
    caller casts, as the reference's callers do."""
    a = np.asarray(array)
    if a.dtype != np.uint8:
        raise TypeError("minipng.write takes uint8 pixels, not %s" % a.dtype)
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.size == 0:
        raise ValueError("minipng.write takes a non-empty (H, W) or (H, W, 3) array, not shape %s" % (a.shape,))
    h, w = int(a.shape[0]), int(a.shape[1])
    rows = np.ascontiguousarray(a).reshape(h, -1)
    # filter type 0 ("None") in front of every scanline
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rows], axis=1).tobytes()
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, level)) + _chunk(b"IEND", b""))


def read(path):
    """The (H, W) or (H, W, 3) uint8 array of a file ``write`` made -- or of any 8-bit grey / RGB PNG that is
    not interlaced and uses filter type 0 on every line.  A chunk whose CRC does not match raises ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != SIGNATURE:
        raise ValueError("%s is not a PNG file" % path)
    pos, ihdr, idat, ended = 8, None, [], False
    while pos < len(raw) and not ended:
        if pos + 12 > len(raw):
            raise ValueError("%s: truncated chunk" % path)
        (n,) = struct.unpack(">I", raw[pos:pos + 4])
        kind, payload = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        if pos + 12 + n > len(raw):
            raise ValueError("%s: truncated chunk %r" % (path, kind))
        (crc,) = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + payload) & 0xFFFFFFFF):
            raise ValueError("%s: CRC mismatch in chunk %r" % (path, kind))
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", payload)
        elif kind == b"IDAT":
            idat.append(payload)
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if ihdr is None or not ended:
        raise ValueError("%s: IHDR or IEND missing" % path)
    w, h, depth, ctype, comp, flt, interlace = ihdr
    if depth != 8 or ctype not in (0, 2) or comp != 0 or flt != 0 or interlace != 0:
        raise NotImplementedError("bit depth %d, colour type %d, interlace %d (8-bit grey / RGB only)" % (depth, ctype, interlace))
    ch = 1 if ctype == 0 else 3
    lines = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if lines.size != h * (1 + w * ch):
        raise ValueError("%s: %d bytes of scanlines, %d expected" % (path, lines.size, h * (1 + w * ch)))
    lines = lines.reshape(h, 1 + w * ch)
    if lines[:, 0].any():
        raise NotImplementedError("scanline filters other than 0")
    px = lines[:, 1:].copy()
    return px.reshape(h, w) if ch == 1 else px.reshape(h, w, 3)
