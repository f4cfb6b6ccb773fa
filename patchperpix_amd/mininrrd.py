"""NRRD files without ``pynrrd``: the one form the `postprocess` task writes, and a reader for the tests.

The reference exports one skeleton per instance with ``nrrd.write(fn, mask.transpose(2, 1, 0))``
(PatchPerPix/util/postprocess.py:110-119): a uint8 mask, pynrrd's default Fortran index order and gzip
encoding.  Written in Fortran order the transposed (X, Y, Z) array is byte for byte the C-order
(Z, Y, X) mask, and the header lists the fastest axis first: ``sizes: X Y Z``.  ``write`` produces
exactly that: ``NRRD0004``, ``type: uint8``, ``dimension: 3``, ``sizes``, ``encoding: gzip``, a blank
line, the gzip stream.  pynrrd is absent here, so byte equality with ITS header text (field order,
comment lines, ``space`` fields it does not write for a bare array) is not a goal and is not checked;
any NRRD reader takes the fields above.
"""
import gzip

import numpy as np

MAGIC = "NRRD0004"


def write(path, mask, level=9):
    """``mask``: a (Z, Y, X) array, written as uint8 (non-zero -> its value as uint8; a bool mask -> 0 / 1)."""
    m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8, copy=False))
    if m.ndim != 3:
        raise ValueError("mininrrd.write takes a (Z, Y, X) array, not %d axes" % m.ndim)
    header = "\n".join([MAGIC, "type: uint8", "dimension: 3",
                        "sizes: %d %d %d" % (m.shape[2], m.shape[1], m.shape[0]), "encoding: gzip", "", ""])
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        # (mtime = 0: the same mask gives the same file)
        with gzip.GzipFile(fileobj=f, mode="wb", compresslevel=level, mtime=0) as z:
            z.write(m.tobytes())


def read(path):
    """(header fields as a dict of strings, the (Z, Y, X) array) of a file ``write`` made -- or any
    uint8 / gzip or raw NRRD with a ``sizes`` field."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"\n\n")
    lines = raw[:end].decode("ascii").split("\n")
    if not lines[0].startswith("NRRD"):
        raise ValueError("%s is not an NRRD file" % path)
    fields = {"magic": lines[0]}
    for line in lines[1:]:
        if line.startswith("#") or ": " not in line:
            continue
        k, v = line.split(": ", 1)
        fields[k] = v
    if fields.get("type") not in ("uint8", "unsigned char", "uchar"):
        raise NotImplementedError("type %r (uint8 only)" % fields.get("type"))
    payload = raw[end + 2:]
    if fields.get("encoding") in ("gzip", "gz"):
        payload = gzip.decompress(payload)
    elif fields.get("encoding") != "raw":
        raise NotImplementedError("encoding %r" % fields.get("encoding"))
    sizes = [int(v) for v in fields["sizes"].split()]
    return fields, np.frombuffer(payload, dtype=np.uint8).reshape(sizes[::-1])
