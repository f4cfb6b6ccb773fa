"""The patch mosaic of the reference's `visualize` task (PatchPerPix/visualize/patches.py): every voxel's
predicted patch shown as one tile of a large image, under the reference's names and kwargs.

The reference builds the mosaic with a Python loop over the voxels.  It is a pure re-arrangement, defined
here once as `mosaic_host` (vectorised NumPy) and computed by the HIP kernel of csrc/ppp_mosaic.hip
(`backend.patch_mosaic`) when there is a device:

    3-d, patch (pz, py, px), input (C, Z, Y, X), C = pz py px, output (Z, Y py, X px):
        out[z, y py + j, x px + i] = 1                                          if j == 0 or i == 0
                                   = max over k of in[(k py + j) px + i, z, y, x]   otherwise   (NumPy's max: NaN wins)
    2-d: pz = 1 and Z = 1, output (1, Y py, X px); with `selected` three output channels, see `mosaic_host`.

The reference writes the ones of row 0 / column 0 into its INPUT array; here the input is read-only.

Dispatch (no switch of its own): the device when there is one and ``PPP_POSTPROCESS`` is not ``host`` --
`postprocess.use_device`, the rule of the other post-steps -- else `mosaic_host`.  A file is read in
z-chunks through the project's container readers, each chunk uploaded, arranged and downloaded; input
chunk + output chunk stay within `HBM_SHARE` of the free device memory, and the result does not depend on
the chunking (a slice of the output depends on the same slice of the input only).

The post-steps of `visualize_patches` (threshold, float16 -> float32, store_int, the uint8 cast of a PNG)
are the reference's NumPy expressions, literally, on the host: their dtype results are NumPy's promotion.
"""
import logging

import numpy as np

from .. import postprocess
from ..vote_instances import io_hdflike

logger = logging.getLogger(__name__)

HBM_SHARE = 0.25     # of the free device memory, for one input chunk and its output chunk


def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "is_cuda")


def _patch_sides(patchshape):
    """the sides > 1 of `patchshape`, as the reference filters them (patches.py:13-15)"""
    ps = np.array(patchshape)
    return [int(p) for p in ps[ps > 1]]


# ----------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------
def mosaic_host(in_array, patch, selected=None):
    """The definition, vectorised: `in_array` (C, Z, Y, X) NumPy, `patch` = (pz, py, px) with C = pz py px,
    `selected` None or (S, Z, Y, X) with S = 1 or 3 (pz = 1).  Returns (Z, Y py, X px) of the input's dtype;
    with `selected` (3, Z, Y py, X px): the tile of a voxel goes to ONE channel -- S = 1: channel 0 where
    selected[0] is set, else channel 2; S = 3: the first of channels 0, 1, 2 whose flag is set, none where no
    flag is -- and the other channels stay 0 there.  The input is not written to."""
    a = np.asarray(in_array)
    pz, py, px = [int(p) for p in patch]
    if a.ndim != 4 or a.shape[0] != pz * py * px:
        raise ValueError("mosaic_host needs (C, Z, Y, X) with C = %d x %d x %d, got shape %s" % (pz, py, px, a.shape))
    C, Z, Y, X = a.shape
    m = np.max(a.reshape(pz, py, px, Z, Y, X), axis=0)          # a new array: (py, px, Z, Y, X)
    m[0, :] = 1
    m[:, 0] = 1
    out = np.ascontiguousarray(m.transpose(2, 3, 0, 4, 1)).reshape(Z, Y * py, X * px)
    if selected is None:
        return out
    sel = np.asarray(selected) != 0
    if pz != 1 or sel.ndim != 4 or sel.shape[0] not in (1, 3) or sel.shape[1:] != (Z, Y, X):
        raise ValueError("selected must be (1 or 3, Z, Y, X) and pz = 1, got shape %s" % (sel.shape,))
    if sel.shape[0] == 1:
        route = np.where(sel[0], 0, 2)
    else:
        route = np.where(sel[0], 0, np.where(sel[1], 1, np.where(sel[2], 2, 3)))
    route = np.repeat(np.repeat(route, py, axis=1), px, axis=2)
    return np.stack([np.where(route == ch, out, np.zeros((), dtype=out.dtype)) for ch in range(3)])


# ----------------------------------------------------------------------------------------
# the device path
# ----------------------------------------------------------------------------------------
def z_chunk(Z, C, Y, X, patch, itemsize, channels, free_bytes, share=HBM_SHARE):
    """slices per chunk such that the input chunk, its output chunk and the selected block fit `share` of
    `free_bytes`; at least one"""
    per_slice = Y * X * (C * itemsize + channels * patch[1] * patch[2] * itemsize + (3 if channels == 3 else 0))
    return max(1, min(int(Z), int(share * free_bytes) // max(int(per_slice), 1)))


def mosaic_device(read_tile, shape, dtype, patch, selected=None, tz=None):
    """The mosaic of a prediction of `shape` = (C, Z, Y, X) and NumPy `dtype` that `read_tile(z, n)` hands out as
    (C, n, Y, X) NumPy arrays, a z-chunk at a time: upload, `backend.patch_mosaic`, download.  `tz`: slices per
    chunk (default: by `z_chunk` from the free device memory).  Returns the NumPy array `mosaic_host` returns."""
    import torch
    from .. import backend
    C, Z, Y, X = [int(s) for s in shape]
    dtype = np.dtype(dtype)
    channels = 1 if selected is None else 3
    if tz is None:
        tz = z_chunk(Z, C, Y, X, patch, dtype.itemsize, channels, torch.cuda.mem_get_info()[0])
    plane = (Z, Y * patch[1], X * patch[2])
    out = np.empty(plane if selected is None else (3,) + plane, dtype=dtype)
    for z in range(0, Z, tz):
        n = min(tz, Z - z)
        d_tile = torch.from_numpy(np.array(read_tile(z, n), dtype=dtype, order="C")).cuda()
        d_sel = None
        if selected is not None:
            d_sel = torch.from_numpy(np.ascontiguousarray((np.asarray(selected)[:, z:z + n] != 0).astype(np.uint8))).cuda()
        res = backend.patch_mosaic(d_tile, patch, d_sel).cpu().numpy()
        if selected is None:
            out[z:z + n] = res
        else:
            out[:, z:z + n] = res
    return out


def _mosaic(arr4, patch, selected=None):
    """`arr4` (C, Z, Y, X), NumPy or tensor, by the dispatch rule; the same kind comes back"""
    C = int(arr4.shape[0])
    if C != patch[0] * patch[1] * patch[2]:
        raise ValueError("%d channels, but the patch %s has %d elements" % (C, tuple(patch), patch[0] * patch[1] * patch[2]))
    if _is_tensor(arr4):
        import torch
        if arr4.is_cuda:
            from .. import backend
            d_sel = None
            if selected is not None:
                d_sel = torch.from_numpy(np.ascontiguousarray((np.asarray(selected) != 0).astype(np.uint8))).to(arr4.device)
            return backend.patch_mosaic(arr4.contiguous(), patch, d_sel)
        bf16 = arr4.dtype == torch.bfloat16                     # (NumPy has no bfloat16: float32 holds it exactly)
        res = _mosaic((arr4.float() if bf16 else arr4).numpy(), patch, selected)
        res = torch.from_numpy(res)
        return res.to(torch.bfloat16) if bf16 else res
    arr4 = np.asarray(arr4)
    # (the kernel has the three element types of a prediction; any other dtype -- the float64 that
    # scipy.special.expit makes of float16 logits -- is arranged by the definition on the host)
    if postprocess.use_device() and arr4.dtype in (np.float32, np.float16):
        return mosaic_device(lambda z, n: arr4[:, z:z + n], arr4.shape, arr4.dtype, patch, selected)
    return mosaic_host(arr4, patch, selected)


def _read_selected(selected):
    """the reference's `selected`: an .hdf file with the dataset 'selected' (patches.py:17-19); an array goes as it is"""
    if selected is None or not isinstance(selected, str):
        return selected
    with io_hdflike.open_container(selected, "r") as f:
        return np.array(f["selected"])


def reshape_affinities(in_array, patchshape, selected=None):
    """patches.py:12-70: the 2-d mosaic.  `in_array` (C, Y, X), `patchshape` with two sides > 1; returns
    (1, Y py, X px), or (3, Y py, X px) with `selected` ((1 or 3, Y, X), or the .hdf file that holds it)."""
    sides = _patch_sides(patchshape)
    if len(sides) != 2:
        raise NotImplementedError("reshape_affinities serves patches with two sides > 1, got %s" % (list(patchshape),))
    if len(in_array.shape) != 3:
        raise ValueError("reshape_affinities needs a (C, Y, X) array, got shape %s" % (tuple(in_array.shape),))
    patch = (1, sides[0], sides[1])
    sel = _read_selected(selected)
    if sel is not None:
        sel = np.asarray(sel)
        if sel.ndim != 3 or sel.shape[0] not in (1, 3) or tuple(sel.shape[1:]) != tuple(in_array.shape[1:]):
            raise ValueError("selected must be (1 or 3, Y, X), got shape %s" % (sel.shape,))
        sel = sel[:, None]
    res = _mosaic(in_array[:, None], patch, sel)
    return res if sel is None else res[:, 0]


def reshape_affinities_3d(in_array, patchshape):
    """patches.py:73-98: the 3-d mosaic with the maximum along the patch's z.  `in_array` (C, Z, Y, X),
    `patchshape` with three sides > 1; returns (Z, Y py, X px)."""
    sides = _patch_sides(patchshape)
    if len(sides) != 3:
        raise NotImplementedError("reshape_affinities_3d serves patches with three sides > 1, got %s" % (list(patchshape),))
    if len(in_array.shape) != 4:
        raise ValueError("reshape_affinities_3d needs a (C, Z, Y, X) array, got shape %s" % (tuple(in_array.shape),))
    return _mosaic(in_array, tuple(sides))


def _mosaic_3d_from_dataset(ds, sides):
    """the 3-d mosaic of a container dataset, read z-chunk by z-chunk (unit axes dropped like np.squeeze)"""
    full = tuple(int(s) for s in ds.shape)
    axes = [a for a, s in enumerate(full) if s != 1]
    C = sides[0] * sides[1] * sides[2]
    if len(axes) != 4 or full[axes[0]] != C:
        raise ValueError("a dataset of shape %s is no (C = %d, Z, Y, X) prediction" % (full, C))
    Z, Y, X = (full[a] for a in axes[1:])

    def read_tile(z, n):
        sel = [slice(None)] * len(full)
        sel[axes[1]] = slice(z, z + n)
        return np.ascontiguousarray(np.asarray(ds[tuple(sel)]).reshape(C, n, Y, X))
    dtype = np.dtype(ds.dtype)
    if postprocess.use_device() and dtype in (np.float32, np.float16):
        return mosaic_device(read_tile, (C, Z, Y, X), dtype, tuple(sides))
    return mosaic_host(read_tile(0, Z), tuple(sides))


def png_pixels(patched, rgb=False):
    """patches.py:192-193, literally; then the shapes a PNG can hold: 2-d, or -- `rgb`, the `selected` form --
    (3, H, W) as RGB (H, W, 3)"""
    patched = (patched * 255).astype(np.uint8)
    patched = np.squeeze(patched)
    if rgb and patched.ndim == 3 and patched.shape[0] == 3:
        return np.ascontiguousarray(np.moveaxis(patched, 0, -1))
    if patched.ndim != 2:
        raise ValueError("a mosaic of shape %s is no picture: a .png holds a 2-d mosaic or the 3 channels of "
                         "`selected`" % (patched.shape,))
    return patched


def visualize_patches(affinities, patchshape, in_key=None, out_file=None, out_key=None, threshold=None,
                      selected=None, sigmoid=False, store_int=False):
    """patches.py:101-203.  `affinities`: a ``.zarr`` / ``.hdf`` file (with `in_key`, a string or a list), a
    NumPy array, or a device tensor.  `patchshape`: two sides > 1 -- the 2-d mosaic of a (C, Y, X) array,
    channels-last (Y, X, C) moved to the front by the reference's own test, `sigmoid` applying
    ``scipy.special.expit`` first, `selected` routing the tiles -- or three, the 3-d mosaic of (C, Z, Y, X).
    Then ``patched[patched < threshold] = 0``; for an ``.hdf`` `out_file` float16 -> float32, `store_int`'s
    ``(patched * 255).astype(np.uint8)`` and a gzip dataset ``out_key[i]`` (default ``in_key[i] + '_patched'``);
    for a ``.png`` the uint8 picture (minipng).  ``.tif`` and every other target raise NotImplementedError.
    Returns the array (a device tensor for a device tensor) when there is no `out_file`, else 0."""
    import scipy.special
    from .. import minipng
    tensor_in = _is_tensor(affinities)
    if isinstance(affinities, str):
        if not affinities.rstrip("/").endswith((".zarr", ".hdf")):
            raise NotImplementedError("visualize_patches reads .zarr and .hdf files, not %s" % affinities)
        assert in_key is not None, "Please provide a key, if affinities are loaded from file."
    elif not (isinstance(affinities, np.ndarray) or tensor_in):
        raise NotImplementedError("visualize_patches takes a file name, a NumPy array or a tensor, not %s" % type(affinities))
    if out_file is not None:
        if out_file.endswith(".tif"):
            raise NotImplementedError("a .tif target is not provided by this repository (there is no TIFF writer)")
        if not out_file.endswith((".hdf", ".png")):
            raise NotImplementedError("visualize_patches writes .hdf and .png files, not %s" % out_file)
    if in_key is not None:
        if type(in_key) not in [list, tuple]:
            in_key = list([in_key])
        if out_key is not None and type(out_key) not in [list, tuple]:
            out_key = list([out_key])
    sides = _patch_sides(patchshape)
    if len(sides) not in (2, 3):
        raise NotImplementedError("a patch needs two or three sides > 1, got %s" % (list(np.array(patchshape)),))
    keys = in_key if isinstance(affinities, str) else [None]

    for i, key in enumerate(keys):
        with (io_hdflike.open_container(affinities, "r") if key is not None else _nothing()) as inf:
            if len(sides) == 3 and key is not None:
                patched = _mosaic_3d_from_dataset(inf[key], sides)
            else:
                if key is not None:
                    labels = np.squeeze(np.array(inf[key]))
                elif tensor_in:
                    labels = affinities.squeeze()
                else:
                    labels = np.squeeze(affinities)
                if len(sides) == 2:
                    patchsize = sides[0] * sides[1]
                    # CHW vs HWC (patches.py:154-155)
                    if labels.shape[0] != patchsize and labels.shape[-1] == patchsize:
                        labels = labels.movedim(-1, 0).contiguous() if tensor_in else \
                            np.ascontiguousarray(np.moveaxis(labels, -1, 0))
                    if sigmoid:
                        labels = labels.sigmoid() if tensor_in else scipy.special.expit(labels)
                    patched = reshape_affinities(labels, sides, selected=selected)
                else:
                    patched = reshape_affinities_3d(labels, sides)

        if _is_tensor(patched):
            if threshold is None and out_file is None:
                return patched
            device, bf16 = patched.device, str(patched.dtype) == "torch.bfloat16"
            patched = (patched.float() if bf16 else patched).cpu().numpy()     # (float32 holds bfloat16 exactly)
        else:
            device = None

        if threshold is not None:
            patched[patched < threshold] = 0

        if out_file is None:
            if device is not None:
                import torch
                patched = torch.from_numpy(patched).to(device)
                return patched.to(torch.bfloat16) if bf16 else patched
            return patched
        if out_file.endswith(".hdf"):
            if out_key is None:
                if in_key is None:
                    raise ValueError("an .hdf target needs out_key, or in_key for the default in_key + '_patched'")
                c_out_key = in_key[i] + "_patched"
            else:
                c_out_key = out_key[i]
            if patched.dtype == np.float16:
                patched = patched.astype(np.float32)
            if store_int:
                patched = (patched * 255).astype(np.uint8)
            with io_hdflike.open_container(out_file, "a") as outf:
                outf.create_dataset(c_out_key, data=patched, compression="gzip")
        else:
            minipng.write(out_file, png_pixels(patched, rgb=selected is not None and len(sides) == 2))
    return 0


class _nothing:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False
