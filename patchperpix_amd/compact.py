"""A prediction kept as ROWS for the foreground voxels only.

``decode`` leaves the background of the (C, Z, Y, X) prediction zero by definition
(``decode.decode_volume``), and flylight volumes are a few percent foreground: the dense block
is 30 times the data.  ``CompactPrediction`` holds the table ``rows [n, C]`` -- row k belongs to the
k-th voxel of ``mask`` in raster order (x fastest) -- and is a PROVIDER of ``tiling.assemble``:
``pred_box(box)`` expands the dense box a tile needs on the device (``ppp_rows_expand``,
csrc/ppp_rows.hip), zero outside the mask.  What it stands for is the dense array D, zero outside
``mask`` with ``rows[k]`` at the k-th mask voxel; a vote on it is the vote on D, tile for tile the
same tensors the voting kernels would read from D.

With the rows on the CPU, plain torch indexing does the same (the CPU tests of the tiled assembly with
``OracleOps``); production keeps the rows in HBM.
"""
import numpy as np

from . import backend


def _torch():
    import torch
    return torch


class CompactPrediction:
    """rows [n, C] device (or CPU) tensor; mask (Z, Y, X), non-zero = has a row; expit: the rows are
    float16 logits and pred_box() returns the float32 logistic of them at the mask voxels (what
    ``DecodeProvider`` does after decoding), 0 elsewhere."""

    def __init__(self, rows, mask, patchshape=None, expit=False, index=None):
        torch = _torch()
        if rows.dim() != 2:
            raise ValueError("CompactPrediction: rows must be [n, C], got %s" % (tuple(rows.shape),))
        self.rows = rows.contiguous()
        dev = self.rows.device
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        if m.dim() != 3:
            raise ValueError("CompactPrediction: mask must be (Z, Y, X), got %s" % (tuple(m.shape),))
        self.mask = (m != 0).to(torch.uint8).to(dev).contiguous()
        self.shape = tuple(int(v) for v in self.mask.shape)
        self.C = int(self.rows.shape[1])
        if patchshape is not None and int(np.prod(patchshape)) != self.C:
            raise ValueError("CompactPrediction: rows of %d values, patches of %s" % (self.C, tuple(patchshape)))
        self.patchshape = None if patchshape is None else tuple(int(p) for p in patchshape)
        self.expit = bool(expit)
        if self.expit and self.rows.dtype != torch.float16:
            raise ValueError("CompactPrediction: expit is defined for float16 logits (loadAffinities reads float16)")
        if self.rows.is_cuda:
            if index is None:
                index, n = backend.rows_index_build(self.mask)
            else:
                n = int(self.rows.shape[0])
            self.index = index
        else:
            self.index = None
            n = int(self.mask.sum())
        if n != int(self.rows.shape[0]):
            raise ValueError("CompactPrediction: %d rows for a mask of %d voxels" % (int(self.rows.shape[0]), n))

    # ---- construction ------------------------------------------------------------------------
    @classmethod
    def from_rows(cls, rows, mask, patchshape=None, expit=False):
        return cls(rows, mask, patchshape, expit)

    @classmethod
    def empty(cls, mask, C, dtype, device, patchshape=None, expit=False):
        """the rows allocated (uninitialised) for `mask`: filled by the caller (decode_rows, from_dense)"""
        torch = _torch()
        device = torch.device(device)
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        m = (m != 0).to(torch.uint8).to(device).contiguous()
        if device.type == "cuda":
            index, n = backend.rows_index_build(m)
        else:
            index, n = None, int(m.sum())
        rows = torch.empty((n, int(C)), dtype=dtype, device=device)
        return cls(rows, m, patchshape, expit, index=index)

    @classmethod
    def from_dense(cls, pred, mask, patchshape=None, expit=False, shape=None, C=None, dtype=None, device=None,
                   box_voxels=1 << 21):
        """pred: a (C, Z, Y, X) tensor, or any provider (``pred_box(box)``; then C, dtype and device
        say what it returns).  Compacted box by box of about `box_voxels` voxels (whole z-slices)
        with ppp_rows_compact: a provider's prediction is never resident as a whole."""
        torch = _torch()
        tensor = torch.is_tensor(pred)
        if tensor:
            C, dtype, device = int(pred.shape[0]), pred.dtype, pred.device
        elif C is None or dtype is None:
            raise ValueError("from_dense: a provider needs C and dtype")
        self = cls.empty(mask, C, dtype, device if device is not None else "cuda", patchshape, expit)
        Z, Y, X = self.shape
        if tensor and tuple(int(v) for v in pred.shape[1:]) != self.shape:
            raise ValueError("from_dense: prediction %s, mask %s" % (tuple(pred.shape), self.shape))
        step = max(1, int(box_voxels) // max(1, Y * X))
        for z0 in range(0, Z, step):
            box = (z0, min(Z, z0 + step), 0, Y, 0, X)
            blk = pred[:, box[0]:box[1]] if tensor else pred.pred_box(box)
            self._compact_box(blk.contiguous(), box)
        return self

    def _compact_box(self, blk, box):
        if self.rows.is_cuda:
            backend.rows_compact(blk, box, self.index, self.shape, self.rows)
            return
        z0, z1, y0, y1, x0, x1 = box
        m = self.mask[z0:z1, y0:y1, x0:x1] != 0
        k = self._row_numbers()[z0:z1, y0:y1, x0:x1][m]
        self.rows[k] = blk[:, m].t().to(self.rows.dtype)

    def _row_numbers(self):
        """CPU form only: the row number of every voxel (raster order = cumulative sum of the flat mask)"""
        torch = _torch()
        if getattr(self, "_rownum", None) is None:
            flat = self.mask.reshape(-1).to(torch.int64)
            self._rownum = (torch.cumsum(flat, 0) - flat).reshape(self.shape)
        return self._rownum

    # ---- the provider protocol ---------------------------------------------------------------
    def pred_box(self, box):
        torch = _torch()
        z0, z1, y0, y1, x0, x1 = [int(v) for v in box]
        if self.rows.is_cuda:
            out = backend.rows_expand(self.rows, self.index, self.shape, (z0, z1, y0, y1, x0, x1))
        else:
            m = self.mask[z0:z1, y0:y1, x0:x1] != 0
            out = torch.zeros((self.C, z1 - z0, y1 - y0, x1 - x0), dtype=self.rows.dtype)
            out[:, m] = self.rows[self._row_numbers()[z0:z1, y0:y1, x0:x1][m]].t()
        if not self.expit:
            return out
        # float16 logits -> float64 logistic -> float32 at the mask voxels of the box, 0 elsewhere:
        # DecodeProvider.pred_box, statement for statement
        res = torch.zeros(out.shape, dtype=torch.float32, device=out.device)
        dst = torch.nonzero(self.mask[z0:z1, y0:y1, x0:x1].reshape(-1)).reshape(-1)
        if dst.numel():
            flat, oflat = out.reshape(self.C, -1), res.reshape(self.C, -1)
            step = max(1, (1 << 24) // max(1, int(dst.numel())))
            for c0 in range(0, self.C, step):
                oflat[c0:c0 + step, dst] = torch.sigmoid(flat[c0:c0 + step, dst].double()).float()
        return res

    def to_dense(self):
        Z, Y, X = self.shape
        return self.pred_box((0, Z, 0, Y, 0, X))

    # ---- sizes ---------------------------------------------------------------------------------
    @property
    def n_rows(self):
        return int(self.rows.shape[0])

    @property
    def nbytes(self):
        """rows + index + mask, as resident"""
        n = int(self.rows.numel()) * int(self.rows.element_size()) + int(self.mask.numel())
        return n + (int(self.index.numel()) if self.index is not None else 0)

    @property
    def dense_dtype(self):
        torch = _torch()
        return torch.float32 if self.expit else self.rows.dtype

    @property
    def dense_nbytes(self):
        torch = _torch()
        return self.C * int(np.prod(self.shape)) * torch.empty((), dtype=self.dense_dtype).element_size()


def vote(cp, foreground, mask_to_cover, numinst, patchshape, **kwargs):
    """to_instance_seg on a CompactPrediction: expanded once and voted resident when the dense block
    takes at most half of the free HBM (the rule of ``tiling._want_stream``), else planned into tiles
    like ``tiling._stitch_streamed`` -- free HBM read now, with the rows resident -- and assembled
    through the provider.  ``_n_slabs`` / ``_yx_tiles`` are honoured on both paths."""
    torch = _torch()
    from . import tiling
    from .vote_instances import vote_instances as vi
    if not kwargs.get("cuda", False):
        raise NotImplementedError("a CompactPrediction is voted on the device: cuda=False (the reference's NumPy "
                                  "semantics) is not implemented for a compact prediction")
    if int(np.prod(patchshape)) != cp.C:
        raise ValueError("compact prediction: rows of %d values, patches of %s" % (cp.C, tuple(int(p) for p in patchshape)))
    if not cp.rows.is_cuda:
        raise NotImplementedError("to_instance_seg needs the rows of a compact prediction on the device "
                                  "(CPU rows serve tiling.assemble with host ops only)")
    if tuple(int(v) for v in np.shape(foreground)) != cp.shape:
        raise ValueError("compact prediction of %s, fields of %s" % (cp.shape, tuple(np.shape(foreground))))
    # `_compact_resident` (private, like `_n_slabs`): True / False decides instead of the rule
    resident = kwargs.pop("_compact_resident", None)
    if resident is None:
        resident = cp.dense_nbytes <= 0.5 * torch.cuda.mem_get_info()[0]
    if resident:
        return vi._to_instance_seg(cp.to_dense(), foreground, mask_to_cover, numinst, patchshape, **kwargs)
    if kwargs.get("pad_with_ps", False) or kwargs.get("independent_slices", False):
        raise NotImplementedError("pad_with_ps / independent_slices are not supported by the tiled / multi-rank assembly")
    if not kwargs.get("blockwise", False) and kwargs.get("skeletonize_foreground"):
        mask_to_cover = vi._skeletonize(mask_to_cover, kwargs.get("skeletonize_backend"))
    n_slabs, yx = kwargs.get("_n_slabs"), kwargs.get("_yx_tiles")
    if n_slabs is None:
        avail = torch.cuda.mem_get_info()[0]
        n_slabs, ny, nx = tiling.tiles_needed(cp.shape, patchshape, max(avail - 120.0 * float(np.prod(cp.shape)) - 8e9, 0.25 * avail),
                                              safety=0.8 if cp.expit else 0.9, copies=2.0)
        if yx is None:
            yx = (ny, nx)
    kw = {k: v for k, v in kwargs.items() if k not in ("_n_slabs", "_yx_tiles")}
    if yx:
        kw["_yx_tiles"] = tuple(int(v) for v in yx)
    return tiling.assemble(cp, 0, cp.shape, foreground, mask_to_cover, numinst, patchshape,
                           tiling.plan_slabs(cp.shape[0], int(n_slabs)), **kw)
