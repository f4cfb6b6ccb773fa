"""The ground-truth patch affinities of a label volume, under the names of the reference's
PatchPerPix/util/train_util.py:349-775 (the `seg_to_affgraph_*_torch*` family, the BCE target of the patch loss
that torch_model.py:201-223 binds to `self.compute_affinities`).

The reference loops over the E edges in Python with about ten torch launches per edge, and over the samples
to slice one patch each.  Here a device tensor goes to ONE kernel launch (csrc/ppp_gt_affs.hip through
`backend.gt_affs_dense` / `backend.gt_affs_samples`); a CPU tensor or a NumPy array goes to the NumPy
definition in this module, `gt_affs_dense_host` / `gt_affs_samples_host`.  The result lives where `seg` lives
(a NumPy array for a NumPy `seg`); `device` is accepted for the reference's signature and not used.

Definitions.  Labels are integers, 0 is background, every other value is an id, negative
ones included: only equality and `!= 0` are used.  Any integer or bool label type is narrowed to int32.

  dense, multi-channel   seg (B, L, Z, Y, X) / (B, L, Y, X), nhood (E, 3) / (E, 2) offsets of any integers.
        aff[b, e, v] = 1 iff v + nhood[e] lies inside the volume and some channel c has seg[b, c, v] != 0 and
        seg[b, c, v] == seg[b, c, v + nhood[e]] -- the same id in the SAME channel -- else 0.  An offset as long
        as an axis or longer gives zeros (the reference raises beyond |n| == S).
  dense, one channel     seg (B, Z, Y, X) / (B, Y, X).  aff[b, e, v] = float32(c * c), c = seg[b, v], where
        c == seg[b, v + nhood[e]], else 0: the id SQUARED, for the reference multiplies by the label values.
        The product is the reference's 32-bit one, so the form is defined for |id| <= 46340.
  sampled, multi-channel samples_loc (N, 1 + d) rows (b, z, y, x) -- (N, d) plus `b` in the `_batch` forms --
        name the CORNER of a cubic patch P of side ps; nhood[e] is an index INTO the patch (negative entries
        from the end, as torch indexes: `% ps`), the centre is (psH, ...).  aff[n, e] = 1 iff some c has
        P[c, ctr] != 0 and P[c, ctr] == P[c, nhood[e]].  (N, E) float32; N = 0 gives (0, E).
  sampled, one channel   neither form can run in the reference (the 3-d one indexes the whole batch where it
        means the patches, the 2-d one uses an undefined name): NotImplementedError, no meaning is invented.

Keywords of this project's own: `check=True` validates in ONE synchronisation -- sample patches inside the
volume, ids that fit int32, |id| <= 46340 in the one-channel forms -- and raises ValueError; `check=False`
skips it (a training loop that has validated its data once).  `box=` (dense forms: z0, z1, y0, y1, x0, x1, or
y0, y1, x0, x1 in 2-d) writes only that part, what torch_model.py:432-441 crops; `out_dtype=` (multi forms:
float32 / float16 / bfloat16)."""
import numpy as np

MAX_SINGLE_ID = 46340            # c * c < 2^31


# ----------------------------------------------------------------------------------------
# the NumPy definitions
# ----------------------------------------------------------------------------------------
def gt_affs_dense_host(seg, nhood, box=None, single=False):
    """The dense definition: `seg` int (B, L, Z, Y, X) -- (B, Z, Y, X) with `single` -- `nhood` (E, 3) of any
    integers, `box` = (z0, z1, y0, y1, x0, x1) or None.  One shifted compare per edge.  float32
    (B, E, z1-z0, y1-y0, x1-x0)."""
    seg = np.asarray(seg)
    if seg.dtype != np.int32:
        seg = seg.astype(np.int32)
    if single:
        seg = seg[:, None]
    if seg.ndim != 5:
        raise ValueError("labels of shape %s: (B, L, Z, Y, X), or (B, Z, Y, X) with single" % (seg.shape,))
    nhood = np.asarray(nhood, dtype=np.int64).reshape(-1, 3)
    B, size = seg.shape[0], seg.shape[2:]
    box = (0, size[0], 0, size[1], 0, size[2]) if box is None else tuple(int(v) for v in box)
    lo0, hi0 = box[0::2], box[1::2]
    if any(a < 0 or b > s or a >= b for a, b, s in zip(lo0, hi0, size)):
        raise ValueError("box %s is empty or leaves the volume %s" % (box, tuple(size)))
    out = np.zeros((B, len(nhood)) + tuple(b - a for a, b in zip(lo0, hi0)), dtype=np.float32)
    for e, n in enumerate(nhood):
        # the centres of the box whose neighbour lies inside the volume
        lo = [max(a, -int(d)) for a, d in zip(lo0, n)]
        hi = [min(b, s - int(d)) for b, s, d in zip(hi0, size, n)]
        if any(a >= b for a, b in zip(lo, hi)):
            continue
        c = seg[(slice(None), slice(None)) + tuple(slice(a, b) for a, b in zip(lo, hi))]
        o = seg[(slice(None), slice(None)) + tuple(slice(a + int(d), b + int(d)) for a, b, d in zip(lo, hi, n))]
        if single:
            val = np.where(c == o, c * c, 0)[:, 0]               # the int32 product
        else:
            val = ((c == o) & (c != 0)).any(axis=1)
        out[(slice(None), e) + tuple(slice(a - a0, b - a0) for a, b, a0 in zip(lo, hi, lo0))] = val
    return out


def gt_affs_samples_host(seg, samples, nhood, ps, ctr):
    """The sampled definition: `seg` int (B, L, Z, Y, X), `samples` (N, 4) rows (b, z, y, x), `nhood` (E, 3)
    indices into the patch of `ps` = (pz, py, px), `ctr` the centre's index.  A voxel outside the volume reads
    as 0, as does an index outside [0, ps) and a row whose b is outside [0, B) (the C entry point's rule; the
    reference raises there, and so do this module's functions under `check`).  float32 (N, E)."""
    seg = np.asarray(seg)
    if seg.dtype != np.int32:
        seg = seg.astype(np.int32)
    samples = np.asarray(samples, dtype=np.int64).reshape(-1, 4)
    nhood = np.asarray(nhood, dtype=np.int64).reshape(-1, 3)
    B, size = seg.shape[0], np.array(seg.shape[2:])
    ps, ctr = np.array(ps, dtype=np.int64), np.array(ctr, dtype=np.int64)

    def read(pos, ok):
        """labels (..., L) at positions `pos` (..., 3) of the rows' batch items, 0 where not `ok`"""
        ok = ok & (pos >= 0).all(axis=-1) & (pos < size).all(axis=-1)
        p = np.where(ok[..., None], pos, 0)
        b = np.broadcast_to(np.where(bok, samples[:, 0], 0).reshape((-1,) + (1,) * (pos.ndim - 2)), ok.shape)
        vals = seg[b, :, p[..., 0], p[..., 1], p[..., 2]]
        return np.where(ok[..., None], vals, 0)

    bok = (samples[:, 0] >= 0) & (samples[:, 0] < B)
    centre = read(samples[:, 1:] + ctr, bok)                                    # (N, L)
    in_patch = ((nhood >= 0) & (nhood < ps)).all(axis=1)                        # (E,)
    other = read(samples[:, None, 1:] + nhood[None], bok[:, None] & in_patch[None])   # (N, E, L)
    return ((other == centre[:, None]) & (other != 0)).any(axis=-1).astype(np.float32)


# ----------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------
def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def _on_device(a):
    return _is_tensor(a) and a.is_cuda


def _np_of(a):
    return a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)


def _int_kind(dtype_name, what):
    if not any(k in dtype_name for k in ("int", "bool")):
        raise ValueError("%s must be of an integer or bool type, got %s" % (what, dtype_name))


def _device_nhood(nhood, device, ndim, wrap=None):
    """`nhood` as a contiguous int32 (E, 3) tensor on `device` (2-d: a zero z column in front; `wrap`: entries
    taken `% wrap`).  For a device tensor the converted copy is kept on it with the version it was made from."""
    import torch
    key = (ndim, wrap)
    if _is_tensor(nhood):
        cache = getattr(nhood, "_ppp_nhood", None)
        if cache is None or cache[0] != nhood._version:
            cache = (nhood._version, {})
            nhood._ppp_nhood = cache
        if key in cache[1]:
            return cache[1][key]
        t = nhood.to(device=device, dtype=torch.int64)
    else:
        cache = None
        t = torch.as_tensor(np.asarray(nhood, dtype=np.int64), device=device)
    if t.dim() != 2 or t.shape[1] != ndim:
        raise ValueError("nhood of shape %s: (E, %d)" % (tuple(t.shape), ndim))
    if wrap is not None:
        t = torch.remainder(t, wrap)
    if ndim == 2:
        t = torch.cat([torch.zeros_like(t[:, :1]), t], dim=1)
    t = t.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
    if cache is not None:
        cache[1][key] = t
    return t


def _host_nhood(nhood, ndim, wrap=None):
    n = np.asarray(_np_of(nhood), dtype=np.int64)
    if n.ndim != 2 or n.shape[1] != ndim:
        raise ValueError("nhood of shape %s: (E, %d)" % (n.shape, ndim))
    if wrap is not None:
        n = n % wrap
    if ndim == 2:
        n = np.concatenate([np.zeros_like(n[:, :1]), n], axis=1)
    return n


def _torch_out_dtype(out_dtype):
    import torch
    if out_dtype is None:
        return torch.float32
    if isinstance(out_dtype, torch.dtype):
        dt = out_dtype
    else:
        dt = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}.get(
            getattr(out_dtype, "__name__", None) or str(np.dtype(out_dtype)))
    if dt not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError("out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    return dt


def _give_back(res, seg, out_dtype):
    """a float32 NumPy result as what the caller of `seg` expects: a NumPy array, or a CPU tensor"""
    if not _is_tensor(seg):
        if out_dtype is None:
            return res
        dt = _torch_out_dtype(out_dtype)
        import torch
        if dt == torch.bfloat16:
            raise ValueError("NumPy has no bfloat16: pass a tensor, or out_dtype float32 / float16")
        return res.astype(np.float16 if dt == torch.float16 else np.float32)
    import torch
    return torch.from_numpy(res).to(_torch_out_dtype(out_dtype))


def _raise_if(flags, messages):
    """ONE device -> host read of the stacked 0-dim bool tensors `flags`"""
    import torch
    if flags:
        bad = torch.stack(flags).cpu().tolist()
        for b, m in zip(bad, messages):
            if b:
                raise ValueError(m)


def _label_checks(seg, single):
    """(flags, messages) of what `check` asks of the labels -- tensors, evaluated later in one read"""
    import torch
    flags, msgs = [], []
    if seg.numel() == 0:
        return flags, msgs
    if seg.dtype in (torch.int64,) or "uint32" in str(seg.dtype) or "uint64" in str(seg.dtype):
        flags.append((seg.amin() < -2 ** 31) | (seg.amax() > 2 ** 31 - 1))
        msgs.append("label ids do not fit int32")
    if single and seg.dtype != torch.bool:
        flags.append((seg.amin() < -MAX_SINGLE_ID) | (seg.amax() > MAX_SINGLE_ID))
        msgs.append("the one-channel form multiplies the ids as 32-bit integers: |id| <= %d" % MAX_SINGLE_ID)
    return flags, msgs


def _host_label_checks(seg, single):
    if seg.size == 0:
        return
    lo, hi = int(seg.min()), int(seg.max())
    if lo < -2 ** 31 or hi > 2 ** 31 - 1:
        raise ValueError("label ids do not fit int32")
    if single and (lo < -MAX_SINGLE_ID or hi > MAX_SINGLE_ID):
        raise ValueError("the one-channel form multiplies the ids as 32-bit integers: |id| <= %d" % MAX_SINGLE_ID)


def _dense(seg, nhood, ndim, single, check, box, out_dtype):
    want = ndim + (1 if single else 2)
    if len(seg.shape) != want:
        raise ValueError("labels of shape %s: %d axes expected" % (tuple(seg.shape), want))
    _int_kind(str(seg.dtype), "labels")
    if single and out_dtype is not None and _torch_out_dtype(out_dtype) != _torch_out_dtype(None):
        raise ValueError("the one-channel form (id squared) is float32 only")
    spatial = tuple(int(s) for s in seg.shape[-ndim:])
    if box is not None:
        box = tuple(int(v) for v in box)
        if len(box) != 2 * ndim:
            raise ValueError("box has %d entries: %d expected" % (len(box), 2 * ndim))
        if any(a < 0 or b > s or a >= b for a, b, s in zip(box[0::2], box[1::2], spatial)):
            raise ValueError("box %s is empty or leaves the volume %s" % (box, spatial))
        if ndim == 2:
            box = (0, 1) + box
    lead = tuple(int(s) for s in seg.shape[:-ndim])
    if _on_device(seg):
        import torch
        from . import backend
        if check:
            _raise_if(*_label_checks(seg, single))
        d_nhood = _device_nhood(nhood, seg.device, ndim)
        labels = seg.reshape(lead + (1,) * (3 - ndim) + spatial).to(torch.int32).contiguous()
        E = int(d_nhood.shape[0])
        if E == 0 or labels.numel() == 0:
            shape3 = (1,) * (3 - ndim) + spatial if box is None else tuple(b - a for a, b in zip(box[0::2], box[1::2]))
            res = torch.zeros((lead[0], E) + shape3, dtype=_torch_out_dtype(out_dtype), device=seg.device)
        else:
            res = backend.gt_affs_dense(labels, d_nhood, box=box, out_dtype=_torch_out_dtype(out_dtype), single=single)
        return res.reshape(res.shape[:2] + res.shape[5 - ndim:])
    host = _np_of(seg)
    if check:
        _host_label_checks(host, single)
    res = gt_affs_dense_host(host.reshape(lead + (1,) * (3 - ndim) + spatial), _host_nhood(nhood, ndim), box, single)
    return _give_back(res.reshape(res.shape[:2] + res.shape[5 - ndim:]), seg, out_dtype)


def _sides(v, ndim, what):
    v = [int(a) for a in np.asarray(_np_of(v)).reshape(-1)]
    if len(v) == 1:
        v = v * ndim
    if len(v) != ndim:
        raise ValueError("%s has %d entries: 1 or %d expected" % (what, len(v), ndim))
    return (1,) * (3 - ndim) + tuple(v), (0,) * (3 - ndim) + tuple(v)


def _samples(seg, nhood, ps, psH, samples_loc, b, ndim, check, out_dtype):
    if len(seg.shape) != ndim + 2:
        raise ValueError("labels of shape %s: %d axes expected" % (tuple(seg.shape), ndim + 2))
    _int_kind(str(seg.dtype), "labels")
    ps3, _ = _sides(ps, ndim, "ps")
    _, ctr3 = _sides(psH, ndim, "psH")
    if any(p < 1 for p in ps3) or any(c < 0 or c >= p for c, p in zip(ctr3, ps3)):
        raise ValueError("centre %s outside the patch %s" % (ctr3[3 - ndim:], ps3[3 - ndim:]))
    wrap_by = ps3[-1] if len(set(ps3[3 - ndim:])) == 1 else None
    if wrap_by is None:
        raise ValueError("the patch is cubic in the reference: ps = %s" % (ps3[3 - ndim:],))
    cols = ndim + (1 if b is None else 0)
    B, L = int(seg.shape[0]), int(seg.shape[1])
    spatial = tuple(int(s) for s in seg.shape[-ndim:])
    size3 = (1,) * (3 - ndim) + spatial
    if _on_device(seg):
        import torch
        from . import backend
        loc = samples_loc if _is_tensor(samples_loc) else torch.as_tensor(np.asarray(samples_loc, dtype=np.int64))
        loc = loc.to(seg.device)
        d_nhood = _device_nhood(nhood, seg.device, ndim, wrap=wrap_by)
        E = int(d_nhood.shape[0])
        if loc.numel() == 0:
            return torch.zeros((0, E), dtype=_torch_out_dtype(out_dtype), device=seg.device)
        if loc.dim() != 2 or loc.shape[1] != cols:
            raise ValueError("samples_loc of shape %s: (N, %d)" % (tuple(loc.shape), cols))
        _int_kind(str(loc.dtype), "samples_loc")
        loc = loc.to(torch.int64)
        parts = [torch.full_like(loc[:, :1], int(b))] if b is not None else [loc[:, :1]]
        if ndim == 2:
            parts.append(torch.zeros_like(loc[:, :1]))
        parts.append(loc[:, (0 if b is not None else 1):])
        rows = torch.cat(parts, dim=1)
        if check:
            flags, msgs = _label_checks(seg, False)
            top = torch.tensor([B - 1] + [s - p for s, p in zip(size3, ps3)], dtype=torch.int64, device=seg.device)
            flags.append(((rows < 0) | (rows > top)).any())
            msgs.append("a sample patch of side %d leaves the volume %s (or its batch index the batch of %d)" % (wrap_by, spatial, B))
            _raise_if(flags, msgs)
        labels = seg.reshape((B, L) + size3).to(torch.int32).contiguous()
        return backend.gt_affs_samples(labels, rows.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous(), d_nhood,
                                       ps3, ctr3, out_dtype=_torch_out_dtype(out_dtype))
    host = _np_of(seg)
    loc = np.asarray(_np_of(samples_loc))
    h_nhood = _host_nhood(nhood, ndim, wrap=wrap_by)
    if loc.size == 0:
        return _give_back(np.zeros((0, len(h_nhood)), dtype=np.float32), seg, out_dtype)
    if loc.ndim != 2 or loc.shape[1] != cols:
        raise ValueError("samples_loc of shape %s: (N, %d)" % (loc.shape, cols))
    _int_kind(str(loc.dtype), "samples_loc")
    loc = loc.astype(np.int64)
    parts = [np.full_like(loc[:, :1], int(b))] if b is not None else [loc[:, :1]]
    if ndim == 2:
        parts.append(np.zeros_like(loc[:, :1]))
    parts.append(loc[:, (0 if b is not None else 1):])
    rows = np.concatenate(parts, axis=1)
    if check:
        _host_label_checks(host, False)
        top = np.array([B - 1] + [s - p for s, p in zip(size3, ps3)])
        if ((rows < 0) | (rows > top)).any():
            raise ValueError("a sample patch of side %d leaves the volume %s (or its batch index the batch of %d)"
                             % (wrap_by, spatial, B))
    res = gt_affs_samples_host(host.reshape((B, L) + size3), rows, h_nhood, ps3, ctr3)
    return _give_back(res, seg, out_dtype)


# ----------------------------------------------------------------------------------------
# the reference's ten names
# ----------------------------------------------------------------------------------------
def seg_to_affgraph_3d_multi_torch_code_batch(seg, nhood, device, ps, psH, samples_loc, b, check=True, out_dtype=None):
    """train_util.py:349-391: seg (B, L, Z, Y, X), samples_loc (N, 3) corners in batch item `b`.  (N, E)."""
    return _samples(seg, nhood, ps, psH, samples_loc, int(b), 3, check, out_dtype)


def seg_to_affgraph_2d_multi_torch_code_batch(seg, nhood, device, ps, psH, samples_loc, b, check=True, out_dtype=None):
    """train_util.py:394-435: seg (B, L, Y, X), samples_loc (N, 2) corners in batch item `b`.  (N, E)."""
    return _samples(seg, nhood, ps, psH, samples_loc, int(b), 2, check, out_dtype)


def seg_to_affgraph_3d_multi_torch_code(seg, nhood, device, ps, psH, samples_loc, check=True, out_dtype=None):
    """train_util.py:438-478: seg (B, L, Z, Y, X), samples_loc (N, 4) rows (b, z, y, x).  (N, E)."""
    return _samples(seg, nhood, ps, psH, samples_loc, None, 3, check, out_dtype)


def seg_to_affgraph_2d_multi_torch_code(seg, nhood, device, ps, psH, samples_loc, check=True, out_dtype=None):
    """train_util.py:481-520: seg (B, L, Y, X), samples_loc (N, 3) rows (b, y, x).  (N, E)."""
    return _samples(seg, nhood, ps, psH, samples_loc, None, 2, check, out_dtype)


def seg_to_affgraph_3d_multi_torch(seg, nhood, device=None, check=True, box=None, out_dtype=None):
    """train_util.py:523-567: seg (B, L, Z, Y, X), nhood (E, 3).  (B, E, Z, Y, X), or the `box` of it."""
    return _dense(seg, nhood, 3, False, check, box, out_dtype)


def seg_to_affgraph_2d_multi_torch(seg, nhood, device=None, check=True, box=None, out_dtype=None):
    """train_util.py:570-610: seg (B, L, Y, X), nhood (E, 2).  (B, E, Y, X), or the `box` of it."""
    return _dense(seg, nhood, 2, False, check, box, out_dtype)


def seg_to_affgraph_2d_torch(seg, nhood, device=None, check=True, box=None):
    """train_util.py:613-651: seg (B, Y, X); the value is the id squared.  (B, E, Y, X) float32."""
    return _dense(seg, nhood, 2, True, check, box, None)


def seg_to_affgraph_3d_torch(seg, nhood, device=None, check=True, box=None):
    """train_util.py:654-695: seg (B, Z, Y, X); the value is the id squared.  (B, E, Z, Y, X) float32."""
    return _dense(seg, nhood, 3, True, check, box, None)


def seg_to_affgraph_3d_torch_code(seg, nhood, device, ps, psH, samples_loc, **kwargs):
    """train_util.py:698-735 cannot run: its factors t2 / t3 index the whole batch `seg[:, psH, psH, psH]`
    where they mean the patches, a shape error unless B == N.  No meaning is invented here."""
    raise NotImplementedError("the reference's seg_to_affgraph_3d_torch_code cannot run (train_util.py:730-731 index "
                              "the batch instead of the patches); use the multi-channel form")


def seg_to_affgraph_2d_torch_code(seg, nhood, device, ps, psH, samples_loc, **kwargs):
    """train_util.py:738-774 cannot run: it reads `fg_seg`, a name it never defines.  No meaning is invented."""
    raise NotImplementedError("the reference's seg_to_affgraph_2d_torch_code cannot run (train_util.py:769-770 read the "
                              "undefined name fg_seg); use the multi-channel form")
