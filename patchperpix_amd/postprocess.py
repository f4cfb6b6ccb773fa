"""Post-steps of the blockwise `label` driver (reference: PatchPerPix/util/postprocess.py:24-52 and
PatchPerPix/vote_instances/stitch_patch_graph.py:831-894): drop small instances, renumber,
dilate.

`remove_small_components`, `relabel` and `dilate_instances` are host NumPy like the reference.  Their
`*_device` forms return the same arrays from the HIP kernels of csrc/ppp_postprocess.hip; `post_steps`
is the block the drivers run after the assembly and picks between the two (`use_device`).

`postprocess_instances` is the reference driver's `postprocess` task (postprocess.py:77-119): the instance
map cleaned again and one 3-d skeleton per instance -- `skeletonize_instances` (host loop, the definition)
or `skeletonize_instances_device` (all instances in one pass, csrc/ppp_skeleton.hip).

`postprocess_fg` is the task's other branch, `process_fg_prediction` (postprocess.py:122-199): the thresholded
foreground without its small components that lie far from the large ones -- `fg_filter` (scipy, the
definition) or `fg_filter_device` (csrc/ppp_edt.hip and the fg_filter kernels of csrc/ppp_postprocess.hip),
both comparing the exact integer squared distance with `min_sq_distance`."""
import logging
import math
import os

import numpy as np
from scipy import ndimage

logger = logging.getLogger(__name__)


def remove_small_components(array, compsize=5):
    """Instances of at most `compsize` voxels become background (postprocess.py:24-37)."""
    labels, inverse, counts = np.unique(array, return_inverse=True, return_counts=True)
    keep = np.where(counts <= compsize, 0, labels).astype(array.dtype)
    return keep[inverse].reshape(array.shape)


def relabel(array, start=None):
    """Consecutive ids in ascending order of the old ones, from `start` (default 1); 0 stays 0
    (postprocess.py:40-52)."""
    labels, inverse = np.unique(array, return_inverse=True)
    first = 1 if start is None else int(start)
    new = np.zeros(len(labels), dtype=array.dtype)
    nz = labels != 0
    new[nz] = first + np.arange(int(np.count_nonzero(nz)))
    return new[inverse].reshape(array.shape)


def color(src, colormap=None):
    """postprocess.py:55-74: an array of shape ``src.shape + (3,)`` and of ``src``'s dtype, zero where
    ``src`` is 0; every other label takes ``np.random.randint(0, 255, 3)``.  The draws are the reference's,
    call for call: ONE call per non-zero label, in ascending label order, from NumPy's global generator --
    unseeded, so the colour of a label is no function of the input, but a caller who seeds ``np.random``
    gets the reference's picture pixel for pixel.  ``colormap='glasbey'`` needs the ``colorcet`` package,
    which is not a dependency here."""
    src = np.asarray(src)
    if colormap == "glasbey":
        raise NotImplementedError("colormap='glasbey' needs the colorcet package, which this repository does not use")
    labels, inverse = np.unique(src, return_inverse=True)
    table = np.zeros((len(labels), 3), dtype=src.dtype)
    for k, label in enumerate(labels):
        if label == 0:
            continue
        table[k] = np.random.randint(0, 255, 3)
    return table[inverse.reshape(src.shape)]


def dilate_instances(instances, iterations=1):
    """stitch_patch_graph.py:871-880: every instance, in ascending id order, is dilated by one
    step of the cross-shaped structuring element and painted over what is there (later ids win,
    and an earlier dilation is seen by the later masks -- the loop works in place)."""
    out = np.copy(instances)
    for lbl in np.unique(instances):
        if lbl == 0:
            continue
        out[ndimage.binary_dilation(out == lbl, iterations=iterations)] = lbl
    return out


# ----------------------------------------------------------------------------------------
# the same steps on the device
# ----------------------------------------------------------------------------------------
MAX_TABLE_ID = 1 << 28      # the count table has one slot per id: 1 GiB at 2^28 ids


def use_device():
    """The one dispatch rule of the post-steps: the device when there is one and PPP_POSTPROCESS is
    not "host", else the host functions above (today's behaviour, not a fallback for a missing
    kernel: with a device the library must load)."""
    if os.environ.get("PPP_POSTPROCESS", "") == "host":
        return False
    import torch
    return torch.cuda.is_available()


def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "is_cuda")


def _on_host(fn, array, *args):
    """the host function on a NumPy array or a tensor, returning the same kind"""
    if not _is_tensor(array):
        return fn(array, *args)
    import torch
    return torch.from_numpy(np.ascontiguousarray(fn(array.cpu().numpy(), *args))).to(array.device)


def _ids_to_device(array):
    """A map of uint16 / uint32 / int32 ids as a contiguous device tensor with int32 STORAGE (its bits
    are the uint32 ids), with (lo, hi) = the extremes of that storage; None for any other dtype or
    an empty map."""
    import torch
    if _is_tensor(array):
        name = str(array.dtype).replace("torch.", "")
        if name not in ("uint16", "uint32", "int32") or array.numel() == 0:
            return None
        t = array if array.is_cuda else array.cuda()
        t = t.to(torch.int32) if name == "uint16" else t.contiguous().view(torch.int32)
        if t.data_ptr() == array.data_ptr():
            t = t.clone()
    else:
        array = np.asarray(array)
        if array.dtype not in (np.uint16, np.uint32, np.int32) or array.size == 0:
            return None
        t = torch.from_numpy(np.ascontiguousarray(array).astype(np.uint32, copy=False).view(np.int32)).cuda()
    lo, hi = torch.aminmax(t)
    return t.contiguous(), int(lo), int(hi)


def _ids_from_device(t, like):
    """back to the kind and dtype of `like`, wrapping the way the host's astype does"""
    import torch
    if _is_tensor(like):
        name = str(like.dtype).replace("torch.", "")
        if name == "uint16":
            t = (t & 0xFFFF).to(torch.uint16)
        elif name == "uint32":
            t = t.view(torch.uint32)
        return t.reshape(like.shape).to(like.device)
    return t.cpu().numpy().view(np.uint32).astype(np.asarray(like).dtype).reshape(np.shape(like))


def _compact_host(array, compsize, do_relabel, start):
    if compsize is not None:
        array = remove_small_components(array, compsize)
    return relabel(array, start) if do_relabel else array


def _compact_device(array, compsize, do_relabel, start):
    """remove_small_components (compsize not None) and / or relabel in ONE pass over the map"""
    from . import backend
    dev = _ids_to_device(array)
    if dev is None or dev[1] < 0 or dev[2] >= MAX_TABLE_ID:
        # (a negative extreme of the int32 storage: a negative id, or a uint32 id >= 2^31)
        logger.debug("post-steps: compaction on the host (dtype %s, or ids beyond the %d-slot table)",
                     getattr(array, "dtype", None), MAX_TABLE_ID)
        return _on_host(_compact_host, array, compsize, do_relabel, start)
    t, _, hi = dev
    size = -1 if compsize is None else int(math.floor(compsize))
    backend.post_compact_ids(t.reshape(-1), hi, compsize=max(size, -1), relabel=do_relabel,
                             start=1 if start is None else int(start))
    return _ids_from_device(t, array)


def remove_small_components_device(array, compsize=5):
    """`remove_small_components` from the device (ppp_post_compact_ids); NumPy array or device tensor
    in, the same kind and dtype out."""
    return _compact_device(array, compsize, False, None)


def relabel_device(array, start=None):
    """`relabel` from the device (ppp_post_compact_ids)."""
    return _compact_device(array, None, True, start)


def dilate_instances_device(instances, iterations=1):
    """`dilate_instances` from the device (ppp_post_dilate: the ascending loop in closed form, no
    loop over instances)."""
    from . import backend
    ndim = len(instances.shape)
    dev = _ids_to_device(instances) if (iterations == 1 and 1 <= ndim <= 3) else None
    signed = str(getattr(instances, "dtype", "")).replace("torch.", "") == "int32"
    if dev is None or (signed and dev[1] < 0):
        logger.debug("post-steps: dilation on the host (dtype %s, iterations %s)", getattr(instances, "dtype", None), iterations)
        return _on_host(dilate_instances, instances, iterations)
    t = dev[0].reshape((1,) * (3 - ndim) + tuple(int(v) for v in instances.shape))
    out, rounds = backend.post_dilate(t)
    backend.note("post_dilate_rounds", rounds)
    return _ids_from_device(out, instances)


def clean_mask_device(mask, structure, size):
    """`vote_instances.stitch_patch_graph.clean_mask` from the device (ppp_post_clean_mask): returns
    (bool array, components found, components kept), or None when the case is the host's (not 2-d / 3-d,
    a structure that is not 3 per axis, centred and centrosymmetric, an empty mask)."""
    from . import backend
    import torch
    m = np.asarray(mask)
    st = np.asarray(structure) != 0
    if m.ndim not in (2, 3) or m.size == 0 or m.size >= 1 << 31 or st.shape != (3,) * m.ndim:
        return None
    if m.ndim == 2:
        st = np.stack([np.zeros_like(st), st, np.zeros_like(st)])
    flat = st.reshape(-1)
    if not flat[13] or not np.array_equal(flat, flat[::-1]):
        return None
    bits = int(sum(1 << i for i in np.flatnonzero(flat)))
    m3 = np.ascontiguousarray(m != 0).astype(np.uint8).reshape((1,) * (3 - m.ndim) + m.shape)
    out, found, kept = backend.post_clean_mask(torch.from_numpy(m3).cuda(), bits, int(math.floor(size)))
    return out.cpu().numpy().astype(bool).reshape(m.shape), found, kept


def compact(instances, compsize):
    """relabel(remove_small_components(instances, compsize)), by the dispatch rule"""
    if use_device():
        return _compact_device(instances, compsize, True, None)
    return relabel(remove_small_components(instances, compsize))


# ----------------------------------------------------------------------------------------
# the `postprocess` task: one 3-d skeleton per instance (postprocess.py:77-119)
# ----------------------------------------------------------------------------------------
def skeletonize_instances(instances, crop=True):
    """The 3-d skeleton of every instance of a (Z, Y, X) or (Y, X) id map, as a map of the same dtype
    and shape: a voxel keeps its id L where ``backend.host_skeletonize_3d(instances == L)`` keeps it, every
    other voxel is 0 -- the loop of postprocess.py:110-112 with the library's own thinning (Lee / Kashyap /
    Chu 1994; parity with scikit-image's skeletonize_3d is UNPINNED, as for skeletonize_backend="ppp").
    This is the host DEFINITION of `skeletonize_instances_device`.

    crop: thin each instance inside its bounding box instead of the whole volume -- the same result (the
    thinning reads a voxel's 26 neighbours only, everything outside the box is empty either way and the
    raster order inside it is the volume's); the box keeps two slices where the volume has more than
    one, because the thinning peels the z borders of a volume of several slices only."""
    from . import backend
    inst = np.asarray(instances)
    shape = inst.shape
    if inst.ndim not in (2, 3):
        raise ValueError("skeletonize_instances needs a (Z, Y, X) or (Y, X) map")
    inst3 = inst.reshape((1,) * (3 - inst.ndim) + shape)
    out = np.zeros_like(inst3)
    labels, inverse = np.unique(inst3, return_inverse=True)
    if not crop:
        for lbl in labels[labels != 0]:
            out[backend.host_skeletonize_3d(inst3 == lbl)] = lbl
        return out.reshape(shape)
    dense = inverse.reshape(inst3.shape).astype(np.int32)       # position in `labels`: find_objects wants small ids
    Z = inst3.shape[0]
    for k, box in enumerate(ndimage.find_objects(dense + 1)):
        lbl = labels[k]
        if lbl == 0 or box is None:
            continue
        if Z > 1 and box[0].stop - box[0].start == 1:
            z0 = min(box[0].start, Z - 2)
            box = (slice(z0, z0 + 2),) + tuple(box[1:])
        out[box][backend.host_skeletonize_3d(inst3[box] == lbl)] = lbl
    return out.reshape(shape)


def skeletonize_instances_device(instances):
    """`skeletonize_instances` from the device in ONE pass over the map, whatever the number of instances
    (backend.skeletonize_labels = ppp_skeletonize_labels, csrc/ppp_skeleton.hip): the same map, voxel for
    voxel.  uint16 / uint32 / int32 maps (NumPy or device tensor) go as they are; a NumPy map of another
    integer dtype goes as uint32 when its ids fit, and comes back in its own dtype."""
    from . import backend
    if _is_tensor(instances) or np.asarray(instances).dtype in (np.uint16, np.uint32, np.int32):
        return backend.skeletonize_labels(instances)
    inst = np.asarray(instances)
    if inst.dtype.kind not in "iu" or (inst.size and (int(inst.min()) < 0 or int(inst.max()) >= 1 << 32)):
        raise ValueError("skeletonize_instances_device: ids must be integers that fit 32 bits (dtype %s)" % inst.dtype)
    return backend.skeletonize_labels(inst.astype(np.uint32)).astype(inst.dtype)


def instance_skeletons(instances):
    """skeletonize_instances, by the dispatch rule; returns (map, the implementation's name)"""
    if use_device():
        return skeletonize_instances_device(instances), "ppp_skeletonize_labels"
    return skeletonize_instances(instances), "ppp_host_skeletonize_3d"


def postprocess_instances(samples, output_folder, **kwargs):
    """The `process_instances` branch of the reference's `postprocess` task (postprocess.py:77-119,
    called from run_ppp.py:2246-2259).  For every result file ``sample`` (.hdf, opened "a"):

    - ``res_key`` is read, ids with ``counts <= remove_small_comps`` are dropped and the rest renumbered
      (`compact`: device or host), and the map is written as dataset ``<res_key>_rm_<remove_small_comps>``
      (gzip), uint16 when its maximum is < 65535, else uint32 -- the reference's rule.  An existing
      dataset of that name is replaced (the reference's create_dataset fails on a second run).
    - ``export_skeleton_nrrds``: the skeleton of every instance of the cleaned map, from ONE
      `instance_skeletons` call instead of one thinning per instance, each written as
      ``<output_folder>/<sample>_<label>.nrrd`` (mininrrd: the payload and sizes of the reference's
      ``nrrd.write(mask.transpose(2, 1, 0))``).
    - ``export_skeleton_labels`` (this project's own option, not the reference's): the skeleton label
      map as ONE dataset ``<res_key>_rm_<n>_skeleton`` instead of one file per instance.

    The thinning is the library's own (Lee / Kashyap / Chu 1994): parity with scikit-image's
    skeletonize_3d, which the reference calls, is UNPINNED; the datasets carry the attribute
    ``skeletonize_instances`` naming the implementation that made the skeletons."""
    from . import minihdf5, mininrrd
    comp_thresh = kwargs["remove_small_comps"]
    res_key = kwargs["res_key"]
    want_nrrds = bool(kwargs.get("export_skeleton_nrrds", False))
    want_labels = bool(kwargs.get("export_skeleton_labels", False))
    for sample in samples:
        with minihdf5.File(sample, "a") as inf:
            cleaned = np.asarray(compact(np.asarray(inf[res_key]), comp_thresh))
            dtype = np.uint16 if int(cleaned.max(initial=0)) < 65535 else np.uint32
            cleaned = cleaned.astype(dtype)
            new_key = res_key + ("_rm_%s" % comp_thresh)
            ds = inf.create_dataset(new_key, data=cleaned, dtype=dtype, compression="gzip")
            if not (want_nrrds or want_labels):
                continue
            skel, served_by = instance_skeletons(cleaned)
            logger.warning("postprocess: instance skeletons by %s; not pinned to scikit-image's skeletonize_3d",
                           served_by)
            ds.attrs["skeletonize_instances"] = served_by
            if want_labels:
                sk = inf.create_dataset(new_key + "_skeleton", data=skel, dtype=dtype, compression="gzip")
                sk.attrs["skeletonize_instances"] = served_by
            if want_nrrds:
                os.makedirs(output_folder, exist_ok=True)
                sample_name = os.path.basename(sample).split(".")[0]
                vol = skel.reshape((1,) * (3 - skel.ndim) + skel.shape)
                for lbl in np.unique(cleaned):
                    if lbl > 0:
                        mininrrd.write(os.path.join(output_folder, sample_name + ("_%i.nrrd" % lbl)), vol == lbl)


# ----------------------------------------------------------------------------------------
# the `postprocess_fg` task: small foreground components far from the large ones removed
# (postprocess.py:122-199)
# ----------------------------------------------------------------------------------------
def min_sq_distance(max_distance):
    """The reference removes a small component when ``dist >= max_distance_to_fg`` holds on all its voxels,
    with ``dist = sqrt(float64(d2))`` of the exact integer squared distance d2 (scipy's
    distance_transform_edt).  sqrt is monotone, so that is ``min d2 >= T`` with T the smallest integer
    t >= 0 such that ``np.sqrt(np.float64(t)) >= np.float64(max_distance)``; this returns T, found by
    searching around ceil(max_distance ** 2).  0 for a value that is not positive (the reference's else
    branch: every small component goes).  From 2 ** 31 on, beyond the diagonal of any volume a call
    accepts, the answer is 2 ** 62: above every squared distance."""
    m = np.float64(max_distance)
    if not m > 0:
        return 0
    if m >= 2.0 ** 31:
        return 1 << 62
    t = int(math.ceil(float(m) * float(m)))
    while t > 0 and np.sqrt(np.float64(t - 1)) >= m:
        t -= 1
    while np.sqrt(np.float64(t)) < m:
        t += 1
    return t


def fg_filter(mask, compsize, max_distance, want_instances=False):
    """postprocess.py:134-174 and :185 on a (Z, Y, X) mask, the host DEFINITION of `fg_filter_device`.
    Components are those of ``ndimage.label(mask, np.ones((3, 3, 3)))``; SMALL: ``count <= compsize``, BIG:
    the others.  With ``T = min_sq_distance(max_distance)``:

    - fg = the voxels of big components and of the small ones whose minimum squared distance to a voxel
      of a big component is < T (T = 0, the reference's else branch: no small one stays);
    - instances = the surviving components numbered in ascending order of their smallest raster
      index, which is ``ndimage.label`` of fg.

    Two inputs on which the reference has no defined result are defined here:

    - no big component while max_distance > 0 (scipy's transform of an all-ones array returns an
      artefact): the minimum over an empty set is infinite, every small component is removed;
    - nothing to remove (the reference raises IndexError: it indexes with an empty float array):
      nothing is removed.

    Returns (uint8 fg, uint32 instances or None, (found, small, removed, kept))."""
    m = np.asarray(mask) != 0
    if m.ndim != 3:
        raise ValueError("fg_filter needs a (Z, Y, X) mask, not %d axes" % m.ndim)
    T = min_sq_distance(max_distance)
    labels, found = ndimage.label(m, np.ones((3, 3, 3)))
    counts = np.bincount(labels.ravel(), minlength=found + 1)
    big = counts > compsize
    big[0] = False
    small = counts <= compsize
    small[0] = False
    remove = small.copy()
    if T > 0 and big.any() and small.any():
        dist = ndimage.distance_transform_edt(np.logical_not(big[labels]))
        d2 = np.rint(dist * dist).astype(np.int64)
        mind2 = np.full(found + 1, np.iinfo(np.int64).max, dtype=np.int64)
        sel = small[labels]
        np.minimum.at(mind2, labels[sel], d2[sel])
        remove &= mind2 >= T
    keep = (big | small) & ~remove
    fg = keep[labels].astype(np.uint8)
    inst = None
    if want_instances:
        inst = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)[labels]
    n_small, n_removed = int(small.sum()), int(remove.sum())
    return fg, inst, (int(found), n_small, n_removed, int(found) - n_removed)


def fg_filter_device(mask, compsize, max_distance, want_instances=False):
    """`fg_filter` from the device (backend.post_fg_filter = ppp_post_fg_filter: union-find components, the
    exact squared distance transform of csrc/ppp_edt.hip, integers only): the same three results.  Masks
    that are empty or hold 2^31 voxels or more are the host's."""
    from . import backend
    import torch
    m = np.asarray(mask)
    if m.ndim != 3 or m.size == 0 or m.size >= 1 << 31 or sum(int(n) ** 2 for n in m.shape) >= (1 << 32) - 1:
        logger.debug("postprocess_fg: component filter on the host (shape %s)", m.shape)
        return fg_filter(m, compsize, max_distance, want_instances)
    T = min(min_sq_distance(max_distance), 0xFFFFFFFF)      # (no squared distance of the volume reaches it)
    size = min(max(int(math.floor(compsize)), -1), m.size)
    t = torch.from_numpy(np.ascontiguousarray(m != 0).astype(np.uint8)).cuda()
    fg, inst, stats = backend.post_fg_filter(t, size, T, want_instances)
    return (fg.cpu().numpy(), None if inst is None else inst.cpu().numpy().view(np.uint32), stats)


def postprocess_fg(samples, output_folder, **kwargs):
    """The `process_fg_prediction` branch of the reference's `postprocess` task (postprocess.py:122-199,
    called from run_ppp.py:2234-2245), under its name and kwargs: fg_key, fg_threshold, remove_small_comps,
    max_distance_to_fg, cc_instances, export_skeleton_nrrds.  For every prediction file ``sample`` (zarr
    through minizarr, ``.hdf`` through minihdf5):

    - ``mask = np.asarray(sample[fg_key]) > fg_threshold`` on the host, the reference's own expression; a
      dataset that is not 3-d raises ValueError (scipy's label refuses it with the 3 x 3 x 3 structure);
    - `fg_filter` / `fg_filter_device` by the dispatch rule (`use_device`), see there for the result and for
      the two inputs the reference leaves undefined;
    - the output file is ``<output_folder>/<basename with .zarr -> .hdf>``, opened "w" (ValueError when
      that is the sample itself): ``volumes/fg`` (uint8, gzip) and, with ``cc_instances``,
      ``volumes/instances`` (``astype(np.uint16)``, gzip: ids above 65535 wrap as in the reference);
    - ``export_skeleton_nrrds``: the 3-d thinning of the foreground (backend.skeletonize_3d on the device,
      else backend.host_skeletonize_3d), written to the output name with ``.nrrd`` (mininrrd: the payload
      of the reference's ``nrrd.write(mask.transpose(2, 1, 0))``).  The thinning is the library's own (Lee /
      Kashyap / Chu 1994): parity with scikit-image's skeletonize_3d stays UNPINNED.

    ``volumes/fg`` carries the attribute ``fg_filter`` naming the implementation used and, with a
    skeleton, ``skeletonize_foreground`` naming the thinning."""
    from . import backend, minihdf5, mininrrd, minizarr
    comp_thresh = kwargs["remove_small_comps"]
    max_distance = kwargs.get("max_distance_to_fg", 0)
    want_inst = bool(kwargs.get("cc_instances", False))
    os.makedirs(output_folder, exist_ok=True)
    for sample in samples:
        outfn = os.path.join(output_folder, os.path.basename(os.path.normpath(sample)).replace(".zarr", ".hdf"))
        if os.path.abspath(outfn) == os.path.abspath(sample):
            raise ValueError("postprocess_fg: the output file %s is the sample itself" % outfn)
        if str(sample).rstrip("/").endswith(".hdf"):
            with minihdf5.File(sample, "r") as inf:
                pred = np.asarray(inf[kwargs["fg_key"]])
        else:
            pred = np.asarray(minizarr.open(sample, "r")[kwargs["fg_key"]])
        if pred.ndim != 3:
            raise ValueError("postprocess_fg: %s[%s] has %d axes, the 3 x 3 x 3 structure needs 3"
                             % (sample, kwargs["fg_key"], pred.ndim))
        mask = pred > kwargs["fg_threshold"]
        device = use_device()
        fg, inst, stats = (fg_filter_device if device else fg_filter)(mask, comp_thresh, max_distance, want_inst)
        logger.info("postprocess_fg %s: %d components, %d small, %d removed, %d kept", os.path.basename(outfn), *stats)
        with minihdf5.File(outfn, "w") as hout:
            ds = hout.create_dataset("volumes/fg", data=fg.astype(np.uint8), dtype=np.uint8, compression="gzip")
            ds.attrs["fg_filter"] = "ppp_post_fg_filter" if device else "scipy"
            if want_inst:
                hout.create_dataset("volumes/instances", data=inst.astype(np.uint16), dtype=np.uint16,
                                    compression="gzip")
            if kwargs.get("export_skeleton_nrrds", False):
                skel = backend.skeletonize_3d(fg) if device else backend.host_skeletonize_3d(fg)
                served_by = "ppp_skeletonize_3d" if device else "ppp_host_skeletonize_3d"
                logger.warning("postprocess_fg: foreground skeleton by %s; not pinned to scikit-image's "
                               "skeletonize_3d", served_by)
                ds.attrs["skeletonize_foreground"] = served_by
                stem = outfn[:-len(".hdf")] if outfn.endswith(".hdf") else outfn
                mininrrd.write(stem + ".nrrd", np.asarray(skel))


def max_projection(instances):
    """``np.max(instances, axis=0)`` as a NumPy array: `torch.amax` on the device by the dispatch rule (ids
    that fit the device's int32 storage), else NumPy on the host.  One small reduction, not a hot path."""
    dev = _ids_to_device(instances) if use_device() and len(np.shape(instances)) >= 2 else None
    if dev is None or dev[1] < 0:
        inst = instances.cpu().numpy() if _is_tensor(instances) else np.asarray(instances)
        return np.max(inst, axis=0)
    import torch
    mip = torch.amax(dev[0], dim=0).cpu().numpy().view(np.uint32)
    dtype = np.dtype(str(instances.dtype).replace("torch.", ""))
    return mip.astype(dtype)


def save_mip_png(path, instances):
    """stitch_patch_graph.py:823-829 / :842-847: ``color(np.max(instances, axis=0)).astype(np.uint8)`` as a
    PNG (minipng).  The projection by `max_projection`, the colouring on the host on the 2-d image."""
    from . import minipng
    mip = max_projection(instances)
    if mip.ndim != 2:
        raise ValueError("save_mip needs a (Z, Y, X) instance map, not shape %s" % (np.shape(instances),))
    minipng.write(path, color(mip).astype(np.uint8))


def post_steps(instances, foreground, res_key, mip_stem=None, **kw):
    """What the label drivers do with the assembled uint32 map (stitch_patch_graph.py:823-894): small
    components removed and the ids compacted when remove_small_comps asks for it, then the datasets of
    the result file, all uint16 like the reference's astype (ids above 65 535 that survive wrap,
    :852-870): <res_key>, vote_foreground, <res_key>_masked and -- dilate_instances --
    <res_key>_dil_1, <res_key>_masked_dil_1.  Returns (instances, datasets).

    ``save_mip`` (:823-829, :842-847; the drivers pass ``mip_stem`` = <result_folder>/<sample>): the
    coloured maximum projection along z of the stitched map goes to ``<mip_stem>.png`` BEFORE the small
    components are removed, and that of the cleaned map to ``<mip_stem>_cleaned.png`` when
    remove_small_comps > 0.  Falsy or absent: no file is written."""
    foreground = np.asarray(foreground)
    save_mip = bool(kw.get("save_mip", False))
    if save_mip and mip_stem is None:
        raise ValueError("save_mip needs the driver's mip_stem (<result_folder>/<sample>)")
    if save_mip:
        save_mip_png(mip_stem + ".png", instances)
    if kw.get("remove_small_comps", 0) > 0:
        instances = compact(instances, kw["remove_small_comps"])
        if save_mip:
            save_mip_png(mip_stem + "_cleaned.png", instances)
    if int(instances.max(initial=0)) > np.iinfo(np.uint16).max:
        logger.warning("instance ids up to %d are written as uint16 like the reference does "
                       "(stitch_patch_graph.py:852-856): set remove_small_comps > 0 to compact "
                       "them first", int(instances.max()))
    masked = instances.copy()
    masked[foreground == 0] = 0
    datasets = {res_key: instances.astype(np.uint16), "vote_foreground": foreground.astype(np.uint16),
                res_key + "_masked": masked.astype(np.uint16)}
    if kw.get("dilate_instances", False):
        dil = dilate_instances_device(instances) if use_device() else dilate_instances(instances)
        datasets[res_key + "_dil_1"] = dil.astype(np.uint16)
        datasets[res_key + "_masked_dil_1"] = np.where(foreground == 0, 0, dil).astype(np.uint16)
    return instances, datasets
