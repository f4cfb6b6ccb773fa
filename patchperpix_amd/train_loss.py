"""The patch loss of training computed FROM THE LABELS: the reference's `add_affinities = "loss"` path makes the
ground-truth patch affinities (train_util.py:349-610) only to hand them to `MaskedBCEWithLogitsLoss`
(experiments/flylight/setups/setup01/torch_loss.py:47-67, called at :127-129).  Here a device tensor goes to the
fused kernels of csrc/ppp_patch_loss.hip: the target is consumed where it is made and never stored, the forward
reads the logits once, the backward reads them once and writes the gradient -- the only allocation of that size.

Definitions.  G is `train_util`'s multi-channel predicate, dense on `box` or sampled;
    l(x, g) = max(x, 0) - x g + log1p(exp(-|x|))
  dense    logits (B, E, bZ, bY, bX) -- the box's extents -- and optional weights w (B, bZ, bY, bX) >= 0:
           with w:     cnt = num_channels * sum w,  loss = sum w l / cnt,  dloss/dx = w (sigmoid(x) - g) / cnt,
                       loss and gradient 0 when cnt == 0 (the reference's `mean(loss) * 0.0`)
           without:    the mean over all B E bV elements.
           A voxel with w == 0 contributes 0 and gets gradient 0 whatever its logits hold.  The reference gives NaN
           there for a non-finite logit (0 * inf); this module does not, on either path.
  sampled  logits (N, E), G as `gt_affs_samples_host`: the mean over N E elements; N = 0 gives 0.
  counts   (x > 0, G, x > 0 and G) over ALL elements, unweighted, int64: what jaccard and accuracy of the patch
           summaries need (torch_loss.py:133-141).  No meaning is borrowed from torchmetrics.
The one-channel "id squared" target is not served (a BCE against c * c has no meaning): pass `seg[:, None]`.

`patch_loss_host` / `patch_loss_samples_host` are the NumPy float64 definitions; `patch_bce_from_labels` /
`patch_bce_from_label_samples` the differentiable functions (device tensors: the kernels; CPU tensors: plain torch
over the NumPy target); `PatchLossFromLabels` the module over both."""
import numpy as np
import torch

from . import train_util as tu


# ----------------------------------------------------------------------------------------
# the NumPy float64 definitions
# ----------------------------------------------------------------------------------------
def _bce64(x, g):
    """l(x, g) and sigmoid(x) - g in float64; the latter as g ? -sigmoid(-x) : sigmoid(x), without cancellation"""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g) != 0
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.exp(-np.abs(x))
        loss = np.where(g, np.maximum(-x, 0.0), np.maximum(x, 0.0)) + np.log1p(t)
        r = 1.0 / (1.0 + t)
        big, small = r, t * r                                    # sigmoid(|x|), sigmoid(-|x|)
        slope = np.where(g, -np.where(x >= 0, small, big), np.where(x >= 0, big, small))
    return loss, slope


def patch_loss_host(logits, seg, nhood, weight=None, box=None, num_channels=None):
    """The dense definition in float64: `logits` (B, E, bZ, bY, bX), `seg` int (B, L, Z, Y, X), `nhood` (E, 3),
    `weight` (B, bZ, bY, bX) or None, `box` = (z0, z1, y0, y1, x0, x1) or None, `num_channels` (default E).
    Returns (loss, grad): a float and the float64 array dloss/dlogits."""
    G = tu.gt_affs_dense_host(seg, nhood, box)
    x = np.asarray(logits, dtype=np.float64)
    if x.shape != G.shape:
        raise ValueError("logits of shape %s: %s expected" % (x.shape, G.shape))
    loss, slope = _bce64(x, G)
    if weight is None:
        if x.size == 0:
            return 0.0, np.zeros_like(x)
        return float(loss.sum() / x.size), slope / x.size
    w = np.asarray(weight, dtype=np.float64)
    if w.shape != (x.shape[0],) + x.shape[2:]:
        raise ValueError("weight of shape %s: %s expected" % (w.shape, (x.shape[0],) + x.shape[2:]))
    w = np.broadcast_to(w[:, None], x.shape)
    cnt = float(x.shape[1] if num_channels is None else num_channels) * float(np.asarray(weight, dtype=np.float64).sum())
    if cnt == 0:
        return 0.0, np.zeros_like(x)
    live = w != 0
    return float(np.where(live, w * loss, 0.0).sum() / cnt), np.where(live, w * slope, 0.0) / cnt


def patch_loss_samples_host(logits, seg, samples, nhood, ps, ctr):
    """The sampled definition in float64: `logits` (N, E); the other arguments as `gt_affs_samples_host`.
    Returns (loss, grad)."""
    G = tu.gt_affs_samples_host(seg, samples, nhood, ps, ctr)
    x = np.asarray(logits, dtype=np.float64).reshape(G.shape)
    if x.size == 0:
        return 0.0, np.zeros_like(x)
    loss, slope = _bce64(x, G)
    return float(loss.sum() / x.size), slope / x.size


def patch_counts_host(logits, G):
    """(x > 0, G, x > 0 and G) over all elements"""
    pos, g = np.asarray(logits) > 0, np.asarray(G) != 0
    return np.array([pos.sum(), g.sum(), (pos & g).sum()], dtype=np.int64)


# ----------------------------------------------------------------------------------------
# autograd over the kernels
# ----------------------------------------------------------------------------------------
class _DenseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, nhood, weight, box, num_channels, want_counts):
        from . import backend
        logits = logits.contiguous()
        loss, state, counts = backend.patch_loss_dense_fwd(logits, labels, nhood, weight=weight, box=box,
                                                           num_channels=num_channels, want_counts=want_counts)
        ctx.save_for_backward(logits, labels, nhood, weight, state)
        ctx.box = box
        if counts is not None:
            ctx.mark_non_differentiable(counts)
        return loss.reshape(()), counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_counts=None):
        from . import backend
        logits, labels, nhood, weight, state = ctx.saved_tensors
        grad_out = grad_loss.to(torch.float32).reshape(1).contiguous()
        grad = backend.patch_loss_dense_bwd(logits, labels, nhood, state, grad_out, weight=weight, box=ctx.box)
        return grad, None, None, None, None, None, None


class _SamplesLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, rows, nhood, ps3, ctr3):
        from . import backend
        logits = logits.contiguous()
        loss, state = backend.patch_loss_samples_fwd(logits, labels, rows, nhood, ps3, ctr3)
        ctx.save_for_backward(logits, labels, rows, nhood, state)
        ctx.geometry = (ps3, ctr3)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        from . import backend
        logits, labels, rows, nhood, state = ctx.saved_tensors
        grad_out = grad_loss.to(torch.float32).reshape(1).contiguous()
        grad = backend.patch_loss_samples_bwd(logits, labels, rows, nhood, ctx.geometry[0], ctx.geometry[1], state, grad_out)
        return grad, None, None, None, None, None


_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def _mask_channel(loss_mask, ndim, shape):
    """the weights of a `loss_mask` (B, Cm, ...) -- channel 0 if Cm == 1, else channel 1 (torch_loss.py:57) -- or
    (B, ...), as float32 of `shape`"""
    if loss_mask.dim() == ndim + 2:
        loss_mask = loss_mask[:, 0 if loss_mask.shape[1] == 1 else 1]
    if tuple(loss_mask.shape) != tuple(shape):
        raise ValueError("loss_mask selects %s: %s expected" % (tuple(loss_mask.shape), tuple(shape)))
    return loss_mask.to(torch.float32)


def _bce_torch(x, G):
    return torch.nn.functional.binary_cross_entropy_with_logits(x, G, reduction="none")


def patch_bce_from_labels(pred_logits, gt_labels, nhood, loss_mask=None, *, box=None, num_channels=None, check=True,
                          want_counts=False):
    """MaskedBCEWithLogitsLoss(pred_logits, seg_to_affgraph_*_multi_torch(gt_labels, nhood), loss_mask) without the
    target: `pred_logits` (B, E, Z, Y, X) or (B, E, Y, X) float32 / float16 / bfloat16 (float64 too on the CPU),
    `gt_labels` (B, L, ...) of an integer or bool type, `nhood` (E, 3) / (E, 2), `loss_mask` (B, Cm, ...) or (B, ...)
    of any float / bool / integer type or None.  `box` = (z0, z1, y0, y1, x0, x1) (2-d: y0, y1, x0, x1) names the
    voxels of the labels the logits belong to; it is required when the two spatial shapes differ.  `num_channels`
    defaults to E.  `check` as in train_util: one synchronisation that validates ids and weights; `check=False`
    makes none.  Returns the 0-dim loss (float32 on the device), differentiable ONCE with respect to the logits;
    with `want_counts` (loss, counts), counts the int64 (x > 0, G, x > 0 and G) over all elements."""
    ndim = pred_logits.dim() - 2
    if ndim not in (2, 3) or gt_labels.dim() != ndim + 2:
        raise ValueError("logits (B, E, ...) of shape %s and labels (B, L, ...) of shape %s: 2 or 3 spatial axes"
                         % (tuple(pred_logits.shape), tuple(gt_labels.shape)))
    tu._int_kind(str(gt_labels.dtype), "labels")
    B, E = int(pred_logits.shape[0]), int(pred_logits.shape[1])
    spatial = tuple(int(s) for s in gt_labels.shape[-ndim:])
    ext = tuple(int(s) for s in pred_logits.shape[-ndim:])
    if box is None:
        if ext != spatial:
            raise ValueError("logits cover %s and the labels %s: say which part with box=" % (ext, spatial))
        box = tuple(v for s in spatial for v in (0, s))
    box = tuple(int(v) for v in box)
    if len(box) != 2 * ndim:
        raise ValueError("box has %d entries: %d expected" % (len(box), 2 * ndim))
    if any(a < 0 or b > s or a >= b for a, b, s in zip(box[0::2], box[1::2], spatial)):
        raise ValueError("box %s is empty or leaves the volume %s" % (box, spatial))
    if tuple(b - a for a, b in zip(box[0::2], box[1::2])) != ext or int(gt_labels.shape[0]) != B:
        raise ValueError("logits of shape %s do not fit box %s of %d batch items" % (tuple(pred_logits.shape), box,
                                                                                     int(gt_labels.shape[0])))
    if ndim == 2:
        box = (0, 1) + box
    ext3 = (1,) * (3 - ndim) + ext
    lead = (B, int(gt_labels.shape[1]))
    nch = float(E if num_channels is None else num_channels)
    weight = None if loss_mask is None else _mask_channel(loss_mask, ndim, (B,) + ext).reshape((B,) + ext3)

    if tu._on_device(pred_logits):
        if pred_logits.dtype not in _FLOATS:
            raise ValueError("device logits are float32, float16 or bfloat16, got %s" % pred_logits.dtype)
        if E == 0:
            raise ValueError("no edges: nhood is empty")
        d_nhood = tu._device_nhood(nhood, pred_logits.device, ndim)
        if int(d_nhood.shape[0]) != E:
            raise ValueError("%d logit channels for %d offsets" % (E, int(d_nhood.shape[0])))
        if check:
            flags, msgs = tu._label_checks(gt_labels, False)
            if weight is not None:
                flags.append(~(weight >= 0).all())
                msgs.append("loss_mask holds negative or NaN weights")
            tu._raise_if(flags, msgs)
        labels = gt_labels.reshape(lead + (1,) * (3 - ndim) + spatial).to(device=pred_logits.device, dtype=torch.int32).contiguous()
        if weight is not None:
            weight = weight.to(pred_logits.device).contiguous()
        loss, counts = _DenseLoss.apply(pred_logits.reshape((B, E) + ext3), labels, d_nhood, weight, box, nch, bool(want_counts))
        return (loss, counts) if want_counts else loss

    # CPU tensors: plain torch over the NumPy target, autograd by torch
    host = tu._np_of(gt_labels)
    if check:
        tu._host_label_checks(host, False)
        if weight is not None and not bool((weight >= 0).all()):
            raise ValueError("loss_mask holds negative or NaN weights")
    h_nhood = tu._host_nhood(nhood, ndim)
    if len(h_nhood) != E:
        raise ValueError("%d logit channels for %d offsets" % (E, len(h_nhood)))
    G = torch.from_numpy(tu.gt_affs_dense_host(host.reshape(lead + (1,) * (3 - ndim) + spatial), h_nhood, box))
    x = pred_logits.reshape((B, E) + ext3)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    G = G.to(x.dtype)
    if weight is None:
        loss = _bce_torch(x, G).mean() if x.numel() else x.sum()
    else:
        w = weight.to(x.dtype)[:, None]
        live = (w != 0).expand_as(x)
        cnt = nch * float(w.sum())
        # a voxel without weight is taken out BEFORE the loss: its logits may hold anything
        total = (_bce_torch(torch.where(live, x, torch.zeros_like(x)), G) * w).sum()
        loss = total / cnt if cnt != 0 else total * 0.0
    if want_counts:
        pos, g = x.detach() > 0, G != 0
        return loss, torch.stack([pos.sum(), g.sum(), (pos & g).sum()]).to(torch.int64)
    return loss


def patch_bce_from_label_samples(pred_logits, gt_labels, nhood, ps, psH, samples_loc, check=True):
    """The `train_code` form: `pred_logits` (N, E) or (N, 1, ps, ...) as the decoder returns them, against
    seg_to_affgraph_*_multi_torch_code(gt_labels, nhood, ps, psH, samples_loc) -- `gt_labels` (B, L, ...),
    `samples_loc` (N, 1 + d) rows (b, z, y, x) / (b, y, x), the corners of the patches -- as the mean over N E
    elements (torch_loss.py:129 passes no mask here).  N = 0 gives 0.  Differentiable once in the logits."""
    ndim = gt_labels.dim() - 2
    if ndim not in (2, 3):
        raise ValueError("labels of shape %s: (B, L, Z, Y, X) or (B, L, Y, X)" % (tuple(gt_labels.shape),))
    tu._int_kind(str(gt_labels.dtype), "labels")
    ps3, _ = tu._sides(ps, ndim, "ps")
    _, ctr3 = tu._sides(psH, ndim, "psH")
    if any(p < 1 for p in ps3) or any(c < 0 or c >= p for c, p in zip(ctr3, ps3)):
        raise ValueError("centre %s outside the patch %s" % (ctr3[3 - ndim:], ps3[3 - ndim:]))
    if len(set(ps3[3 - ndim:])) != 1:
        raise ValueError("the patch is cubic in the reference: ps = %s" % (ps3[3 - ndim:],))
    wrap_by = ps3[-1]
    B, L = int(gt_labels.shape[0]), int(gt_labels.shape[1])
    spatial = tuple(int(s) for s in gt_labels.shape[-ndim:])
    size3 = (1,) * (3 - ndim) + spatial
    N = int(pred_logits.shape[0])
    x = pred_logits.reshape(N, int(np.prod(pred_logits.shape[1:])))
    top = [B - 1] + [s - p for s, p in zip(size3, ps3)]
    leaves = "a sample patch of side %d leaves the volume %s (or its batch index the batch of %d)" % (wrap_by, spatial, B)

    if tu._on_device(pred_logits):
        if pred_logits.dtype not in _FLOATS:
            raise ValueError("device logits are float32, float16 or bfloat16, got %s" % pred_logits.dtype)
        dev = pred_logits.device
        d_nhood = tu._device_nhood(nhood, dev, ndim, wrap=wrap_by)
        E = int(d_nhood.shape[0])
        if int(x.shape[1]) != E and N:
            raise ValueError("logits of shape %s: (%d, %d) expected" % (tuple(pred_logits.shape), N, E))
        loc = samples_loc if tu._is_tensor(samples_loc) else torch.as_tensor(np.asarray(samples_loc, dtype=np.int64))
        if N == 0 or loc.numel() == 0:
            if N != 0 or loc.numel() != 0:
                raise ValueError("%d rows of logits for %d samples" % (N, int(loc.shape[0]) if loc.dim() else 0))
            return x.to(torch.float32).sum()
        if loc.dim() != 2 or loc.shape[1] != ndim + 1 or int(loc.shape[0]) != N:
            raise ValueError("samples_loc of shape %s: (%d, %d)" % (tuple(loc.shape), N, ndim + 1))
        tu._int_kind(str(loc.dtype), "samples_loc")
        loc = loc.to(device=dev, dtype=torch.int64)
        parts = [loc[:, :1]] + ([torch.zeros_like(loc[:, :1])] if ndim == 2 else []) + [loc[:, 1:]]
        rows = torch.cat(parts, dim=1)
        if check:
            flags, msgs = tu._label_checks(gt_labels, False)
            flags.append(((rows < 0) | (rows > torch.tensor(top, dtype=torch.int64, device=dev))).any())
            msgs.append(leaves)
            tu._raise_if(flags, msgs)
        labels = gt_labels.reshape((B, L) + size3).to(device=dev, dtype=torch.int32).contiguous()
        rows = rows.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
        return _SamplesLoss.apply(x, labels, rows, d_nhood, ps3, ctr3)

    host = tu._np_of(gt_labels)
    h_nhood = tu._host_nhood(nhood, ndim, wrap=wrap_by)
    loc = np.asarray(tu._np_of(samples_loc))
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    if N == 0 or loc.size == 0:
        if N != 0 or loc.size != 0:
            raise ValueError("%d rows of logits for %d samples" % (N, len(loc)))
        return x.sum()
    if loc.ndim != 2 or loc.shape[1] != ndim + 1 or len(loc) != N or int(x.shape[1]) != len(h_nhood):
        raise ValueError("logits of shape %s and samples_loc of shape %s: (N, %d) and (N, %d)"
                         % (tuple(pred_logits.shape), loc.shape, len(h_nhood), ndim + 1))
    tu._int_kind(str(loc.dtype), "samples_loc")
    loc = loc.astype(np.int64)
    parts = [loc[:, :1]] + ([np.zeros_like(loc[:, :1])] if ndim == 2 else []) + [loc[:, 1:]]
    rows = np.concatenate(parts, axis=1)
    if check:
        tu._host_label_checks(host, False)
        if ((rows < 0) | (rows > np.array(top))).any():
            raise ValueError(leaves)
    G = torch.from_numpy(tu.gt_affs_samples_host(host.reshape((B, L) + size3), rows, h_nhood, ps3, ctr3)).to(x.dtype)
    return _bce_torch(x, G).mean()


class PatchLossFromLabels(torch.nn.Module):
    """The reference's `patch_loss` (torch_loss.py:86-87, :127-129) fed with the labels instead of the target.
    `num_channels`: the divisor's factor of the masked form (the reference passes the patch size; default E).
    forward(pred_logits, gt_labels, nhood, loss_mask=None, box=None) is `patch_bce_from_labels`; with
    `samples_loc` (and `ps`, `psH`) it is `patch_bce_from_label_samples`, which takes no mask."""

    def __init__(self, num_channels=None, check=True):
        super().__init__()
        self.num_channels = num_channels
        self.check = check

    def forward(self, pred_logits, gt_labels, nhood, loss_mask=None, box=None, ps=None, psH=None, samples_loc=None):
        if samples_loc is not None:
            return patch_bce_from_label_samples(pred_logits, gt_labels, nhood, ps, psH, samples_loc, check=self.check)
        return patch_bce_from_labels(pred_logits, gt_labels, nhood, loss_mask, box=box, num_channels=self.num_channels,
                                     check=self.check)
