"""`visualize_instances` of the reference's `visualize` task (PatchPerPix/visualize/instances.py:17-79): an
instance map as a coloured picture."""
import numpy as np

from .. import minipng, postprocess
from ..vote_instances import io_hdflike


def visualize_instances(label_fn, label_key, output_file, max_axis=None, show_outline=False,
                        raw_file=None, raw_key=None):
    """instances.py:17-79: dataset `label_key` of the ``.zarr`` / ``.hdf`` file `label_fn`, squeezed, the maximum
    along `max_axis` when that is given, coloured by `postprocess.color` (the reference's draw sequence: a
    caller who seeds ``np.random`` gets the reference's picture), ``astype(np.uint8)``, written as a PNG
    (minipng).  A map that is not 2-d after the projection raises ValueError (the reference hands it to
    ``imsave`` as it is).  ``show_outline`` needs the ``colorcet`` package and stays refused; `raw_file` /
    `raw_key` are read by that branch only."""
    if show_outline:
        raise NotImplementedError("show_outline=True needs the colorcet package, which this repository does not use")
    if not label_fn.rstrip("/").endswith((".zarr", ".hdf")):
        raise NotImplementedError("visualize_instances reads .zarr and .hdf files, not %s" % label_fn)
    if not output_file.endswith(".png"):
        raise NotImplementedError("visualize_instances writes .png files, not %s" % output_file)
    with io_hdflike.open_container(label_fn, "r") as inf:
        label = np.squeeze(np.array(inf[label_key]))
    if max_axis is not None:
        label = np.max(label, axis=max_axis)
    if label.ndim != 2:
        raise ValueError("a label array of shape %s is no picture: give max_axis, or a 2-d map" % (label.shape,))
    colored = postprocess.color(label)
    minipng.write(output_file, colored.astype(np.uint8))
