"""The reference's `visualize` package (PatchPerPix/visualize/__init__.py), under its names."""
from .patches import visualize_patches  # noqa: F401
from .instances import visualize_instances  # noqa: F401
