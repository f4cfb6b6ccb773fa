"""GPU: the reference-side ctypes binding (integration/ppp_reference_binding.py, the C ABI and nothing
else of this repository) reaches ppp_rows_index_build / ppp_rows_expand."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_binding_expands_rows_into_a_box():
    import torch
    spec = importlib.util.spec_from_file_location(
        "ppp_reference_binding", os.path.join(REPO, "integration", "ppp_reference_binding.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    ctx = b.init_cuda()
    rng = np.random.default_rng(5)
    shape, C = (4, 6, 71), 27
    mask = rng.uniform(size=shape) < 0.3
    index, n = b.rows_index_build(mask)
    assert n == int(mask.sum())
    rows = torch.from_numpy(rng.normal(size=(n, C)).astype(np.float16)).cuda()
    box = b.Box(1, 2, 3, 4, 6, 70)                      # z0, y0, x0, z1, y1, x1
    got = b.rows_expand(rows, index, shape, box)
    b.sync(ctx)
    D = np.zeros((C,) + shape, dtype=np.float16)
    D[:, mask] = rows.cpu().numpy().T
    assert np.array_equal(got.cpu().numpy().view(np.uint16), D[:, 1:4, 2:6, 3:70].view(np.uint16))
    b.delete_cuda(ctx)
