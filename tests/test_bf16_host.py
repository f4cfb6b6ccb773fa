"""bfloat16 predictions, the parts that need no GPU: the dtype query of the C ABI, the dtype code and
the pass-through of ``backend.to_device_pred``, and the halo exchange moving bf16 slices bit for bit
(two gloo ranks on the CPU)."""
import os
import socket
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_says_which_dtype_codes_it_reads():
    from patchperpix_amd import backend
    L = backend.lib()
    assert [L.ppp_pred_dtype_supported(c) for c in (0, 1, 2)] == [1, 1, 1]
    assert [L.ppp_pred_dtype_supported(c) for c in (3, -1)] == [0, 0]
    assert (backend.F32, backend.F16, backend.BF16) == (0, 1, 2)


def test_dtype_code_of_a_bf16_tensor():
    import pytest
    import torch
    from patchperpix_amd import backend
    assert backend.pred_dtype_code(torch.zeros(2, dtype=torch.bfloat16)) == backend.BF16 == 2
    assert backend.pred_dtype_code(torch.zeros(2, dtype=torch.float16)) == backend.F16
    assert backend.pred_dtype_code(torch.zeros(2, dtype=torch.float32)) == backend.F32
    with pytest.raises(TypeError):
        backend.pred_dtype_code(torch.zeros(2, dtype=torch.float64))


def test_to_device_pred_keeps_a_bf16_tensor_as_it_is():
    import torch
    from patchperpix_amd import backend
    t = torch.linspace(0, 1, 3 * 4 * 5 * 6).reshape(3, 4, 5, 6).to(torch.bfloat16)
    got = backend.to_device_pred(t, device="cpu")
    assert got.dtype == torch.bfloat16 and got.data_ptr() == t.data_ptr()
    assert backend.NOTES["pred_dtype"] == "bfloat16"
    # a strided view is made contiguous, still without widening
    v = t[:, ::2]
    got = backend.to_device_pred(v, device="cpu")
    assert got.dtype == torch.bfloat16 and got.is_contiguous() and torch.equal(got.view(torch.int16), v.contiguous().view(torch.int16))
    # everything else as before: other dtypes widen to float32, float16 stays
    got = backend.to_device_pred(np.linspace(0, 1, 24).reshape(1, 2, 3, 4), device="cpu")
    assert got.dtype == torch.float32
    got = backend.to_device_pred(np.zeros((1, 2, 3, 4), dtype=np.float16), device="cpu")
    assert got.dtype == torch.float16
    assert backend.NOTES["pred_dtype"] == "float16"
    assert backend.to_device_pred(torch.zeros(2, dtype=torch.float64), device="cpu").dtype == torch.float32
    assert backend.to_device_pred(torch.zeros(2, dtype=torch.float16), device="cpu", keep_f16=False).dtype == torch.float32


HALO_WORKER = r"""
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
from patchperpix_amd import tiling
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
comm = tiling.TorchDistComm()
Z, H = 6, 2
cuts = [0, 2, Z]
a, b = cuts[rank], cuts[rank + 1]
na, nb = max(0, a - H), min(Z, b + H)
# every 16-bit pattern class: normal values, a denormal (2^-133), -0.0, inf, a nan payload
bits = (torch.arange(3 * Z * 4 * 5, dtype=torch.int32) * 181 + 7).to(torch.int16).reshape(3, Z, 4, 5)
bits[0, :, 0, 0] = torch.tensor([0x0001, -0x8000, 0x7F80, 0x7FC1, 0x3F80, 0x0000], dtype=torch.int32).to(torch.int16)
vol = bits.view(torch.bfloat16)
assert vol.shape == (3, 6, 4, 5)
got = tiling.exchange_halo(vol[:, a:b].contiguous(), (a, b), (na, nb), comm, z_axis=1)
assert got.dtype == torch.bfloat16 and got.shape == (3, nb - na, 4, 5), rank
assert torch.equal(got.view(torch.int16), bits[:, na:nb]), rank
# channel-chunked (one channel per step), and in place into a halo-sized buffer
got = tiling.exchange_halo(vol[:, a:b].contiguous(), (a, b), (na, nb), comm, z_axis=1, chunk_bytes=100)
assert torch.equal(got.view(torch.int16), bits[:, na:nb]), rank
buf = torch.zeros((3, nb - na, 4, 5), dtype=torch.bfloat16)
buf[:, a - na:b - na] = vol[:, a:b]
got = tiling.exchange_halo(buf.narrow(1, a - na, b - a), (a, b), (na, nb), comm, z_axis=1, out=buf)
assert got.data_ptr() == buf.data_ptr() and torch.equal(buf.view(torch.int16), bits[:, na:nb]), rank
open(os.path.join({out!r}, "ok%d" % rank), "w").write("ok")
dist.destroy_process_group()
"""


def test_exchange_halo_moves_bf16_slices_bit_for_bit(tmp_path):
    """tiling.exchange_halo of a (3, 6, 4, 5) bf16 block on two gloo ranks, compared as int16 views
    (nan payloads and -0.0 included: a conversion on the way would not keep them)."""
    script = tmp_path / "halo_worker.py"
    script.write_text(HALO_WORKER.format(repo=REPO, out=str(tmp_path)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", port, str(script)], env=env, timeout=600)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(2))
