"""The deletion rule of the 3-d thinning as one function of a 27-bit neighbourhood word
(csrc/ppp_skel_rule.hpp, what the device kernels of csrc/ppp_skeleton.hip evaluate) against the
predicates of the host thinning (csrc/ppp_host_skel.cpp) on EVERY neighbourhood; the size query of the
device entry point; the device backend's refusal to run without a device.  No GPU needed."""
import numpy as np
import pytest

from patchperpix_amd import backend


def test_rule_agrees_with_the_host_predicates_on_all_neighbourhoods():
    """all 2^26 patterns of the 26 neighbours, in 16 chunks (each split over up to 16 threads by the
    entry point: one core takes about 45 s for the sweep, the threads about 5 s)"""
    chunk = 1 << 22
    bad = [backend.host_skel_rule_mismatches(first, chunk) for first in range(0, 1 << 26, chunk)]
    assert bad == [0] * 16
    # the single-threaded path of short ranges, the end of the domain, and what lies beyond it
    assert backend.host_skel_rule_mismatches(0, 1 << 12) == 0
    assert backend.host_skel_rule_mismatches((1 << 26) - 1000, 1000) == 0
    assert backend.host_skel_rule_mismatches(1 << 26, 0) == 0
    with pytest.raises(ValueError):
        backend.host_skel_rule_mismatches((1 << 26) - 1000, 1001)


def test_workspace_query_grows_with_every_extent_and_refuses_2_to_31_voxels():
    q = backend.lib().ppp_skeletonize_3d_workspace_bytes
    for shape in [(1, 1, 1), (1, 70, 70), (3, 5, 70), (40, 40, 40), (140, 140, 140), (512, 512, 512)]:
        base = q(*shape)
        assert base > 0
        for axis in range(3):
            prev = base
            for step in (1, 2, 31, 64):
                grown = list(shape)
                grown[axis] += step
                now = q(*grown)
                assert now >= prev, (shape, axis, step)
                prev = now
    # two bit images and three lists of about half the voxels: far below a byte map and two id maps
    assert q(512, 512, 512) < 7 * 512 ** 3
    for shape in [(2048, 1024, 1024), (1, 1 << 16, 1 << 15), (1 << 11, 1 << 10, 1 << 10)]:
        assert q(*shape) == -4, shape                       # PPP_ERR_UNSUPPORTED
    assert q(2047, 1024, 1024) > 0
    assert q(0, 4, 4) < 0 and q(4, -1, 4) < 0
    assert q(65536, 2, 2) == -4                             # more slices than a launch has workgroup rows


def test_device_backend_raises_without_a_device(monkeypatch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from patchperpix_amd.vote_instances import vote_instances as vi
    m = np.zeros((9, 9, 20), bool)
    m[3:6, 3:6, 2:18] = True
    monkeypatch.delenv("PPP_SKELETONIZE", raising=False)
    with pytest.raises(RuntimeError, match="no HIP device"):
        vi._skeletonize(m, "ppp_device")
    monkeypatch.setenv("PPP_SKELETONIZE", "ppp_device")
    with pytest.raises(RuntimeError, match="no HIP device"):
        vi._skeletonize(m)
    with pytest.raises(ValueError, match="ppp_device"):
        vi._skeletonize(m, "device")
