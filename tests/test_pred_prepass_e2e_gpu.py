"""GPU: to_instance_seg on a resident 24^3 volume with the shipped flags returns the same instance map whether the
prediction is read once for the clean flag, S2's masks and the patch bits (the default) or four times
(PPP_PRED_PREPASS=0) -- for 5^3 and 7^3 patches, and for an unclean prediction (a value equal to the threshold), where
S1 takes its exact classification in both arms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _run(torch, case, ps, pred, switch, monkeypatch):
    """(instances, foreground, what backend.pred_prepass returned in this run, the clean flag S1 was given)"""
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import vote_instances as vi
    from tests_flags import FLYLIGHT_SHIPPED
    if switch is None:
        monkeypatch.delenv("PPP_PRED_PREPASS", raising=False)
    else:
        monkeypatch.setenv("PPP_PRED_PREPASS", switch)
    seen = []
    real = backend.pred_prepass

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(backend, "pred_prepass", spy)
    backend.NOTES.pop("pred_unclean_bits", None)
    kw = dict(FLYLIGHT_SHIPPED, save_no_intermediates=True, sample=1.0, result_folder="/tmp", affinities="x.zarr")
    inst, fg = vi.to_instance_seg(pred.copy(), case["foreground"].copy(), case["foreground"].copy(), case["numinst"].copy(),
                                  np.array(ps), **kw)
    monkeypatch.setattr(backend, "pred_prepass", real)
    return inst, fg, seen, backend.NOTES.get("pred_unclean_bits")


@pytest.mark.parametrize("p,unclean", [(5, False), (7, False), (7, True)])
def test_instances_do_not_depend_on_the_prepass(p, unclean, torch_cuda, monkeypatch):
    from patchperpix_amd import synth
    ps = (p, p, p)
    case = synth.make_case((24, 24, 24), ps, seed=240 + p, cell=[2 * p, 2 * p, 2 * p], overlap_frac=0.02)
    pred = case["pred"].astype(np.float16)
    if unclean:
        # a foreground voxel's partner value exactly at the threshold: votes nowhere, S1's exact path serves the call
        z, y, x = [int(v[0]) for v in np.nonzero(case["foreground"][p:24 - p, p:24 - p, p:24 - p])]
        pred[(p ** 3) // 2 + 1, z + p, y + p, x + p] = 0.5
    inst1, fg1, seen1, bits1 = _run(torch_cuda, case, ps, pred, None, monkeypatch)
    inst0, fg0, seen0, bits0 = _run(torch_cuda, case, ps, pred, "0", monkeypatch)
    assert inst1.any()
    assert np.array_equal(inst1, inst0) and inst1.dtype == inst0.dtype
    assert np.array_equal(fg1, fg0)
    # the default arm took the fused pass (once), the other one the separate launches; both saw the same flag
    assert len(seen1) == 1 and seen1[0] is not None and seen1[0].clean == (2 if unclean else 1)
    assert seen0 == [None]
    assert bits1 == bits0 and (bits1 != 0) == unclean
