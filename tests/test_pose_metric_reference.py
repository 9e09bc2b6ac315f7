"""The namesakes of the reference's vggsfm/utils/metric.py and vggsfm/utils/align.py (vggsfm_amd/utils/metric.py,
vggsfm_amd/utils/align.py) against what the reference's own functions returned for the same seeded inputs, recorded in
tests/golden/reference_calls/pose_metric.npz (oracle/ref_replay.py; re-recorded by running this module with
VGG_RECORD_REFERENCE=1 where the reference tree exists).  S = 6 cameras.  "Agree to tol" is |ours - reference| <= tol x
max(1, the largest magnitude of the reference's output): 1e-6 for float32 inputs, 1e-12 for float64 inputs."""
import numpy as np
import pytest
import torch

from oracle import ref_replay
from tests import sim3_cases as SC
from vggsfm_amd.utils import align, metric

REF = ref_replay.calls("pose_metric")
R_METRIC, R_ALIGN = REF.module("vggsfm.utils.metric"), REF.module("vggsfm.utils.align")
S = 6
TOL = {torch.float32: 1e-6, torch.float64: 1e-12}


def _agree(ours, ref, tol):
    ours = ours if isinstance(ours, (tuple, list)) else (ours,)
    ref = ref if isinstance(ref, (tuple, list)) else (ref,)
    assert len(ours) == len(ref)
    for a, b in zip(ours, ref):
        a, b = (np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64) for x in (a, b))
        assert a.shape == b.shape and np.abs(a - b).max(initial=0) <= tol * max(1.0, np.abs(b).max(initial=0))


def _poses(dtype):
    pred, gt = SC.pose_set(S, 81, rot_noise=0.3, trans_noise=0.5)
    return torch.from_numpy(pred).to(dtype), torch.from_numpy(gt).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_angles_and_auc(dtype):
    pred, gt = _poses(dtype)
    rot = metric.rotation_angle(gt[:, :, :3], pred[:, :, :3])
    _agree(rot, R_METRIC.rotation_angle(gt[:, :, :3], pred[:, :, :3]), TOL[dtype])
    _agree(metric.rotation_angle(gt[:, :, :3], pred[:, :, :3], batch_size=2),
           R_METRIC.rotation_angle(gt[:, :, :3], pred[:, :, :3], batch_size=2), TOL[dtype])
    trans = metric.translation_angle(gt[:, :, 3], pred[:, :, 3])
    _agree(trans, R_METRIC.translation_angle(gt[:, :, 3], pred[:, :, 3]), TOL[dtype])
    _agree(metric.translation_angle(gt[:, :, 3], pred[:, :, 3], ambiguity=False),
           R_METRIC.translation_angle(gt[:, :, 3], pred[:, :, 3], ambiguity=False), TOL[dtype])
    # errors spread over the bins: 40 x the angles above, capped at 29.5 degrees
    r, t = (40 * rot).clamp(max=29.5), (40 * trans).clamp(max=29.5)
    _agree(metric.calculate_auc(r, t), R_METRIC.calculate_auc(r, t), TOL[dtype])
    _agree(metric.calculate_auc(r, t, max_threshold=10, return_list=True),
           R_METRIC.calculate_auc(r, t, max_threshold=10, return_list=True), TOL[dtype])
    _agree(metric.calculate_auc_np(r.numpy(), t.numpy()), R_METRIC.calculate_auc_np(r.numpy(), t.numpy()), TOL[dtype])
    _agree(metric.calculate_auc_np(r.numpy(), t.numpy(), max_threshold=5),
           R_METRIC.calculate_auc_np(r.numpy(), t.numpy(), max_threshold=5), TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_closed_form_inverses(dtype):
    pred, _ = _poses(dtype)
    cv = torch.eye(4, dtype=dtype)[None].repeat(S, 1, 1)
    cv[:, :3] = pred
    p3d = cv.transpose(1, 2).contiguous()
    _agree(metric.closed_form_inverse_OpenCV(cv), R_METRIC.closed_form_inverse_OpenCV(cv), TOL[dtype])
    _agree(metric.closed_form_inverse(p3d), R_METRIC.closed_form_inverse(p3d), TOL[dtype])
    assert torch.allclose(metric.closed_form_inverse_OpenCV(cv) @ cv, torch.eye(4, dtype=dtype).expand(S, 4, 4), atol=1e-5)
    i1, i2 = metric.batched_all_pairs(2, 4)
    assert i1.tolist() == [0, 0, 0, 1, 1, 2, 4, 4, 4, 5, 5, 6] and i2.tolist() == [1, 2, 3, 2, 3, 3, 5, 6, 7, 6, 7, 7]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_alignment(dtype):
    pred, gt = _poses(dtype)
    ours = align.align_camera_extrinsics(pred, gt)
    ref = R_ALIGN.align_camera_extrinsics(pred, gt)
    _agree(ours, ref, TOL[dtype])
    _agree(align.align_camera_extrinsics(pred, gt, estimate_scale=False), R_ALIGN.align_camera_extrinsics(pred, gt, estimate_scale=False),
           TOL[dtype])
    R, T, s = ref
    _agree(align.apply_transformation(pred, R, T, s), R_ALIGN.apply_transformation(pred, R, T, s), TOL[dtype])
    _agree(align.apply_transformation(pred, R, T, s, return_extri=False), R_ALIGN.apply_transformation(pred, R, T, s, return_extri=False),
           TOL[dtype])
