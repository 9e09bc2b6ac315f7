"""Pose-error metrics: the names and parameter lists of the reference's vggsfm/utils/metric.py as torch functions, and the
lean forms over the device kernel (csrc/sim3.hip, vggs_pose_pair_errors) that take (S,3,4) world-to-camera extrinsics
in the OpenCV convention and store no 4x4 matrix per pair.  DESIGN.md section 20."""
import numpy as np
import torch

from .. import _lib


def _unit_quaternion(matrix):
    """(...,3,3) rotations -> (...,4) unit quaternions (w, x, y, z), each from the branch of Shepperd's method whose
    divisor is the largest.  The sign is whatever that branch gives: the metrics below square the product."""
    m = matrix
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    four = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], dim=-1)
    root = torch.sqrt(four.clamp(min=0))
    by_w = torch.stack([root[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1)
    by_x = torch.stack([m21 - m12, root[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1)
    by_y = torch.stack([m02 - m20, m10 + m01, root[..., 2] ** 2, m12 + m21], dim=-1)
    by_z = torch.stack([m10 - m01, m20 + m02, m21 + m12, root[..., 3] ** 2], dim=-1)
    cand = torch.stack([by_w, by_x, by_y, by_z], dim=-2) / (2.0 * root[..., None].clamp(min=0.1))
    pick = root.argmax(dim=-1)
    return torch.gather(cand, -2, pick[..., None, None].expand(pick.shape + (1, 4)))[..., 0, :]


def rotation_angle(rot_gt, rot_pred, batch_size=None, eps=1e-15):
    """Angle in degrees between (N,3,3) rotations: arccos(1 - 2 max(1 - (q_pred . q_gt)^2, eps))."""
    dot = (_unit_quaternion(rot_pred) * _unit_quaternion(rot_gt)).sum(dim=1)
    loss = (1 - dot ** 2).clamp(min=eps)
    deg = torch.arccos(1 - 2 * loss) * 180 / np.pi
    return deg if batch_size is None else deg.reshape(batch_size, -1)


def compare_translation_by_angle(t_gt, t, eps=1e-15, default_err=1e6):
    """Angle in radians between the directions of (N,3) translations, sign ignored; default_err where it is not finite."""
    t = t / (torch.norm(t, dim=1, keepdim=True) + eps)
    t_gt = t_gt / (torch.norm(t_gt, dim=1, keepdim=True) + eps)
    loss = torch.clamp_min(1.0 - torch.sum(t * t_gt, dim=1) ** 2, eps)
    err = torch.acos(torch.sqrt(1 - loss))
    err[torch.isnan(err) | torch.isinf(err)] = default_err
    return err


def translation_angle(tvec_gt, tvec_pred, batch_size=None, ambiguity=True):
    deg = compare_translation_by_angle(tvec_gt, tvec_pred) * 180.0 / np.pi
    if ambiguity:
        deg = torch.min(deg, (180 - deg).abs())
    return deg if batch_size is None else deg.reshape(batch_size, -1)


def closed_form_inverse_OpenCV(se3, R=None, T=None):
    """Inverse of (N,4,4) rigid transforms [[R, t], [0, 1]] (column vectors)."""
    R = se3[:, :3, :3] if R is None else R
    T = se3[:, :3, 3:] if T is None else T
    Rt = R.transpose(1, 2)
    out = torch.eye(4, dtype=R.dtype, device=R.device)[None].repeat(len(se3), 1, 1)
    out[:, :3, :3] = Rt
    out[:, :3, 3:] = -Rt.bmm(T)
    return out


def closed_form_inverse(se3, R=None, T=None):
    """Inverse of (N,4,4) rigid transforms [[R, 0], [T, 1]] (row vectors, the PyTorch3D layout)."""
    R = se3[:, :3, :3] if R is None else R
    T = se3[:, 3:, :3] if T is None else T
    Rt = R.transpose(1, 2)
    left = torch.cat((Rt, -T.bmm(Rt)), dim=1)
    return torch.cat((left, se3[:, :, 3:].detach().clone()), dim=-1)


def batched_all_pairs(B, N):
    """Flat indices (i1, i2) of all pairs i < j within each of B groups of N, in the order of torch.combinations."""
    first, second = torch.combinations(torch.arange(N), 2, with_replacement=False).unbind(-1)
    shift = torch.arange(B)[:, None] * N
    return (first[None] + shift).reshape(-1), (second[None] + shift).reshape(-1)


def calculate_auc_np(r_error, t_error, max_threshold=30):
    """(mean of the cumulative normalised histogram of max(r, t) over the bins [0,1), ..., [max_threshold-1,
    max_threshold], the normalised histogram)."""
    worst = np.max(np.concatenate((r_error[:, None], t_error[:, None]), axis=1), axis=1)
    hist, _ = np.histogram(worst, bins=np.arange(max_threshold + 1))
    hist = hist.astype(float) / float(len(worst))
    return np.mean(np.cumsum(hist)), hist


def calculate_auc(r_error, t_error, max_threshold=30, return_list=False):
    """The torch form: max_threshold + 1 equal bins over [0, max_threshold] (torch.histc)."""
    worst, _ = torch.max(torch.stack((r_error, t_error), dim=1), dim=1)
    hist = torch.histc(worst, bins=max_threshold + 1, min=0, max=max_threshold) / float(worst.size(0))
    auc = torch.cumsum(hist, dim=0).mean()
    return (auc, hist) if return_list else auc


def camera_to_rel_deg(pred_cameras, gt_cameras, device, batch_size):
    """Relative rotation and translation errors in degrees over all pairs of each batch; the cameras are anything with
    get_world_to_view_transform().get_matrix() -> (B*N,4,4) in the PyTorch3D layout."""
    with torch.no_grad():
        gt = gt_cameras.get_world_to_view_transform().get_matrix()
        pred = pred_cameras.get_world_to_view_transform().get_matrix()
        i1, i2 = batched_all_pairs(batch_size, gt.shape[0] // batch_size)
        i1 = i1.to(device)
        rel_gt = closed_form_inverse(gt[i1]).bmm(gt[i2])
        rel_pred = closed_form_inverse(pred[i1]).bmm(pred[i2])
        return (rotation_angle(rel_gt[:, :3, :3], rel_pred[:, :3, :3]),
                translation_angle(rel_gt[:, 3, :3], rel_pred[:, 3, :3]))


def pose_pair_errors(extrinsics_pred, extrinsics_gt):
    """(rotation error, translation-direction error) in degrees, each (S (S - 1) / 2,), of the relative poses of all
    pairs i < j (torch.combinations order) of (S,3,4) world-to-camera extrinsics: camera_to_rel_deg on the device."""
    if extrinsics_pred.shape != extrinsics_gt.shape or extrinsics_pred.dim() != 3 or tuple(extrinsics_pred.shape[1:]) != (3, 4):
        raise ValueError(f"extrinsics must both be (S,3,4), got {tuple(extrinsics_pred.shape)} and {tuple(extrinsics_gt.shape)}")
    _lib.require_gpu(extrinsics_pred, extrinsics_gt)
    pred = extrinsics_pred.to(torch.float64).contiguous()
    gt = extrinsics_gt.to(torch.float64).contiguous()
    S = pred.shape[0]
    rot = torch.empty((S * (S - 1) // 2,), dtype=torch.float64, device=pred.device)
    trans = torch.empty_like(rot)
    _lib.check(_lib.lib().vggs_pose_pair_errors(pred, gt, S, rot, trans, _lib.stream_ptr()), "vggs_pose_pair_errors")
    return rot, trans


def pose_auc(extrinsics_pred, extrinsics_gt, max_threshold=30):
    """calculate_auc of pose_pair_errors."""
    rot, trans = pose_pair_errors(extrinsics_pred, extrinsics_gt)
    return calculate_auc(rot, trans, max_threshold=max_threshold)
