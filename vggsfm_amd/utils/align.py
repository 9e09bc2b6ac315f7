"""The reference's vggsfm/utils/align.py by its own names and parameter lists; the arithmetic lives in vggsfm_amd/video.py,
whose window alignment uses it.  For the Sim(3) between two reconstructions see vggsfm_amd/sim3.py."""
from .. import video


def align_camera_extrinsics(cameras_src, cameras_tgt, estimate_scale=True, eps=1e-9):
    """(B,3,4) source and target cameras, OpenCV convention -> (align_t_R (1,3,3), align_t_T (1,3), align_t_s)."""
    return video.align_camera_extrinsics(cameras_src, cameras_tgt, estimate_scale=estimate_scale, eps=eps)


def apply_transformation(cameras_src, align_t_R, align_t_T, align_t_s, return_extri=True):
    """R_i <- R_i align_t_R, t_i <- R_i align_t_T + align_t_s t_i; (B,3,4), or (R, t) when return_extri is False."""
    return video.apply_transformation(cameras_src, align_t_R, align_t_T, align_t_s, return_extri=return_extri)
