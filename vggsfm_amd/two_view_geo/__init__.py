"""Two-view stage in front of the hot path (vggsfm/two_view_geo/): fundamental matrices for all (query frame, other
frame) pairs at once on the device, and essential matrices by 5-point LO-RANSAC for callers with known intrinsics
(DESIGN.md section 16), and EPnP (section 17).  SURVEY.md section 8(f).3; PARITY UNPINNED against the reference."""
from .camera_prior import CameraPrior, geometric_camera_prior  # noqa: F401
from .essential import estimate_essential, relative_pose_from_essential, run_5point  # noqa: F401
from .estimate_preliminary import estimate_preliminary_cameras  # noqa: F401
from .fundamental import estimate_fundamental  # noqa: F401
from .perspective_n_points import EpnpSolution, efficient_pnp  # noqa: F401
from .utils import (calculate_residual_indicator, generate_samples, inlier_by_fundamental,  # noqa: F401
                    sampson_epipolar_distance_batched)
