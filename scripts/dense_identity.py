"""One SHA-256 per tensor that the dense stage and the tracker return on the small cases of the GPU tests: every case of
tests/mvs_cases.py, tests/patchmatch_cases.py, tests/fusion_cases.py, tests/meshing_cases.py and tests/klt_cases.py, once,
through the public functions of vggsfm_amd; one line per call, its tensors' hashes in the order returned.  Two builds that
compute the same bits write the same file (profiles/dense_refactor_identity_{parent,change}.txt).  A tool, not a test: the
hashes belong to one compiler version.

    python scripts/dense_identity.py --out FILE        # needs an MI355X; a few seconds
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import fusion_cases as FC  # noqa: E402
from tests import klt_cases as KC  # noqa: E402
from tests import meshing_cases as VC  # noqa: E402
from tests import mvs_cases as MC  # noqa: E402
from tests import patchmatch_cases as PC  # noqa: E402
from vggsfm_amd import fusion, klt, meshing, mvs  # noqa: E402
from vggsfm_amd import patchmatch as PM  # noqa: E402

LINES = []


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def record(label, tensors):
    """one line per call: the label, then per returned tensor the SHA-256 of its bytes (`none` where there is none)"""
    digests = ["none" if t is None else hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()
               for t in tensors]
    LINES.append(" ".join([label.replace(" ", ":")] + digests))


def run_mvs():
    for name, c in MC.sweep_cases()[0].items():
        record(f"mvs.plane_sweep {name}",
               mvs.plane_sweep(D(c["frames"]), D(c["poses"]), D(c["cams"]), c["ref"], c["sources"], c["depth_near"], c["depth_far"],
                               c["num_planes"], c["radius"], c["min_views"], c["min_variance"], c["min_conf"], return_cost=True,
                               rays=D(c["rays"])))
    for name, c in MC.filter_cases().items():
        record(f"mvs.filter_consistent {name}",
               mvs.filter_consistent(D(c["depth"]), D(c["poses"]), D(c["cams"]), c["ref"], c["sources"], c["rel_depth_tol"],
                                     c["reproj_tol"], c["min_consistent"], rays=D(c["rays"]), ray_index=c["ray_index"]))


def run_patchmatch():
    for name, c in PC.cases().items():
        record(f"patchmatch.refine_depth {name}",
               PM.refine_depth(D(c["frames"]), D(c["poses"]), D(c["cams"]), c["ref"], c["sources"], c["depth_near"],
                               c["depth_far"], D(c["init_depth"]), D(c["init_normals"]), c["iterations"], c["radius"],
                               c["min_views"], c["min_variance"], c["min_conf"], c["seed"], c["depth_step"], c["slope_step"],
                               c["max_tilt_deg"], D(c["rays"]), c["num_planes"]))


def run_fusion():
    for name, c in FC.normals_cases().items():
        record(f"fusion.depth_normals {name}",
               [fusion.depth_normals(D(c["depth"]), D(c["poses"]), np.zeros((len(c["depth"]), 4)), c["max_rel_jump"],
                                     rays=D(c["rays"]), ray_index=c["ray_index"])])
    for name, c in FC.fusion_cases().items():
        c = dict(c)
        angle = c.pop("max_normal_angle_deg", FC.MAX_ANGLE_DEG)
        cloud, claimed = fusion.fuse_depth_maps(D(c["depth"]), D(c["poses"]), D(c["cams"]), c["sources"], D(c["colors"]),
                                                D(c["normals"]), c["rel_depth_tol"], c["reproj_tol"], angle, c["min_views"],
                                                c["view_order"], rays=D(c["rays"]), ray_index=c["ray_index"],
                                                return_claimed=True)
        record(f"fusion.fuse_depth_maps {name}", list(cloud) + [claimed])


def record_mesh(label, vol, min_weight):
    count = vol.count(min_weight)
    record(f"{label} count", [count[k] for k in sorted(count)])
    record(f"{label} extract", vol.extract(min_weight))


def run_meshing():
    for name, c in VC.integration_cases().items():
        color = c.get("frames") is not None
        vol = meshing.TSDFVolume(c["origin"], c["voxel"], c["dims"], color=color)
        vol.integrate(D(c["depth"]), D(c["poses"]), D(c["cams"]), D(c["weights"]), D(c["frames"]), c["trunc"])
        record(f"meshing.integrate {name}", (vol.tsdf_sum, vol.weight_sum, vol.rgb_sum))
        record_mesh(f"meshing {name}", vol, c["min_weight"])
    for name, c in VC.volume_cases().items():
        vol = meshing.TSDFVolume(c["origin"], c["voxel"], c["dims"], color=c["rgb_sum"] is not None)
        vol.tsdf_sum.copy_(D(c["tsdf_sum"]))
        vol.weight_sum.copy_(D(c["weight_sum"]))
        if c["rgb_sum"] is not None:
            vol.rgb_sum.copy_(D(c["rgb_sum"]))
        record_mesh(f"meshing volume {name}", vol, c["min_weight"])


def run_klt():
    for name, c in KC.lk_cases().items():
        pyr = klt.build_pyramid(D(c["frames"]), c["levels"])
        record(f"klt.track_pair {name}", klt.track_pair(pyr, 0, 1, D(c["points"]), D(c.get("guess")), **c["kw"]))
    frames, centres, _ = KC.sequence_case()
    record("klt.track_features sequence", klt.track_features(D(frames), D(centres)))
    record("klt.detect_features sequence", [klt.detect_features(D(frames), 0, 40)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    for run in (run_mvs, run_patchmatch, run_fusion, run_meshing, run_klt):
        run()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"{len(LINES)} calls hashed -> {args.out}")


if __name__ == "__main__":
    main()
