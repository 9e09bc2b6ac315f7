"""Writes tests/golden/klt_scene_a.npz: the tracks of the NumPy restatement of the tracker (tests/klt_cases.py: detector and
track_features, on the CPU) on scene A -- 8 frames of 128 x 160 rendered from 120 Gaussian blobs at projected 3D points --
with the scene's parameters.  tests/test_gpu_klt_reconstruct.py reconstructs from these tracks as its yardstick.
    python scripts/make_golden_klt.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import klt_cases as C  # noqa: E402


def main():
    sc = C.projected_scene(**C.SCENE_A)
    query, track, vis, score = C.restated_tracks(sc["images"], **C.SCENE_A_TRACKER)
    print(f"{len(query)} tracks; visible per frame {vis.mean(1).round(3).tolist()}")
    out = os.path.join(ROOT, "tests", "golden", "klt_scene_a.npz")
    np.savez_compressed(out, tracks=track.astype(np.float32), vis=vis.astype(np.float32), score=score.astype(np.float32),
                        query=query, points3D=sc["points3D"], amplitude=sc["amplitude"], sigma=sc["sigma"],
                        extrinsics=sc["extrinsics"], intrinsics=sc["intrinsics"],
                        **{f"scene_{k}": np.asarray(v) for k, v in C.SCENE_A.items()})
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
