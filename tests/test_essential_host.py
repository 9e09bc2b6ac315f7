"""5-point essential matrices, the part that needs no GPU: argument validation before the library is touched, the
independent CPU solver's own known-answer test, and the caps stored in the golden files."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import essential_cases as EC
from vggsfm_amd import _lib
from vggsfm_amd import two_view_geo as TV
from vggsfm_amd.two_view_geo import essential as ES



def test_entries_refuse_bad_sizes_before_any_launch():
    L = _lib.lib()
    one = torch.zeros(64, dtype=torch.float64)          # (host memory: nothing is launched on these paths)
    bad, unsupported = -1, -4
    assert L.vgge_emat_five_point(one, one, one, 1, 4, 4, one, one, None) == bad            # fewer than five points
    assert L.vgge_emat_five_point(one, one, one, 1, 8, 0, one, one, None) == bad
    assert L.vgge_emat_five_point(None, one, one, 1, 8, 4, one, one, None) == bad
    assert L.vgge_emat_five_point(None, None, None, 0, 8, 4, None, None, None) == 0         # no pairs: a no-op
    assert L.vgge_emat_five_point(one, one, one, 65536, 8, 4, one, one, None) == unsupported
    assert L.vgge_emat_solve(one, one, None, 1, 4, one, one, None) == bad
    assert L.vgge_emat_solve(one, one, None, -1, 8, one, one, None) == bad
    assert L.vgge_emat_solve(None, None, None, 0, 8, None, None, None) == 0
    assert L.vgge_emat_solve(one, one, None, 2 ** 31, 8, one, one, None) == unsupported
    assert L.vgge_emat_score(one, one, one, one, None, 1, 8, 4, one, one, None) == bad      # no thresholds
    assert L.vgge_emat_score(one, one, one, one, one, 1, 8, 0, one, one, None) == bad
    assert L.vgge_emat_score(one, one, one, one, one, 65536, 8, 4, one, one, None) == unsupported
    assert L.vgge_emat_refine(one, one, one, one, one, one, 1, 8, 4, 0, one, one, None) == bad
    assert L.vgge_emat_refine(one, one, one, one, None, one, 1, 8, 4, 2, one, one, None) == bad
    assert L.vgge_emat_refine(one, one, one, one, one, one, 65536, 8, 4, 2, one, one, None) == unsupported
    with pytest.raises(ctypes.ArgumentError):
        L.vgge_emat_five_point(one, one, one, 1, 2 ** 31, 4, one, one, None)


# --- the public functions -------------------------------------------------------------------------------------------------
def test_exports():
    assert TV.estimate_essential is ES.estimate_essential and TV.run_5point is ES.run_5point
    assert TV.relative_pose_from_essential is ES.relative_pose_from_essential


def test_arguments_are_validated_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    p, k = torch.zeros(2, 8, 2, dtype=torch.float64), torch.ones(2, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="at least 5"):
        ES.estimate_essential(p[:, :4], p[:, :4], k, k)
    with pytest.raises(ValueError):
        ES.estimate_essential(p, p[:, :7], k, k)
    with pytest.raises(ValueError, match=r"\(B,4\)"):
        ES.estimate_essential(p, p, k[:, :2], k)
    with pytest.raises(ValueError, match="lo_num"):
        ES.estimate_essential(p, p, k, k, lo_num=-1)
    with pytest.raises(ValueError, match="samples"):
        ES.estimate_essential(p, p, k, k, samples=np.zeros((4, 7), np.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ES.estimate_essential(p, p, k, k)
    with pytest.raises(ValueError, match="at least 5"):
        ES.run_5point(p[:, :4], p[:, :4])
    with pytest.raises(ValueError, match="masks"):
        ES.run_5point(p, p, masks=torch.ones(2, 7))
    with pytest.raises(NotImplementedError):
        ES.run_5point(p, p, weights=torch.ones(2, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ES.run_5point(p, p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ES.relative_pose_from_essential(torch.eye(3)[None], p[:1], p[:1], k[:1], k[:1])


# --- the CPU solver -----------------------------------------------------------------------------------------------------------
def test_cpu_solver_finds_the_true_essential_matrix():
    rng = np.random.default_rng(0)
    f, pp = np.array([800.0, 820, 790, 805]), np.array([320.0, 240, 330, 250])
    worst, counts = 0.0, set()
    for _ in range(40):
        px1, px2, R, t, _ = EC.two_view_scene(rng, 5, f, pp)
        p1, p2 = EC.normalise(px1, px2, f, pp)
        Es = EC.five_point(p1, p2)
        counts.add(len(Es))
        worst = max(worst, EC.distance(Es, EC.true_essential(R, t)).min())
        for E in Es:
            assert max(EC.constraint_residuals(E, p1, p2)) <= EC.CONSTRAINT_BOUND
    print(f"CPU solver: true E within {worst:.2e}; real solutions per sample {sorted(counts)}")
    assert worst <= 1e-8 and counts <= {2, 4, 6, 8, 10} and len(counts) > 1


def test_cpu_solver_on_many_weighted_matches():
    rng = np.random.default_rng(1)
    px1, px2, R, t, inl = EC.two_view_scene(rng, 60, np.ones(4), np.zeros(4), outliers=0.25)
    Es = EC.five_point(px1, px2, inl.astype(np.float64))
    assert EC.distance(Es, EC.true_essential(R, t)).min() <= 1e-8


# --- the golden files ---------------------------------------------------------------------------------------------------
def test_every_golden_file_is_known_and_small():
    assert sorted(os.path.basename(f) for f in EC.files()) == sorted(f"essential_{n}.npz" for n in EC.ALL_FILES)
    assert all(os.path.getsize(f) < 1_000_000 for f in EC.files())


def test_golden_files_obey_their_caps():
    g = EC.load("solver")
    assert float(g["cap"]) == EC.CAP and g["admit_sample"].dtype == np.bool_
    assert 1.0 - g["admit_sample"].mean() <= EC.CAP
    assert g["points1"].shape == (3, 64, 2) and g["samples"].shape == (64, 5) and g["cpu_emat"].shape == (3, 64, 10, 3, 3)
    # the stored candidates are what the CPU solver gives today
    for b, h in ((0, 0), (1, 17), (2, 63)):
        idx = g["samples"][h]
        Es = EC.five_point(g["points1"][b, idx], g["points2"][b, idx])
        assert len(Es) == g["cpu_num"][b, h] and EC.set_deviation(Es, g["cpu_emat"][b, h, :len(Es)]) <= 1e-9
    for name in EC.FLOW_CASES:
        g = EC.load(name)
        assert float(g["cap"]) == EC.CAP and g["admit_pair"].all() and 1.0 - g["admit_match"].mean() <= EC.CAP
        assert g["points1"].dtype == np.float32 and g["points1"].shape == (2, 64, 2) and g["samples"].shape == (16, 5)
        assert int(g["lo_num"]) >= 10 * len(g["samples"])
        thr = (float(g["max_error"]) / g["focal_length"].astype(np.float64).mean(1)) ** 2
        # the reference's float32 mask equals the float64 one on the admitted matches
        assert ((g["ref_residuals"] <= thr[:, None]) == g["ref_inlier_mask"])[g["admit_match"]].all()
        assert EC.distance(g["ref_emat"], g["ref_emat"]).max() == 0 and g["ref_emat"].dtype == np.float64
    equal, mixed = EC.load("flow_equal")["focal_length"], EC.load("flow_mixed")["focal_length"]
    assert len(np.unique(equal)) == 1 and len(np.unique(mixed.mean(1))) == 2 and (mixed[:, :2] != mixed[:, 2:]).any()
