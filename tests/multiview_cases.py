"""The multi-view goldens (tests/golden/multiview_*.npz, scripts/make_golden_multiview.py): loader, the admission rules as
the tests apply them, a numpy restatement of every function, and the bounds.  A helper module, not a test.

Admission is decided by the script, from the reference alone, and stored in the files (admit_points / admit_che /
admit_flag); angles are compared for admitted points only, as angles where the reference's cosine is <= 1 - 1e-6 and as
cosines elsewhere (acos is ill-conditioned next to 1).  Deviations: points relative in the 2-norm, angles absolute in
degrees (radians for the angular error in radians), cosines absolute.

Bounds.  Measured on an MI355X over all goldens and all admitted entries (tests/test_gpu_multiview.py prints them):
    points   5.6e-11 relative (lr_lo50; 7e-13 at most outside the two local-refinement files)   -> POINT_TOL  1e-9
    angles   2.4e-11 degrees  (the table of behind_s6)                                            -> ANGLE_TOL  1e-9
    cosines  2.2e-16                                                                              -> COS_TOL    1e-14
each constant the smallest power of ten at least 10 x the measured value (room for another eigen-solver's rounding on
another box), none above 1e-9, the bound tests/test_gpu_pose_regimes.py uses for quantities of this kind.  The numpy
restatement below (LAPACK eigh, as the reference) deviates by 7.9e-11 / 7.3e-12 / 2.2e-16 and is held to the same
constants.  (The local-refinement scenes have baselines down to one degree; their admitted points move by up to 1e-10 under
the script's 1e-13 jitter, and two correct eigen-solvers differ there by 5e-11.)
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POINT_TOL, ANGLE_TOL, COS_TOL = 1e-9, 1e-9, 1e-14
CAP = 0.02
COS_SPLIT = 1.0 - 1e-6

TRI_CASES = ("bool_s8", "float_s8", "nomask_s6", "two_views", "many_s24", "behind_s6", "coincident_s5", "f32_s8")
LR_CASES = ("lr_lo1", "lr_lo50")
# entries of the "angles" golden whose point lies AT the first camera centre of the pair: `denominator <= eps`, angle 0
EPS_BRANCH = {"batched": (0, 2 * 6 + 3), "exhaustive": (4 * 7 + 1, 3), "pairs": (5, 0)}
ALL_FILES = TRI_CASES + LR_CASES + ("from_tracks", "angles", "angerr")


def load(name):
    with np.load(os.path.join(GOLDEN, f"multiview_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def files():
    return sorted(glob.glob(os.path.join(GOLDEN, "multiview_*.npz")))


# --- deviations ------------------------------------------------------------------------------------------------------
def point_deviation(got, ref, admit):
    """largest relative deviation (2-norm) over the admitted points; got / ref (...,3), admit (...)"""
    got, ref, admit = np.asarray(got).reshape(-1, 3), np.asarray(ref).reshape(-1, 3), np.asarray(admit).reshape(-1)
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert np.isfinite(rel[admit]).all()
    return float(rel[admit].max()) if admit.any() else 0.0


def angle_deviation(got, ref, admit=None, unit=np.pi / 180.0, ref_cos=None, got_cos=None):
    """(largest |angle difference| where the reference's cosine is <= 1 - 1e-6, largest |cosine difference| elsewhere) over
    the admitted entries.  `unit`: radians per unit of the angles; the cosines are taken from the angles unless given."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    admit = np.ones(ref.shape, bool) if admit is None else np.broadcast_to(admit, ref.shape)
    rc = np.cos(ref * unit) if ref_cos is None else ref_cos
    gc = np.cos(got * unit) if got_cos is None else got_cos
    as_angle = admit & (np.abs(rc) <= COS_SPLIT)
    as_cos = admit & ~as_angle
    assert np.isfinite(got[admit]).all()
    da = float(np.abs(got - ref)[as_angle].max()) if as_angle.any() else 0.0
    dc = float(np.abs(gc - rc)[as_cos].max()) if as_cos.any() else 0.0
    return da, dc


def assert_close(what, figures, report=print):
    """figures: {"points": x, "angles": y, "cosines": z} (any subset); prints each before asserting."""
    tol = {"points": POINT_TOL, "angles": ANGLE_TOL, "cosines": COS_TOL}
    report(f"[multiview] {what}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= tol[k], f"{what}: {k} deviate by {v:.3e} (bound {tol[k]:.0e})"


# --- numpy restatement -----------------------------------------------------------------------------------------------
def np_triangulate(cams, pts2, mask=None):
    """cams (B,S,3,4), pts2 (B,S,2), mask (B,S) -> points (B,3), invalid cheirality (B)"""
    cams, pts2 = np.asarray(cams, np.float64), np.asarray(pts2, np.float64)
    h = np.concatenate([pts2, np.ones(pts2.shape[:2] + (1,))], -1)
    r = h / np.linalg.norm(h, axis=-1, keepdims=True)
    terms = cams - r[..., :, None] * np.einsum("bsi,bsik->bsk", r, cams)[:, :, None, :]
    if mask is not None:
        terms = terms * np.asarray(mask, np.float64)[:, :, None, None]
    A = np.einsum("bsij,bsik->bjk", terms, terms)
    v = np.linalg.eigh(A)[1][:, :, 0]
    X = v[:, :3] / v[:, 3:]
    z = np.einsum("bsj,bj->bs", cams[:, :, 2, :3], X) + cams[:, :, 2, 3]
    return X, (z <= 0).any(1)


def np_centers(cams):
    return -np.einsum("...ji,...j->...i", cams[..., :3], cams[..., 3])


def _sq(d):
    return np.linalg.norm(d, axis=-1) ** 2


def np_angle_deg(r1, r2, bsq, eps=1e-12):
    den = 2.0 * np.sqrt(r1 * r2)
    nom = r1 + r2 - bsq
    bad = den <= eps
    c = np.clip(np.where(bad, 1.0, nom) / np.where(bad, 1.0, den), -1.0, 1.0)
    th = np.abs(np.arccos(c))
    return np.minimum(th, np.pi - th) * (180.0 / np.pi)


def np_angle_table(cams, X, eps=1e-12):
    """cams (B,S,3,4), X (B,3) -> (B,S*S)"""
    c = np_centers(np.asarray(cams, np.float64))
    B, S, _ = c.shape
    c1 = np.broadcast_to(c[:, :, None], (B, S, S, 3)).reshape(B, S * S, 3)
    c2 = np.broadcast_to(c[:, None], (B, S, S, 3)).reshape(B, S * S, 3)
    return np_angle_deg(_sq(X[:, None] - c1), _sq(X[:, None] - c2), _sq(c1 - c2), eps)


def np_angle_pairs(c1, c2, X, eps=1e-12):
    """c1, c2 (K,3), X (P,3) -> (K,P)"""
    return np_angle_deg(_sq(X[None] - c1[:, None]), _sq(X[None] - c2[:, None]), _sq(c1 - c2)[:, None], eps)


def np_angle_exhaustive(cams, X):
    c = np_centers(np.asarray(cams, np.float64))
    S = len(c)
    return np_angle_pairs(np.broadcast_to(c[:, None], (S, S, 3)).reshape(-1, 3), np.broadcast_to(c[None], (S, S, 3)).reshape(-1, 3), X)


def np_angular_error(p2, p3, cams, to_degree=False):
    """p2 (B,N,2), p3 (P,N,3), cams (B,3,4) -> angle (P,B,N), cos (P,B,N)"""
    r1 = np.concatenate([p2, np.ones(p2.shape[:2] + (1,))], -1)
    r1 = r1 / np.maximum(np.linalg.norm(r1, axis=-1, keepdims=True), 1e-12)
    r2 = np.einsum("bij,pnj->pbni", cams[:, :, :3], p3) + cams[None, :, None, :, 3]
    r2 = r2 / np.maximum(np.linalg.norm(r2, axis=-1, keepdims=True), 1e-12)
    c = np.clip((r1[None] * r2).sum(-1), -1.0, 1.0)
    a = np.arccos(c)
    return (a * (180.0 / np.pi) if to_degree else a), c


def np_local_refinement(points1, ext, thr, inl, order, lo):
    """-> points (B,lo,3), tri_angle_masks (B,lo), invalid cheirality (B,lo)"""
    B, N, _ = points1.shape
    lo_mask = inl[np.arange(B)[:, None], order[:, :lo]]                   # (B,lo,N)
    p = np.where(lo_mask[..., None], points1[:, None], 0.0).reshape(B * lo, N, 2)
    cams = np.repeat(ext, lo, axis=0)
    X, invalid = np_triangulate(cams, p, lo_mask.reshape(B * lo, N))
    flag = (np_angle_table(cams, X) >= thr).any(1)
    return X.reshape(B, lo, 3), flag.reshape(B, lo), invalid.reshape(B, lo)
