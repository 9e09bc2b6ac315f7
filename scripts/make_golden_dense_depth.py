"""Writes tests/golden/dense_depth_<case>.npz: the reference's dense-depth stage run on synthetic scenes.

Runs the reference's own ``VGGSfMRunner.extract_sparse_depth_and_point_from_reconstruction`` (vggsfm/runners/runner.py:
744-772) and ``align_dense_depth_maps`` (vggsfm/utils/utils.py:635-770, scikit-learn 1.7) through oracle.ref_harness on a
``pycolmap_compat.Reconstruction`` built from a ``vggsfm_amd.scene`` scene (cameras scaled to 64 px images so that the
dense clouds stay small).  Disparities are synthetic: a known affine function of the true inverse depth at the sparse
points' pixels, plus noise, a zero ("sky") band, gross outliers and a few huge values; some sparse points fall off the
maps.  scikit-learn's draws are recorded by wrapping ``sample_without_replacement`` under a fixed ``np.random.seed``, and a
seed is rejected if any point of an evaluated hypothesis lies within 1e-9 * threshold of the inlier threshold, so that
exact inlier-mask equality is well posed.  The colour half of the dense cloud is not stored: it is rgb / 255 over the
valid pixels, which the script asserts against the reference's output before writing.

Run where the reference tree exists:  python scripts/make_golden_dense_depth.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from vggsfm_amd import pycolmap_compat as pc  # noqa: E402
from vggsfm_amd.scene import make_scene  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SCALE = 16.0           # 1024 px scene images -> 64 px
IMAGE_PX = 64
WORLD_SCALE = 0.01

CASES = {
    # name: (S, N, camera, shared, inlier fraction, map sizes (H, W) per image or None, constant-map image or -1, empty image)
    "pinhole": (5, 400, "SIMPLE_PINHOLE", False, 0.7, None, -1, False),
    "radial_shared": (5, 400, "SIMPLE_RADIAL", True, 0.7, [(54, 60), (50, 66), (58, 58), (48, 62), (57, 53)], 3,
                      True),
    "low_inlier": (3, 600, "SIMPLE_PINHOLE", False, 0.15, None, -1, False),
}


def build_reconstruction(S, N, camera, shared, seed, empty_image):
    sc = make_scene(S, N, camera, shared_camera=shared, seed=seed, full_visibility=False)
    # world scaled by 1/100 (same images): inverse depths ~25 spread over ~13, so that the inlier band of the reference
    # (squared residual <= median / 30, i.e. |r| <~ 0.9) separates inliers from outliers
    sc.points3D *= WORLD_SCALE
    sc.extrinsics[:, :, 3] *= WORLD_SCALE
    rec = pc.Reconstruction.from_arrays(sc.points3D, sc.extrinsics, sc.intrinsics, sc.tracks, sc.mask,
                                        np.array([1024, 1024]), shared_camera=shared, camera_type=camera,
                                        extra_params=sc.extra_params)
    for c in rec.cameras.values():
        c._params[:3] /= SCALE
        c.width, c.height = IMAGE_PX, IMAGE_PX
    if empty_image:
        cam = next(iter(rec.cameras.values()))
        rec.add_image(pc.Image(S, f"image_{S}", cam.camera_id, rec.images[0].cam_from_world))
    return sc, rec


def make_maps(rec, sparse_depth, frac, sizes, const_img, rng):
    disp, rgb = {}, {}
    for k, name in enumerate(sparse_depth):
        H, W = sizes[k] if sizes else (56, 60)
        a, b = rng.uniform(0.5, 2.0), rng.uniform(-0.05, 0.05)
        d = rng.uniform(5.0, 40.0, size=(H, W)).astype(np.float32)
        uvd = np.array(sparse_depth[name])
        iu, iv = np.round(uvd[:, 0]).astype(int), np.round(uvd[:, 1]).astype(int)
        ok = (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
        inl = rng.uniform(size=len(uvd)) < frac
        val = np.where(inl, (1.0 / uvd[:, 2] - b) / a + rng.normal(0, 2e-4, len(uvd)), rng.uniform(0.0, 60.0, len(uvd)))
        d[iv[ok], iu[ok]] = val[ok].astype(np.float32)
        d[: H // 8] = 0.0                                      # sky
        d[H // 2, : W // 4] = 3e4                              # beyond 1e4 once rescaled
        d[H // 2 + 1, : W // 4] = -1.0                         # negative once rescaled
        if k == const_img:
            d[...] = 0.5
        disp[name] = d
        rgb[name] = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return disp, rgb


def run_case(name, seed):
    S, N, camera, shared, frac, sizes, const_img, empty = CASES[name]
    ref_harness.install()
    sys.modules["pycolmap"] = pc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import sklearn.linear_model._ransac as ransac_mod
        from vggsfm.runners import runner as R
        from vggsfm.utils import utils as U

    sc, rec = build_reconstruction(S, N, camera, shared, seed, empty)
    runner = object.__new__(R.VGGSfMRunner)
    pred = runner.extract_sparse_depth_and_point_from_reconstruction({"reconstruction": rec})
    sparse_depth, sparse_point = pred["sparse_depth"], pred["sparse_point"]
    rng = np.random.default_rng(seed)
    disp, rgb = make_maps(rec, sparse_depth, frac, sizes, const_img, rng)
    disp_in = {k: v.copy() for k, v in disp.items()}

    fits = []
    orig_sample, orig_fit = ransac_mod.sample_without_replacement, ransac_mod.RANSACRegressor.fit

    def sample(n, k, random_state=None):
        idx = orig_sample(n, k, random_state=random_state)
        fits[-1]["draws"].append(np.array(idx))
        return idx

    def fit(self, X, y, **kw):
        fits.append({"draws": [], "X": X.copy(), "y": np.array(y, copy=True), "thr": self.residual_threshold})
        out = orig_fit(self, X, y, **kw)
        fits[-1].update(n_trials=self.n_trials_, mask=self.inlier_mask_.copy(), coef=self.estimator_.coef_.copy(),
                        intercept=np.asarray(self.estimator_.intercept_))
        return out

    ransac_mod.sample_without_replacement, ransac_mod.RANSACRegressor.fit = sample, fit
    try:
        np.random.seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            depth_dict, cloud = U.align_dense_depth_maps(rec, sparse_depth, disp, rgb, visual_dense_point_cloud=True)
    finally:
        ransac_mod.sample_without_replacement, ransac_mod.RANSACRegressor.fit = orig_sample, orig_fit

    # well-posedness: no point of an evaluated hypothesis within 1e-9 * thr of the threshold
    from sklearn.linear_model import LinearRegression
    for f in fits:
        for idx in f["draws"]:
            m = LinearRegression().fit(f["X"][idx], f["y"][idx])
            r2 = (f["y"] - m.predict(f["X"])) ** 2
            if np.min(np.abs(r2 - f["thr"])) <= 1e-9 * f["thr"]:
                return None
    names = list(sparse_depth)
    out = dict(case=name, seed=seed, camera=camera, shared=shared, S=S, N=N, empty_image=empty, scale=SCALE,
               names=np.array(names), points3D=sc.points3D, extrinsics=sc.extrinsics, intrinsics=sc.intrinsics,
               tracks=sc.tracks, mask=sc.mask, extra_params=sc.extra_params if sc.extra_params is not None else np.zeros((0, 1)))
    for k, n in enumerate(names):
        f = fits[k]
        out.update({f"uvd_{k}": np.array(sparse_depth[n]), f"xyzid_{k}": np.array(sparse_point[n]),
                    f"disp_in_{k}": disp_in[n], f"rgb_{k}": rgb[n], f"draws_{k}": np.array(f["draws"], np.int32).reshape(-1, 2),
                    f"n_trials_{k}": f["n_trials"], f"inlier_mask_{k}": f["mask"], f"coef_{k}": f["coef"],
                    f"intercept_{k}": f["intercept"], f"thr_{k}": f["thr"], f"depth_{k}": depth_dict[n], f"disp_out_{k}": disp[n],
                    f"cloud_xyz_{k}": cloud[n][0]})
        # the cloud's colour half is rgb / 255 over the valid pixels (utils.py:755-758): checked here, not stored
        assert np.array_equal(cloud[n][1], (rgb[n] / 255.0).reshape(-1, 3)[(disp[n] != 0).reshape(-1)])
    out["coef_dtype"] = str(fits[0]["coef"].dtype)
    out["intercept_dtype"] = str(fits[0]["intercept"].dtype)
    out["disp_dtype"] = str(disp[names[0]].dtype)
    out["depth_dtype"] = str(depth_dict[names[0]].dtype)
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        for seed in range(1, 50):
            out = run_case(name, seed)
            if out is not None:
                break
        else:
            raise RuntimeError(f"{name}: no well-posed seed")
        path = os.path.join(OUT, f"dense_depth_{name}.npz")
        np.savez_compressed(path, **out)
        trials = [int(out[f"n_trials_{k}"]) for k in range(len(out["names"]))]
        print(f"{path}: seed {out['seed']}, n_trials {trials}, {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
