"""GPU: the projection, filter and undistortion kernels (csrc/geometry.hip) on the cases of tests/geometry_cases.py, against the
long-double restatement recorded in tests/golden/geom_regimes_*.npz (the CPU half of the argument is
tests/test_geometry_cases.py).  Decisions -- masks, detail masks, iteration counts, the nan_to_num elements -- are compared
bit for bit wherever they are admitted; values are held to the bounds of geometry_cases.py, built from what float64 does
with the reference's own formulas.  Every test prints its figures before it asserts."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import geometry_cases as C
from tests.poison import equals_pattern, poisoned_allocations
from vggsfm_amd import _lib
from vggsfm_amd.utils import triangulation_helpers as H

pytestmark = pytest.mark.gpu
PATTERN = 0x7F
POISONED = ("pairs_s65_p65", "nonfinite_undistort")          # these two run on poisoned, guard-banded allocations


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def poisoned(name):
    return poisoned_allocations(PATTERN) if name in POISONED else contextlib.nullcontext()


def run_filter(job, points=slice(None), tracks=None):
    tracks = job["tracks"] if tracks is None else tracks
    m, d = H.filter_all_points3D(D(job["pts"][points]), D(tracks[:, points]), D(job["ext"]), D(job["K"]), D(job["extra"]),
                                 return_detail=True, **job["kw"])
    return m.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("name", C.FILTER_NAMES)
def test_filter_case(name):
    g = C.load(name)
    job = C.case_from_fixture(name, g)
    with poisoned(name):
        m, d = run_filter(job)
    am, ad = g["adm_mask"], g["adm_detail"]
    print(f"\n{name}: S {job['ext'].shape[0]} P {len(m)} {job['tracks'].dtype} tracks, {0 if job['extra'] is None else job['extra'].shape[1]} "
          f"distortion parameters | admitted masks {am.mean():.4f} details {ad.mean():.4f} | dev64 err {g['figures'][0]:.2e} cz "
          f"{g['figures'][1]:.2e} angle {g['figures'][2]:.2e} | accepted {int(m.sum())} (long double {int(g['ld_mask'].sum())}) | bits differing "
          f"on admitted: mask {int((m != g['ld_mask'])[am].sum())} detail {int((d != g['ld_detail'])[ad].sum())}, on the rest: "
          f"{int((m != g['ld_mask'])[~am].sum())} {int((d != g['ld_detail'])[~ad].sum())}")
    assert np.array_equal(m[am], g["ld_mask"][am]) and np.array_equal(d[ad], g["ld_detail"][ad])
    if job["tracks"].dtype == np.float32:                 # float64 tracks holding the float32 numbers: the float32 result
        m64, d64 = run_filter(job, tracks=job["tracks"].astype(np.float64))
        assert np.array_equal(m64, m) and np.array_equal(d64, d)


def test_filter_limits():
    """S = 4097 is refused and nothing is written; P = 0 returns empty results."""
    L = _lib.lib()
    S, P = C.MAX_FRAMES + 1, 2
    dev = torch.device("cuda")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    mask = torch.full((P,), PATTERN, dtype=torch.uint8, device=dev)
    detail = torch.full((S, P), PATTERN, dtype=torch.uint8, device=dev)
    ws = torch.full((L.vgg_filter_points_workspace_bytes(S),), PATTERN, dtype=torch.uint8, device=dev)
    rc = L.vgg_filter_points(z(P, 3), P, torch.zeros((S, P, 2), dtype=torch.float32, device=dev), 0, z(S, 3, 4), z(S, 3, 3), None, 0, S,
                             4.0, 1.5, 1, 300.0, 1e6, mask, detail, ws, _lib.stream_ptr())
    torch.cuda.synchronize()
    untouched = bool((mask == PATTERN).all()) and bool((detail == PATTERN).all()) and bool((ws == PATTERN).all())
    print(f"\nS = {S}: return code {rc}, outputs and workspace untouched: {untouched}")
    assert rc == -1 and untouched
    with pytest.raises(RuntimeError):
        H.filter_all_points3D(z(P, 3), torch.zeros((S, P, 2), dtype=torch.float32, device=dev), z(S, 3, 4), z(S, 3, 3))
    for chk in (False, True):
        m, d = H.filter_all_points3D(z(0, 3), torch.zeros((5, 0, 2), dtype=torch.float64, device=dev), z(5, 3, 4), z(5, 3, 3),
                                     check_triangle=chk, return_detail=True)
        assert m.shape == (0,) and d.shape == (5, 0)


@pytest.mark.parametrize("name", ["pairs_s65_p65", "pairs_s129_p130", "pairs_s4_p65", "loop", "nonfinite_f32"])
def test_filter_does_not_depend_on_the_other_points(name):
    """The result of a point does not depend on which points share its call: a permutation, and the call split in two."""
    job = C.case_from_fixture(name)
    P = len(job["pts"])
    m, d = run_filter(job)
    perm = np.random.default_rng(7).permutation(P)
    mp, dp = run_filter(job, perm)
    cut = P // 2 + 1
    parts = [run_filter(job, slice(0, cut)), run_filter(job, slice(cut, P))]
    ms, ds = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts], 1)
    same = [np.array_equal(mp, m[perm]), np.array_equal(dp, d[:, perm]), np.array_equal(ms, m), np.array_equal(ds, d)]
    print(f"\n{name}: P {P}: permuted mask / detail, split mask / detail identical: {same}")
    assert all(same)


@pytest.mark.parametrize("name", C.PROJECT_NAMES)
def test_project_case(name):
    g = C.load(name)
    job = C.case_from_fixture(name, g)
    P = C.PROJECT_STRIDE_P if name == "project_stride" else len(job["pts"])        # the distinct points, tiled to the launch size
    pts = C.tile(job["pts"], P, axis=0)
    with poisoned(name):
        px, pc = H.project_3D_points(D(pts), D(job["ext"]), D(job["K"]), D(job["extra"]), return_points_cam=True)
        only = H.project_3D_points(D(pts), D(job["ext"]), only_points_cam=True)
        same_cam = torch.equal(only.view(torch.int64), pc.view(torch.int64))
        px, pc = px.cpu().numpy(), pc.cpu().numpy()
    ld_px, ld_pc, cls, adm = (C.tile(g[k], P, axis=a) for k, a in (("ld_px", 1), ("ld_pc", 2), ("cls", 1), ("adm", 1)))
    fin = adm & (cls == 0)
    ex_px, b_px = C.value_excess(px, ld_px, g["figures"][0], fin)
    ex_pc, b_pc = C.value_excess(pc, ld_pc, g["figures"][1], np.isfinite(ld_pc))
    special = adm & (cls != 0)
    print(f"\n{name}: S {len(job['ext'])} P {P} | classes finite / NaN / +max / -max {np.bincount(cls.ravel(), minlength=4)} admitted {adm.mean():.4f} "
          f"| pixel deviation {ex_px:.3e} (bound {b_px:.3e}, dev64 {g['figures'][0]:.2e}) | camera deviation {ex_pc:.3e} (bound {b_pc:.3e}) | "
          f"nan_to_num elements differing {int((px != ld_px)[special].sum())} of {int(special.sum())} | only_points_cam identical {same_cam}")
    assert px.shape == (len(job["ext"]), P, 2) and pc.shape == (len(job["ext"]), 3, P) and same_cam
    assert np.array_equal(px[special], ld_px[special])
    assert ex_px <= b_px and ex_pc <= b_pc


def cam_from_img_abi(tracks, K, extra, max_iterations):
    """vgg_cam_from_img as the header declares it -> (normalised tracks, iterations_run)."""
    L = _lib.lib()
    S, P = tracks.shape[:2]
    k = 0 if extra is None else extra.shape[1]
    out = torch.empty((S, P, 2), dtype=torch.float64, device="cuda")
    ws = torch.empty(L.vgg_cam_from_img_workspace_bytes(S, P, max_iterations), dtype=torch.uint8, device="cuda") if k else None
    iters = ctypes.c_int(-1)
    rc = L.vgg_cam_from_img(D(tracks), int(tracks.dtype == np.float64), D(K), D(extra), k, S, P, out, max_iterations, 1e-10, 1e-6,
                            C.EPS64, ws, ctypes.byref(iters), _lib.stream_ptr())
    assert rc == 0
    return out, iters.value


@pytest.mark.parametrize("name", C.UNDISTORT_NAMES)
def test_undistort_case(name):
    g = C.load(name)
    job = C.case_from_fixture(name, g)
    P = {"undistort_stride": C.UNDISTORT_STRIDE_P, "normalise_stride": C.NORMALISE_STRIDE_P}.get(name, job["tracks"].shape[1])
    tracks = C.tile(job["tracks"], P)                        # (the grid-stride cases: the distinct tracks, tiled to the launch size)
    f64 = C._undistort(job, np.float64)                      # the float64 evaluation, deciding for itself
    f64 = C.tile(np.stack([f64["u"], f64["v"]], -1), P)
    with poisoned(name):
        out, iters = cam_from_img_abi(tracks, job["K"], job["extra"], job["max_iterations"])
        wrapped = H.cam_from_img(D(tracks), D(job["K"]), D(job["extra"])) if job["max_iterations"] == 100 else out
        same = torch.equal(wrapped.view(torch.int64), out.view(torch.int64))
        if tracks.dtype == np.float32:                       # float64 tracks holding the float32 numbers: the float32 result
            out64, iters64 = cam_from_img_abi(tracks.astype(np.float64), job["K"], job["extra"], job["max_iterations"])
            same = same and iters64 == iters and torch.equal(out64.view(torch.int64), out.view(torch.int64))
        out = out.cpu().numpy()
    ld, adm_elem = C.tile(g["ld_values"], P), C.tile(g["adm_elem"], P)
    adm = adm_elem[..., None] & np.isfinite(ld) & bool(g["adm_count"])
    ex, bound = C.value_excess(out, ld, g["figures"][0], adm)
    with np.errstate(all="ignore"):
        oracle_ok = np.abs(out - f64) <= C.ORACLE_ATOL + C.ORACLE_RTOL * np.abs(f64)
    print(f"\n{name}: S {tracks.shape[0]} P {P} {tracks.dtype} | iterations_run {iters} (long double {int(g['ld_iters'])}, admitted "
          f"{bool(g['adm_count'])}) | elements admitted {adm_elem.mean():.4f}, swaps in step 1 {int(g['swaps'][0])} | deviation {ex:.3e} (bound "
          f"{bound:.3e}, dev64 {g['figures'][0]:.2e}) | beyond rtol {C.ORACLE_RTOL:g} of the float64 evaluation: {int((~oracle_ok)[adm].sum())} | "
          f"non-finite {int((~np.isfinite(out)).sum())} (long double {int((~np.isfinite(ld)).sum())}) | wrapper and float64-track call identical {same}")
    assert not equals_pattern(out, PATTERN).any() and same
    assert bool(g["adm_count"]) and iters == int(g["ld_iters"])
    assert np.array_equal(np.isfinite(out), np.isfinite(ld))                      # NaN and inf stay in their element
    assert ex <= bound
    assert oracle_ok[adm].all()
