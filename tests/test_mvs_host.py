"""CPU tests of the multi-view stereo: what its C-ABI registry has of its own (the registry itself is
tests/test_side_libraries.py's), the yardstick of the GPU tests (the NumPy restatement of tests/mvs_cases.py) against
analytic truth, the margins of every decision the GPU tests compare exactly, the host bookkeeping of vggsfm_amd/mvs.py, and
the loud failure of the product module without the library.  No kernel is called here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import mvs_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_mvs
from vggsfm_amd import pycolmap_compat as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_table_and_library_agree():
    """What only the stereo has (tests/test_side_libraries.py compares table, header and symbols): prototypes pinned by
    hand, and the header's constants against the binding and the restatement."""
    header = open(_lib_mvs.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert functions["vggm_plane_sweep"][1][8:12] == ["pointer", "int", "double", "double"]
    assert functions["vggm_consistency_filter"][1][4:6] == ["pointer", "int"] and functions["vggm_build_arch"] == ("pointer", [])
    consts = dict(re.findall(r"#define VGGM_(\w+) (\d+)", header))
    assert [int(consts[k]) for k in ("MAX_SOURCES", "MAX_PLANES", "MAX_RADIUS")] == \
        [_lib_mvs.MAX_SOURCES, _lib_mvs.MAX_PLANES, _lib_mvs.MAX_RADIUS] == [C.MAX_SOURCES, 1024, 3]


def test_the_dense_stage_states_its_shared_code_once():
    """Over the sources and headers under csrc/, comments stripped: one definition of each helper the dense libraries share,
    and the cost nest (named by its zncc expression) in one file."""
    csrc = os.path.join(ROOT, "vggsfm_amd", "csrc")
    code = {}
    for folder, _, names in os.walk(csrc):
        for name in names:
            if name.endswith((".hip", ".hpp", ".h")):
                path = os.path.join(folder, name)
                code[os.path.relpath(path, csrc)] = re.sub(r"//[^\n]*", "", open(path).read())
    assert {"mvs/mvs.hip", "patchmatch/patchmatch.hip", "fuse/fuse.hip", "tsdf/tsdf.hip", "klt/klt.hip", "dense.hip"} <= set(code)
    for helper in ("relative_pose", "transfer_project", "inside_image", "bilinear", "clampi", "make_views", "block_scan_flag",
                   "block_scan_int"):
        # a definition: after a type, the name, its parameters, then the body (a call is followed by ; or an operator)
        definition = re.compile(r"[\w>*&]\s+" + helper + r"\s*\([^;{}]*\)\s*\{")
        where = [path for path, text in code.items() for _ in definition.findall(text)]
        assert len(where) == 1, (helper, where)
        uses = sum(len(re.findall(r"\b" + helper + r"(?:<\w+>)?\s*\(", text)) for text in code.values())
        assert uses >= 3, helper                                                    # the definition and at least two calls
    nest = [path for path, text in code.items() if re.search(r"zncc\s*=\s*den\s*>\s*0\.0\s*\?\s*tab\s*/\s*den", text)]
    assert nest == ["mvs/mvs_cost.hpp"], nest


def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch (sources and ray_index are host arrays): every
    out-of-range argument returns VGG_ERR_INVALID_ARGUMENT, an empty frame is a no-op."""
    import torch
    L = _lib_mvs.lib()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    good = dict(num_frames=3, height=4, width=5, ref=1, sources=i32(0, 2), num_sources=2, far=0.2, near=0.3, planes=8, radius=2,
                min_views=1)

    def sweep(**kw):
        a = dict(good, **kw)
        return L.vggm_plane_sweep(None, None, None, None, a["num_frames"], a["height"], a["width"], a["ref"], a["sources"],
                                  a["num_sources"], a["far"], a["near"], a["planes"], a["radius"], a["min_views"], 1e-5, 0.5,
                                  None, None, None, None, None)
    assert sweep(height=0) == 0 and sweep(width=0) == 0                    # a count of 0: a no-op
    assert sweep() == -1                                                    # NULL pointers with pixels to work on
    for bad in (dict(planes=0), dict(planes=1025), dict(radius=0), dict(radius=4), dict(num_sources=0), dict(min_views=0),
                dict(min_views=3), dict(ref=-1), dict(ref=3), dict(sources=i32(0, 3)), dict(sources=i32(-1, 2)),
                dict(sources=i32(1, 2)), dict(far=0.0), dict(far=-0.1), dict(far=0.3, near=0.2), dict(far=0.25, near=0.25),
                dict(near=float("inf")), dict(far=float("nan")), dict(height=-1), dict(num_frames=0),
                dict(sources=i32(*range(2, 11)), num_sources=9, num_frames=12)):
        assert sweep(**dict({"height": 0}, **bad)) == -1, bad

    def flt(**kw):
        a = dict(dict(good, ray_index=i32(0, 0, 0), num_rays=1, rel=0.01, reproj=1.0, min_consistent=1), **kw)
        return L.vggm_consistency_filter(None, None, None, None, a["ray_index"], a["num_rays"], a["num_frames"], a["height"],
                                         a["width"], a["ref"], a["sources"], a["num_sources"], a["rel"], a["reproj"],
                                         a["min_consistent"], None, None, None)
    assert flt(height=0) == 0 and flt() == -1
    for bad in (dict(min_consistent=0), dict(rel=-1.0), dict(reproj=float("nan")), dict(ray_index=i32(0, 1, 0)),
                dict(ray_index=i32(0, -1, 0)), dict(num_rays=0), dict(ref=3), dict(sources=i32(1, 0)), dict(num_sources=0)):
        assert flt(**dict({"height": 0}, **bad)) == -1, bad


def test_restatement_against_truth():
    """The yardstick itself, at 24 x 32, 3 views, 24 planes, radius 2, k = 0 and k = 0.08: median and 90th percentile of the
    inverse-depth error in plane spacings and the share of pixels without a depth, within 2 x the values measured when the
    test was written (mvs_cases.TRUTH_*: 0.3324 / 1.0457 spacings, none invalid; k = 0: 0.3311 / 1.0456, k = 0.08:
    0.3323 / 1.0003)."""
    cases, truth = C.sweep_cases()
    for name in truth:
        med, p90, valid = C.truth_errors(C.sweep_reference(name), truth[name])
        print(f"\n{name}: median {med:.4f}, 90th percentile {p90:.4f} plane spacings, valid {valid:.4f}")
        assert cases[name]["num_planes"] == 24 and cases[name]["radius"] == 2 and cases[name]["frames"].shape == (3, 24, 32)
        assert med <= 2 * C.TRUTH_MEDIAN and p90 <= 2 * C.TRUTH_P90 and 1.0 - valid <= 2 * C.TRUTH_INVALID
    assert {float(c["cams"][0, 3]) for n, c in cases.items() if n in truth} == {0.0, 0.08}


def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests exclude no pixel, so in every case they use: no two lowest costs of a pixel closer than 1e-9, no conf
    within 1e-9 of min_conf, no window variance within 1e-9 (relative) of min_variance, no parabola denominator within 1e-9
    of 0, no projection within 1e-9 of the image border or the camera plane where that decides; in the consistency cases no
    reprojection distance or relative depth difference within 1e-9 of its tolerance, no coordinate within 1e-9 of the
    rounding boundary of the nearest pixel."""
    for name in C.sweep_cases()[0]:
        m = C.sweep_reference(name)["margins"]
        print(name, {k: f"{v:.2e}" for k, v in m.items()})
        assert min(m.values()) > 1e-9, (name, m)
    for name in C.filter_cases():
        m = C.filter_reference(name)["margins"]
        print(name, {k: f"{v:.2e}" for k, v in m.items()})
        assert min(m.values()) > 1e-9, (name, m)
    spread = C.sweep_order_spread()
    print(f"order spread of the cost volume {spread:.3e}")
    assert 0 < spread < 1e-11


def test_cases_cover_what_the_kernel_can_get_wrong():
    cases, _ = C.sweep_cases()
    ref = {n: C.sweep_reference(n) for n in cases}
    assert {c["radius"] for c in cases.values()} == {1, 2, 3} and {1, 2, 3, 24} <= {c["num_planes"] for c in cases.values()}
    assert {len(c["sources"]) for c in cases.values()} >= {1, 2, 8} and {c["min_views"] for c in cases.values()} == {1, 2}
    assert {c["frames"].shape[1:] for c in cases.values()} == {(24, 32), (21, 35)} and any(c["ref"] != 0 for c in cases.values())
    assert cases["M8"]["frames"].shape[0] == 9
    for name in ("facing_away", "constant_reference"):
        assert (ref[name]["index"] == -1).all() and (ref[name]["depth"] == 0).all() and np.isinf(ref[name]["cost"]).all()
    wide = ref["wide_baseline"]["cost"]
    assert np.isinf(wide).any(axis=0).any() and np.isfinite(wide).any()      # part of the frame projects outside
    idx = ref["k08_24x32"]["index"]
    assert ((idx > 0) & (idx < 23)).any()                                    # the parabola is used
    assert (ref["D2"]["index"] == -1).any() and (ref["D2"]["index"] >= 0).any()      # min_conf cuts some pixels
    f = {n: C.filter_reference(n) for n in C.filter_cases()}
    assert (f["holes_mc2"]["count"] == 2).any() and (f["holes_mc2"]["count"] < 2).any()
    assert f["disagree_mc2"]["count"].max() == 1 and not f["disagree_mc2"]["depth"].any() and f["disagree_mc1"]["depth"].any()
    assert np.array_equal(f["two_ray_maps"]["count"], f["holes_mc2"]["count"])


# --------------------------------------------------------------------------------------------------- host bookkeeping
def _host():
    from vggsfm_amd import mvs
    return mvs.select_source_views, mvs.range_rule


def _reconstruction(centres, tracks, points):
    """images at `centres` (identity rotation), point p seen by the images of tracks[p]"""
    rec = P.Reconstruction()
    rec.add_camera(P.Camera("SIMPLE_PINHOLE", 64, 48, [50.0, 32.0, 24.0], 0))
    n = len(points)
    rec._reserve(n)
    rec._xyz[:n], rec._alive[:n], rec._n = np.asarray(points, float), True, n
    for i, c in enumerate(centres):
        pids = np.array([p + 1 for p in range(n) if i in tracks[p]], np.int64)
        img = P.Image(i, f"image_{i}", 0, P.Rigid3d(P.Rotation3d(np.eye(3)), -np.asarray(c, float)))
        img.points2D = P.ListPoint2D.from_arrays(np.zeros((len(pids), 2)), pids)
        img._registered = True
        rec.add_image(img)
    return rec


def test_select_source_views_counts_ties_and_the_angle_cut():
    select, _ = _host()
    centres = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0.001, 0, 0), (50, 0, 0)]
    points = [(0.5, 0.1 * p, 10.0) for p in range(6)]
    # image 0 shares 4 points with 1, 4 with 2 (a tie: the lower id first), 6 with 3 (too close: under the angle), none with 4
    tracks = [{0, 1, 2, 3}, {0, 1, 2, 3}, {0, 1, 2, 3}, {0, 1, 2, 3}, {0, 3}, {0, 3}]
    rec = _reconstruction(centres, tracks, points)
    got = select(rec, num_sources=4, min_angle_deg=2.0)
    assert got[0] == [1, 2] and got[1] == [0, 2, 3] and got[3] == [1, 2] and got[4] == []      # fewer candidates than asked
    assert select(rec, num_sources=1, min_angle_deg=2.0)[0] == [1]
    assert select(rec, num_sources=4, min_angle_deg=0.0)[0] == [3, 1, 2]                       # no cut: 6, 4, 4 points
    assert select(rec, num_sources=4, min_angle_deg=9.0)[0] == [2]                             # 0-1: 5.7 deg, 0-2: 11.4 deg
    rec.deregister_image(2)
    assert 2 not in select(rec)[0] and 2 not in select(rec)


def test_depth_range_rule():
    _, rule = _host()
    z = np.concatenate([np.linspace(2.0, 4.0, 101), [-1.0, 0.0, np.nan, np.inf]])
    near, far = rule(z, (5.0, 95.0), 1.25)
    assert near == pytest.approx(2.1 / 1.25) and far == pytest.approx(3.9 * 1.25)
    assert rule(z, (0.0, 100.0), 1.0) == (2.0, 4.0) and rule([3.0]) == (3.0 / 1.25, 3.0 * 1.25)
    for bad in (dict(depths=[-1.0, 0.0]), dict(depths=[1.0], widen=0.5), dict(depths=[1.0], percentiles=(60.0, 40.0))):
        with pytest.raises(ValueError):
            rule(**bad)


def test_import_without_the_library_fails_loudly(tmp_path):
    """A copy of the package without libvggsfm_amd_mvs.so: importing vggsfm_amd.mvs raises the error of _lib_mvs.lib(), naming
    the missing file and the build command; there is no fallback."""
    import shutil
    pkg = tmp_path / "vggsfm_amd"
    pkg.mkdir()
    src = os.path.join(ROOT, "vggsfm_amd")
    for name in ("_lib.py", "_lib_mvs.py", "mvs.py"):
        shutil.copy(os.path.join(src, name), pkg / name)
    (pkg / "__init__.py").write_text("")
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "try:\n    import vggsfm_amd.mvs\nexcept RuntimeError as e:\n    print('RuntimeError:', e)\nelse:\n    print('imported')\n")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("RuntimeError:") and "libvggsfm_amd_mvs.so is missing" in out.stdout \
        and "make -C vggsfm_amd/csrc/mvs" in out.stdout and "no CPU or eager fallback" in out.stdout, out.stdout
