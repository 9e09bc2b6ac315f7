"""CPU tests of the depth-map fusion: what its C-ABI registry has of its own (the registry itself is
tests/test_side_libraries.py's), what the entries refuse, the yardstick of the GPU tests (the NumPy restatement of
tests/fusion_cases.py) against analytic truth, the de-duplication as a condition, the margins of every decision the GPU tests
compare exactly, the PLY round trip, and the loud failure of the product module without the library.  No kernel is called
here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_fuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vggf_build_arch", "vggf_depth_normals", "vggf_fuse_view"]


def test_header_table_and_library_agree():
    """What only the fusion has (tests/test_side_libraries.py compares table, header and symbols): the names and prototypes
    pinned by hand, and the header's constant against the binding and the restatement."""
    header = open(_lib_fuse.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert list(_lib_fuse.SIGNATURES) == list(functions) == NAMES
    assert functions["vggf_build_arch"] == ("pointer", [])
    assert functions["vggf_depth_normals"][1] == ["pointer"] * 4 + ["int"] * 4 + ["double", "pointer", "pointer"]
    assert functions["vggf_fuse_view"][1][7:18] == ["int"] * 5 + ["pointer", "int", "double", "double", "double", "int"]
    assert functions["vggf_fuse_view"][1][26] == "long" and len(functions["vggf_fuse_view"][1]) == 34
    consts = dict(re.findall(r"#define VGGF_(\w+) (\d+)", header))
    assert int(consts["MAX_SOURCES"]) == _lib_fuse.MAX_SOURCES == C.MAX_SOURCES         # (and the stereo's: test_side_libraries.py)


def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch (sources and ray_index are host arrays): every
    out-of-range argument returns VGG_ERR_INVALID_ARGUMENT, an empty frame is a no-op."""
    import torch
    L = _lib_fuse.lib()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    good = dict(num_frames=3, height=4, width=5, view=1, sources=i32(0, 2), num_sources=2, ray_index=i32(0, 0, 0), num_rays=1,
                rel=0.01, reproj=1.0, cos=0.8, min_views=2, jump=0.05, capacity=10)

    def normals(**kw):
        a = dict(good, **kw)
        return L.vggf_depth_normals(None, None, None, a["ray_index"], a["num_rays"], a["num_frames"], a["height"], a["width"],
                                    a["jump"], None, None)
    assert normals(height=0) == 0 and normals(width=0) == 0                # a frame of 0 pixels: a no-op
    assert normals() == -1                                                  # NULL pointers with pixels to work on
    for bad in (dict(jump=-0.1), dict(jump=float("nan")), dict(ray_index=i32(0, 1, 0)), dict(ray_index=i32(0, -1, 0)),
                dict(num_rays=0), dict(num_frames=0), dict(height=-1), dict(ray_index=None)):
        assert normals(**dict({"height": 0}, **bad)) == -1, bad

    def fuse(**kw):
        a = dict(good, **kw)
        return L.vggf_fuse_view(None, None, None, None, None, None, a["ray_index"], a["num_rays"], a["num_frames"], a["height"],
                                a["width"], a["view"], a["sources"], a["num_sources"], a["rel"], a["reproj"], a["cos"],
                                a["min_views"], None, None, None, None, None, None, None, None, a["capacity"], None, None, None,
                                None, None, None, None)
    assert fuse(height=0) == 0 and fuse(width=0) == 0 and fuse() == -1
    assert fuse(height=0, sources=None, num_sources=0, min_views=1) == 0    # zero sources are legal
    assert fuse(height=0, min_views=1) == 0 and fuse(height=0, min_views=3) == 0
    for bad in (dict(view=-1), dict(view=3), dict(sources=i32(0, 3)), dict(sources=i32(-1, 2)), dict(sources=i32(1, 2)),
                dict(sources=i32(*range(2, 11)), num_sources=9, num_frames=12), dict(num_sources=-1), dict(min_views=0),
                dict(min_views=4), dict(sources=None, num_sources=0, min_views=2), dict(rel=-0.01), dict(rel=float("nan")),
                dict(reproj=-1.0), dict(reproj=float("nan")), dict(cos=float("nan")), dict(ray_index=i32(0, 1, 0)),
                dict(ray_index=i32(0, 0, -1)), dict(num_rays=0), dict(num_frames=0), dict(height=-1), dict(capacity=-1),
                dict(sources=None)):
        assert fuse(**dict({"height": 0}, **bad)) == -1, bad


def test_python_side_raises_without_a_device():
    """The checks of vggsfm_amd.fusion that come before any device work raise on host tensors too."""
    import torch
    from vggsfm_amd import fusion
    sc = C.scenes()["k08"]
    depth = torch.from_numpy(sc["truth"].astype(np.float32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.depth_normals(depth, sc["poses"], sc["cams"], rays=torch.from_numpy(sc["rays"]), ray_index=sc["ray_index"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.fuse_depth_maps(depth, sc["poses"], sc["cams"], C.others(3))
    with pytest.raises(ValueError):
        fusion.depth_normals(depth.double(), sc["poses"], sc["cams"])
    with pytest.raises(ValueError):
        fusion.depth_normals(depth[0], sc["poses"], sc["cams"])


def test_restatement_against_truth():
    """The yardstick itself on the true depth maps rounded to float32, 3 and 9 views of 24 x 32, k = 0 and k = 0.08, every
    other view a source, tolerances 1 % and 1 px, 30 degrees, jump 0.05: the largest distance of a fused point from the
    plane and the largest angle of a depth normal against the plane's, within 2 x the values measured when the test was
    written (fusion_cases.TRUTH_*: 2.3696e-7 and 2.8715e-4 degrees); every pixel has a normal; the counts are the ones measured
    then (3 views at min_views 1 / 2 / 3: 948 / 844 / 808 at k = 0; 9 views at min_views 2: 1067)."""
    cases = C.fusion_cases()
    worst_d = worst_a = 0.0
    for name in C.TRUTH_CASES:
        case, ref = cases[name], C.fusion_reference(name)
        assert case["depth"].shape[1:] == (24, 32) and case["sources"] == C.others(len(case["depth"]))
        dist = float(C.plane_distance(ref["xyz"]).max())
        angle = C.normal_angle_deg(case["normals"])
        fused = C.normal_angle_deg(ref["normal"])
        print(f"\n{name}: {len(ref['xyz'])} points of {case['depth'].size} pixels, per view {ref['counts']}, seeds "
              f"{ref['seeds']}; distance {dist:.4e}; depth normals {np.nanmax(angle):.4e} deg, fused {np.nanmax(fused):.4e} deg")
        assert not np.isnan(angle).any() and not np.isnan(fused).any()       # every pixel and every point has a normal
        assert dist <= 2 * C.TRUTH_PLANE_DISTANCE
        assert np.nanmax(angle) <= 2 * C.TRUTH_NORMAL_ANGLE_DEG and np.nanmax(fused) <= 2 * C.TRUTH_NORMAL_ANGLE_DEG
        worst_d, worst_a = max(worst_d, dist), max(worst_a, float(np.nanmax(angle)))
    print(f"worst distance {worst_d:.4e}, worst normal angle {worst_a:.4e} deg")
    assert worst_d > 0.5 * C.TRUTH_PLANE_DISTANCE and worst_a > 0.5 * C.TRUTH_NORMAL_ANGLE_DEG    # the constants are not slack
    assert [len(C.fusion_reference(n)["xyz"]) for n in ("k0_mv1", "k0_mv2", "k0_mv3", "nine_views")] == [948, 844, 808, 1067]
    assert C.fusion_reference("k0_mv1")["seeds"] == [768, 66, 114]
    assert {float(cases[n]["cams"][0, 3]) for n in C.TRUTH_CASES} == {0.0, 0.08}


def test_fusion_removes_the_duplicates():
    """A condition, not a measurement: on the true maps the fused cloud has at most half as many points as there are pixels
    with depth, and at 3 views the views after the first seed fewer than a quarter of their pixels (measured: 0.41 and at
    most 0.15)."""
    for name in C.TRUTH_CASES:
        case, ref = C.fusion_cases()[name], C.fusion_reference(name)
        with_depth = int((case["depth"] > 0).sum())
        later = max(ref["seeds"][1:]) / case["depth"][0].size
        print(f"\n{name}: {len(ref['xyz'])} points / {with_depth} pixels with depth = {len(ref['xyz']) / with_depth:.3f}; "
              f"largest share of seeds after the first view {later:.3f}")
        assert len(ref["xyz"]) <= 0.5 * with_depth
        if len(case["depth"]) == 3:
            assert later < 0.25


def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests compare bits and exclude no pixel, so in every case they use no decision is closer than 1e-9 to its
    threshold: both tolerance tests, the rounding to the nearest pixel, the camera plane of both transfers, the normal's
    cosine against its limit, the jump test, n . P against 0 and |n| against 0."""
    for name in C.normals_cases():
        m = C.normals_reference(name)["margins"]
        print(name, {k: f"{v:.2e}" for k, v in m.items()})
        assert min(m.values()) > 1e-9, (name, m)
    for name, case in C.fusion_cases().items():
        m = C.fusion_reference(name)["margins"]
        print(name, {k: f"{v:.2e}" for k, v in m.items()})
        assert min(m.values()) > 1e-9, (name, m)
        if case["normals"] is not None:                                     # the normal maps the cases fuse with
            nm = C.depth_normals(case["depth"], case["poses"], case["rays"], case["ray_index"])["margins"]
            assert min(nm.values()) > 1e-9, (name, nm)


def test_cases_cover_what_the_kernel_can_get_wrong():
    ncases, fcases = C.normals_cases(), C.fusion_cases()
    nref = {n: C.normals_reference(n)["normals"] for n in ncases}
    assert {c["depth"].shape[1:] for c in ncases.values()} == {(24, 32), (21, 35)}       # 21 x 35: no multiple of the tile
    assert C.scenes()["k0"]["cams"][0, 3] == 0.0 and C.scenes()["k08"]["cams"][0, 3] == 0.08      # both camera models
    for name in ("k0_24x32", "k08_24x32", "k08_21x35", "depth_step"):
        assert C._nonzero(nref[name]).all(), name
    holes, none = ncases["holes"]["depth"], ~C._nonzero(nref["holes"])
    assert (none & (holes > 0)).any() and (none == (holes == 0))[holes == 0].all()       # isolated pixels and the holes
    # one-sided differences: pixels with a normal and a hole beside them
    beside = np.zeros_like(holes, bool)
    beside[:, :, 1:] |= holes[:, :, :-1] == 0
    assert (beside & ~none).any()
    # the jump cuts: across the step the normals are still the plane's (one-sided), not the step's
    assert np.nanmax(C.normal_angle_deg(nref["depth_step"])) < 1e-3
    assert np.array_equal(nref["two_ray_maps"], nref["holes"]) and len(ncases["two_ray_maps"]["rays"]) == 2
    f = {n: C.fusion_reference(n) for n in fcases}
    assert {c["min_views"] for c in fcases.values()} == {1, 2, 3}
    assert {len(c["sources"][0]) for c in fcases.values()} == {0, 2, 8} and len(fcases["nine_views"]["depth"]) == 9
    assert {c["depth"].shape[1:] for c in fcases.values()} == {(24, 32), (21, 35)}
    assert all(c["depth"][0].size > 256 and c["depth"][0].size % 256 for c in fcases.values() if c["depth"].shape[1] == 21)
    assert len(f["k0_mv1"]["xyz"]) > len(f["k0_mv2"]["xyz"]) > len(f["k0_mv3"]["xyz"]) > 0
    assert set(f["nine_views"]["num_views"]) >= {2, 9}
    assert (fcases["holes"]["depth"] == 0).any() and (~C._nonzero(fcases["holes"]["normals"])).any()
    # view 2 is 6 % off: it supports nothing, seeds its own points at min_views 1 and gives none at 2
    assert f["off_mv1"]["num_views"].max() == 2 and f["off_mv1"]["counts"][2] == f["off_mv1"]["seeds"][2] > 0
    assert f["off_mv2"]["counts"][2] == 0 and not f["off_mv2"]["claimed"][2].any() and f["off_mv2"]["counts"][0] > 0
    # the tilted normal map: sources pass the geometric test and fail the normal test
    assert f["tilted_normals"]["rejected_by_normal"] > 0 and f["k08_mv2"]["rejected_by_normal"] == 0
    assert f["tilted_normals"]["counts"][1] == 0 and not f["tilted_normals"]["claimed"][1].any()
    assert fcases["no_normals"]["normals"] is None and not f["no_normals"]["normal"].any()
    assert fcases["no_colors"]["colors"] is None and not f["no_colors"]["rgb"].any() and f["k08_mv2"]["rgb"].any()
    for k in ("xyz", "num_views", "view", "pixel"):
        assert np.array_equal(f["no_normals"][k], f["k08_mv2"][k]) and np.array_equal(f["no_colors"][k], f["k08_mv2"][k])
    zero = f["zero_sources"]
    assert (zero["num_views"] == 1).all() and len(zero["xyz"]) == int((fcases["zero_sources"]["depth"] > 0).sum())
    away = f["facing_away"]
    assert away["counts"][2] == 0 and not away["claimed"][2].any() and away["num_views"].max() == 2
    copy = f["copy_of_view0"]
    assert copy["claimed"][1].all() and copy["counts"][1] == 0 and copy["seeds"][1] == 0 and copy["counts"][0] == 768
    a, b = f["order_201"], f["order_012"]
    assert list(a["view"][[0, -1]]) == [2, 1] and list(b["view"][[0, -1]]) == [0, 2] and len(a["xyz"]) != len(b["xyz"])
    assert not np.array_equal(a["claimed"], b["claimed"])
    assert len(f["all_zero"]["xyz"]) == 0 and f["all_zero"]["xyz"].shape == (0, 3)
    # the order: views as fused, row-major inside a view
    for name, ref in f.items():
        order = fcases[name]["view_order"]
        key = np.array([order.index(v) for v in ref["view"]], np.int64) * 10 ** 6 + ref["pixel"]
        assert (np.diff(key) > 0).all(), name


def test_ply_round_trip(tmp_path):
    """write_ply then read_ply: positions, normals and counts come back bit for bit, colours (clipped to [0, 1]) to the uchar rounding; a cloud
    of 0 points round-trips; the header is the one the issue names."""
    from vggsfm_amd import fusion
    ref = C.fusion_reference("k08_mv2")
    cloud = fusion.FusedCloud(*(ref[k] for k in fusion.FusedCloud._fields))
    path = str(tmp_path / "cloud.ply")
    fusion.write_ply(path, cloud)
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(ref['xyz'])}"]
    assert head[3:-1] == ["property double x", "property double y", "property double z", "property float nx",
                          "property float ny", "property float nz", "property uchar red", "property uchar green",
                          "property uchar blue", "property int num_views"]
    assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + 43 * len(ref["xyz"])
    back = fusion.read_ply(path)
    assert back.xyz.dtype == np.float64 and back.xyz.tobytes() == ref["xyz"].tobytes()
    assert back.normal.dtype == np.float32 and back.normal.tobytes() == ref["normal"].tobytes()
    assert np.array_equal(back.num_views, ref["num_views"]) and back.num_views.dtype == np.int32
    assert back.rgb.dtype == np.float32 and np.abs(back.rgb.astype(np.float64) - np.clip(ref["rgb"], 0, 1)).max() <= 0.5 / 255 + 1e-7
    assert (back.view == -1).all() and (back.pixel == -1).all()
    empty = C.fusion_reference("all_zero")
    fusion.write_ply(path, fusion.FusedCloud(*(empty[k] for k in fusion.FusedCloud._fields)))
    back = fusion.read_ply(path)
    assert back.xyz.shape == back.normal.shape == back.rgb.shape == (0, 3) and back.num_views.shape == (0,)
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        fusion.read_ply(path)


def test_import_without_the_library_fails_loudly(tmp_path):
    """A copy of the package without libvggsfm_amd_fuse.so: importing vggsfm_amd.fusion raises the error of _lib_fuse.lib(),
    naming the missing file and the build command; there is no fallback."""
    import shutil
    pkg = tmp_path / "vggsfm_amd"
    pkg.mkdir()
    src = os.path.join(ROOT, "vggsfm_amd")
    for name in ("_lib.py", "_lib_fuse.py", "fusion.py"):
        shutil.copy(os.path.join(src, name), pkg / name)
    (pkg / "__init__.py").write_text("")
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "try:\n    import vggsfm_amd.fusion\nexcept RuntimeError as e:\n    print('RuntimeError:', e)\nelse:\n    print('imported')\n")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("RuntimeError:") and "libvggsfm_amd_fuse.so is missing" in out.stdout \
        and "make -C vggsfm_amd/csrc/fuse" in out.stdout and "no CPU or eager fallback" in out.stdout, out.stdout
