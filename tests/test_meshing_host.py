"""CPU tests of the meshing: what its C-ABI registry has of its own (the registry itself is tests/test_side_libraries.py's),
what the entries refuse, the kernel's written-out case table against the one derived from the header's rule, the yardstick
of the GPU tests (the NumPy restatement of tests/meshing_cases.py) on closed surfaces, on a volume with holes and against
analytic truth, the margins of every decision the GPU tests compare exactly, and the PLY round-trip.  No kernel is called
here."""
import re

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import meshing_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_tsdf

NAMES = ["vggv_build_arch", "vggv_case_table", "vggv_integrate", "vggv_mesh_count", "vggv_mesh_emit"]


# --------------------------------------------------------------------------------------------------- registry
def test_header_table_and_library_agree():
    """What only the meshing has (tests/test_side_libraries.py compares table, header and symbols): the names and prototypes
    pinned by hand, and the header's constants against the binding and the restatement."""
    header = open(_lib_tsdf.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert list(_lib_tsdf.SIGNATURES) == list(functions) == NAMES
    assert functions["vggv_build_arch"] == ("pointer", [])
    assert functions["vggv_case_table"] == ("int", ["pointer"])
    assert functions["vggv_integrate"][1] == ["pointer"] * 5 + ["int"] * 3 + ["double"] * 4 + ["int"] * 3 + ["double"] + ["pointer"] * 4
    assert functions["vggv_mesh_count"][1] == ["pointer"] * 2 + ["int"] * 3 + ["double"] + ["pointer"] * 7
    assert functions["vggv_mesh_emit"][1] == ["pointer"] * 3 + ["double"] * 4 + ["int"] * 3 + ["double"] + ["pointer"] * 4 + \
        ["long"] * 2 + ["pointer"] * 5
    consts = dict(re.findall(r"#define VGGV_(\w+) (\d+)", header))
    assert [int(consts[k]) for k in ("GROUP", "MAX_VIEWS")] == [_lib_tsdf.GROUP, _lib_tsdf.MAX_VIEWS] == [C.GROUP, 256]
    assert _lib_tsdf.MAX_NODES == (2 ** 31 - 1) // 7


# --------------------------------------------------------------------------------------------------- refusals
def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch: every out-of-range argument returns
    VGG_ERR_INVALID_ARGUMENT (a grid of more than (2^31 - 1) / 7 nodes VGG_ERR_UNSUPPORTED), a grid of 0 nodes and a frame
    of 0 pixels are no-ops, and Python refuses the same arguments first."""
    L = _lib_tsdf.lib()
    nan, inf = float("nan"), float("inf")
    good = dict(num_frames=3, height=4, width=5, voxel=0.1, dims=(3, 4, 5), trunc=0.4, min_weight=1.0, vcap=0, fcap=0)

    def integrate(**kw):
        a = dict(good, **kw)
        return L.vggv_integrate(None, None, None, None, None, a["num_frames"], a["height"], a["width"], 0.0, 0.0, 0.0, a["voxel"],
                                *a["dims"], a["trunc"], None, None, None, None)

    def count(**kw):
        a = dict(good, **kw)
        return L.vggv_mesh_count(None, None, *a["dims"], a["min_weight"], None, None, None, None, None, None, None)

    def emit(**kw):
        a = dict(good, **kw)
        return L.vggv_mesh_emit(None, None, None, 0.0, 0.0, 0.0, a["voxel"], *a["dims"], a["min_weight"], None, None, None, None,
                                a["vcap"], a["fcap"], None, None, None, None, None)
    grids = (dict(dims=(1, 4, 5)), dict(dims=(3, 1, 5)), dict(dims=(3, 4, 1)), dict(dims=(-1, 4, 5)), dict(dims=(3, 4, -2)),
             dict(dims=(0, 1, 5)), dict(dims=(0, 4, -1)))
    voxel = (dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan))
    weight = (dict(min_weight=0.0), dict(min_weight=-1.0), dict(min_weight=nan))
    for entry, refused in ((integrate, grids + voxel + (dict(trunc=0.0), dict(trunc=-0.2), dict(trunc=nan), dict(num_frames=0),
                                                       dict(height=-1), dict(width=-1))),
                           (count, grids + weight), (emit, grids + voxel + weight + (dict(vcap=-1), dict(fcap=-1)))):
        assert entry() == -1, entry.__name__                                      # NULL pointers with nodes to work on
        for empty in ((0, 4, 5), (3, 0, 5), (3, 4, 0), (0, 0, 0)):                # a grid of 0 nodes: a no-op
            assert entry(dims=empty) == 0, (entry.__name__, empty)
        for bad in refused:
            assert entry(**dict({} if "dims" in bad else {"dims": (0, 4, 5)}, **bad)) == -1, (entry.__name__, bad)
        for big in ((1024, 1024, 293), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (46341, 46341, 2)):
            assert entry(dims=big) == -4, (entry.__name__, big)
    assert integrate(height=0) == 0 and integrate(width=0) == 0                   # a frame of 0 pixels: a no-op
    assert integrate(height=0, trunc=0.0) == -1 and integrate(dims=(0, 4, 5), trunc=inf) == 0
    assert count(dims=(674, 674, 675), min_weight=inf) == -1                      # 306 653 700 nodes fit: NULL pointers refuse
    assert L.vggv_case_table(None) == -1
    with pytest.raises(Exception):
        emit(vcap=2 ** 63)                                                        # the binding refuses what does not fit

    from vggsfm_amd import meshing
    for bad in ((1, 4, 5), (3, 4), (3, 4, 0), (1024, 1024, 293)):
        with pytest.raises(ValueError, match="dims|too large"):
            meshing.TSDFVolume((0, 0, 0), 0.1, bad)
    for bad in (0.0, -1.0, nan):
        with pytest.raises(ValueError, match="voxel"):
            meshing.TSDFVolume((0, 0, 0), bad, (3, 4, 5))
    with pytest.raises(ValueError, match="origin"):
        meshing.TSDFVolume((0, nan, 0), 0.1, (3, 4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.TSDFVolume((0, 0, 0), 0.1, (3, 4, 5), device="cpu")


# --------------------------------------------------------------------------------------------------- case table
def g_rot(a, b):
    """a and b are the same cycle"""
    return any(tuple(a[i:]) + tuple(a[:i]) == tuple(b) for i in range(len(a)))


def test_case_table_is_the_rule():
    """The 16 cases per orientation that tsdf.hip writes out equal the table derived here from the header's rule; the rule
    itself: 0, 1 or 2 triangles for 0 / 4, 1 / 3 or 2 inside corners, every vertex on an edge whose ends differ, the two
    orientations mirror images, and complementary patterns the same triangles turned round."""
    from vggsfm_amd import meshing
    got, want = meshing.case_table(), C.derive_case_table()
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape == (2, 16, 7)
    assert np.array_equal(got, want)
    for si in range(2):
        for pattern in range(16):
            row = want[si, pattern]
            inside = bin(pattern).count("1")
            assert row[0] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[inside] and (row[1 + 3 * row[0]:] == -1).all()
            for e in row[1:1 + 3 * row[0]]:
                x, y = C.TET_EDGES[e]
                assert (pattern >> x & 1) != (pattern >> y & 1)
            tris = [tuple(row[1 + 3 * r:4 + 3 * r]) for r in range(row[0])]
            cyc = lambda t: {(t[0], t[1], t[2]), (t[1], t[2], t[0]), (t[2], t[0], t[1])}
            used = lambda rows: sorted({int(e) for t in rows for e in t})
            other = [tuple(want[1 - si, pattern][1 + 3 * r:4 + 3 * r]) for r in range(row[0])]
            flipped = [tuple(want[si, 15 - pattern][1 + 3 * r:4 + 3 * r]) for r in range(row[0])]
            for group in (other, flipped):                                   # the same vertices, the other way round
                assert used(group) == used(tris)
                if row[0] == 1:
                    assert cyc(group[0]) == cyc(tris[0][::-1])
                if row[0] == 2:                                              # the quad's cycle, reversed
                    quad = lambda g: (g[0][0], g[0][1], g[0][2], g[1][2])
                    q, r4 = quad(tris), quad(group)[::-1]
                    assert g_rot(q, r4)
    assert [C.perm_sign(p) for p in C.PERMS] == [1, -1, -1, 1, 1, -1]
    assert [C.tet_corners(t)[1:3] for t in (0, 5)] == [[(1, 0, 0), (1, 1, 0)], [(0, 0, 1), (0, 1, 1)]]


def test_every_sign_pattern_of_one_cell_is_consistent():
    """All 256 sign patterns of a 2 x 2 x 2 grid: every face names three different vertices that exist, a directed edge
    appears at most once, the vertices are zeros of the piecewise-linear interpolant of the split, and that interpolant grows
    along every triangle's normal."""
    for pattern in range(256):
        case = C.sign_pattern_volume(pattern)
        out = C.extract(**case)
        faces, V = out["faces"], len(out["vertices"])
        assert V == int(out["counts"][0]) == bin(int(out["edge_mask"][0])).count("1") + sum(
            bin(int(m)).count("1") for m in out["edge_mask"][1:])
        if pattern in (0, 255):
            assert V == 0 and len(faces) == 0
            continue
        assert len(faces) > 0 and faces.min() >= 0 and faces.max() < V
        assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
        top = C.topology(faces, V)
        assert top["duplicates"] == 0, pattern
        n, c = C.face_normals(out["vertices"], faces)
        length = np.linalg.norm(n, axis=1)
        assert (length > 0).all()
        s8 = case["tsdf_sum"] / case["weight_sum"]
        step = 1e-3 * n / length[:, None]
        assert (C.kuhn_interpolant(s8, c + step) > C.kuhn_interpolant(s8, c - step)).all(), pattern
        assert np.abs(C.kuhn_interpolant(s8, out["vertices"])).max() < 1e-12      # the vertices are zeros of the interpolant


# --------------------------------------------------------------------------------------------------- topology
def test_sphere_is_closed_and_faces_outwards():
    """13 x 11 x 10, centre (6.1, 5.2, 4.6), radius 3.7, unit voxels: each directed edge once and its reverse once,
    V - E + F = 2, every face normal . (centroid - centre) > 0, no face of zero area; the vertex normals are unit vectors that
    point outwards (measured: within 1.9 degrees of the radial direction) and the vertices lie on the sphere within L^2 / (8 R) = 3 / (8 R) = 0.101 voxels, the error of
    the linear interpolation of a distance of curvature 1 / R along an edge of length L <= sqrt(3)."""
    ref = C.volume_reference("sphere")
    V, F = len(ref["vertices"]), len(ref["faces"])
    top = C.topology(ref["faces"], V)
    n, c = C.face_normals(ref["vertices"], ref["faces"])
    radial = ref["vertices"] - C.SPHERE_CENTRE
    r = np.linalg.norm(radial, axis=1)
    cos = (ref["normals"].astype(np.float64) * radial).sum(-1) / r
    print(f"\nsphere: {V} vertices, {F} faces, euler {top['euler']}; |r - R| <= {np.abs(r - C.SPHERE_RADIUS).max():.3e}; "
          f"normal against radial: cos >= {cos.min():.6f}")
    assert (V, F) == (764, 1524) and top["closed"] and top["euler"] == 2 and top["used"] == V
    assert ((n * (c - C.SPHERE_CENTRE)).sum(-1) > 0).all() and (np.linalg.norm(n, axis=1) > 0).all()
    assert np.abs(r - C.SPHERE_RADIUS).max() <= 3.0 / (8.0 * C.SPHERE_RADIUS) and cos.min() > 0
    assert np.abs(np.linalg.norm(ref["normals"].astype(np.float64), axis=1) - 1).max() < 1e-6
    want = C._colour_field(C.SPHERE_DIMS).reshape(10, 11, 13, 3)              # a linear colour field is reproduced
    v = ref["vertices"]
    lin = np.stack([0.2 + 0.05 * v[:, 0], 0.9 - 0.04 * v[:, 1], 0.3 + 0.03 * v[:, 2]], -1)
    assert np.abs(ref["rgb"] - lin).max() < 1e-6 and want.shape[-1] == 3
    plain = C.volume_reference("sphere_no_colour")
    assert plain["faces"].tobytes() == ref["faces"].tobytes() and plain["vertices"].tobytes() == ref["vertices"].tobytes()
    assert not plain["rgb"].any()


def test_two_spheres_have_euler_number_four():
    ref = C.volume_reference("two_spheres")
    top = C.topology(ref["faces"], len(ref["vertices"]))
    print(f"\ntwo spheres: {len(ref['vertices'])} vertices, {len(ref['faces'])} faces, euler {top['euler']}")
    assert top["closed"] and top["euler"] == 4 and top["used"] == len(ref["vertices"])
    n, c = C.face_normals(ref["vertices"], ref["faces"])
    nearest = np.where((np.linalg.norm(c - C.TWO_CENTRES[0], axis=1) < np.linalg.norm(c - C.TWO_CENTRES[1], axis=1))[:, None],
                       C.TWO_CENTRES[0], C.TWO_CENTRES[1])
    assert ((n * (c - nearest)).sum(-1) > 0).all()


def test_all_inside_all_outside_and_one_cell():
    for name in ("all_inside", "all_outside"):
        ref = C.volume_reference(name)
        assert len(ref["vertices"]) == 0 and len(ref["faces"]) == 0 and not ref["edge_mask"].any() and not ref["counts"].any()
    tiny = C.volume_reference("tiny")
    assert tiny["group_counts"].shape == (1, 2) and len(tiny["faces"]) > 0
    big = C.volume_reference("plane_67x65x63")
    G = len(big["group_counts"])
    assert G == 1072 > 1024                                  # both levels of the count carry: more groups than one chunk
    assert (big["group_counts"][1024:] > 0).any() and big["group_offsets"][1024:, 0].min() > 0
    n, c = C.face_normals(big["vertices"], big["faces"])
    assert (n @ np.array(C.PLANE_NORMAL) > 0).all()
    assert C.topology(big["faces"], len(big["vertices"]))["duplicates"] == 0


def test_holes_open_the_mesh_only_where_nodes_are_invalid():
    """A block of invalid nodes in the sphere's volume: no vertex sits on an edge with an invalid end, every face names
    vertices that exist, and the only directed edges without a reverse lie within one voxel of the block."""
    ref, full = C.volume_reference("holes"), C.volume_reference("sphere")
    nx, ny, nz = C.SPHERE_DIMS
    invalid = np.zeros((nz, ny, nx), bool)
    invalid[C.HOLE] = True
    owner, edge = ref["vertex_edge"].T
    other = owner + np.array([C._offset(C._code(d), C.SPHERE_DIMS) for d in C.EDGE_DIRS])[edge]
    assert not invalid.reshape(-1)[owner].any() and not invalid.reshape(-1)[other].any()
    V = len(ref["vertices"])
    assert 0 < V < len(full["vertices"]) and 0 < len(ref["faces"]) < len(full["faces"])
    assert ref["faces"].min() >= 0 and ref["faces"].max() < V
    top = C.topology(ref["faces"], V)
    assert not top["closed"] and top["duplicates"] == 0 and len(top["boundary"]) > 0
    lo = np.array([C.HOLE[2].start, C.HOLE[1].start, C.HOLE[0].start]) - 1.0
    hi = np.array([C.HOLE[2].stop, C.HOLE[1].stop, C.HOLE[0].stop])           # stop - 1 + 1
    ends = ref["vertices"][top["boundary"].reshape(-1)]
    print(f"\nholes: {V} vertices, {len(ref['faces'])} faces, {len(top['boundary'])} open edges")
    assert ((ends >= lo) & (ends <= hi)).all()
    n, c = C.face_normals(ref["vertices"], ref["faces"])
    assert ((n * (c - C.SPHERE_CENTRE)).sum(-1) > 0).all()


# --------------------------------------------------------------------------------------------------- against truth
@pytest.mark.parametrize("name", C.TRUTH_CASES)
def test_restatement_against_the_true_plane(name):
    """24 x 32, 3 views, true depths rounded to float32, voxel 0.05, truncation 0.2, 21 x 17 x 13 nodes: 1353 vertices and
    2560 faces, all facing the cameras; the distance of the vertices from the true plane within 2 x what was measured when
    the test was written (meshing_cases.TRUTH_MEDIAN, TRUTH_LARGEST): median 3.353e-3, largest 8.230e-3 (k = 0) and
    3.353e-3, 8.210e-3 (k = 0.08) -- the along-axis distance of a plane slanted by 12 degrees, sampled at the nearest pixel."""
    ref = C.integration_reference(name)
    dist = FC.plane_distance(ref["vertices"])
    n, _ = C.face_normals(ref["vertices"], ref["faces"])
    print(f"\n{name}: {len(ref['vertices'])} vertices, {len(ref['faces'])} faces; distance to the plane: median "
          f"{np.median(dist):.4e}, largest {dist.max():.4e}")
    assert (len(ref["vertices"]), len(ref["faces"])) == (1353, 2560)
    assert np.median(dist) <= 2 * C.TRUTH_MEDIAN and dist.max() <= 2 * C.TRUTH_LARGEST
    assert (n[:, 2] < 0).all() and (ref["normals"][:, 2] < 0).all()             # the cameras look along +z
    angle = FC.normal_angle_deg(ref["normals"])
    print(f"vertex normals against the plane's: median {np.nanmedian(angle):.3f} deg, largest {np.nanmax(angle):.3f} deg")
    assert C._nonzero_rows(ref["normals"]).all()
    frames = C.integration_cases()[name]["frames"]                              # a colour is a mean of means of frame values
    assert (ref["rgb"] >= frames.min() - 1e-6).all() and (ref["rgb"] <= frames.max() + 1e-6).all() and ref["rgb"].std() > 0


# --------------------------------------------------------------------------------------------------- ties
def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests compare bits, so in every case they use no decision may sit on its threshold: the smallest |s| at a
    valid node, |sdf + trunc|, the distance of x + 0.5 and y + 0.5 from an integer, |weight_sum - min_weight|, |Xc[2]| and
    the length of an interpolated gradient are each > 1e-9.  Measured: value 1.2e-4 (the 67 x 65 x 63 plane) .. 3.2e-2,
    trunc 3.9e-5, round 6.4e-7, weight 4.7e-3, front 3.7, gradient 0.59."""
    worst = {}
    for kind, names, ref in (("volume", C.volume_cases(), C.volume_reference),
                             ("integration", C.integration_cases(), C.integration_reference)):
        for name in names:
            m = ref(name)["margins"]
            print(kind, name, {k: f"{v:.2e}" for k, v in m.items()})
            for k, v in m.items():
                assert v > 1e-9, (name, k, v)
                worst[k] = min(worst.get(k, np.inf), v)
    assert set(worst) == {"value", "weight", "gradient", "front", "round", "trunc"}
    print({k: f"{v:.2e}" for k, v in worst.items()})


def test_cases_cover_what_the_kernel_can_get_wrong():
    cases = C.integration_cases()
    assert {c["depth"].shape[1:] for c in cases.values()} == {(24, 32), (21, 35)}
    assert {c["dims"] for c in cases.values()} == {(21, 17, 13), (9, 7, 5)} and cases["many_views"]["depth"].shape[0] == 258
    assert {float(c["cams"][0, 3]) for c in cases.values()} == {0.0, 0.08}
    assert cases["weights"]["weights"] is not None and (cases["weights_zeros"]["weights"] == 0).any()
    assert cases["no_frames"]["frames"] is None and C.integration_reference("no_frames")["rgb_sum"] is None
    empty = C.integration_reference("all_zero")
    assert not empty["weight_sum"].any() and len(empty["vertices"]) == 0 and len(empty["faces"]) == 0
    # the view facing away adds nothing: the volumes of the first two views alone
    away = C.integration_reference("facing_away")
    two = C.run_integration(cases["facing_away"], 0, 2)
    assert away["tsdf_sum"].tobytes() == two[0].tobytes() and away["weight_sum"].tobytes() == two[1].tobytes()
    assert away["weight_sum"].max() == 2.0 and C.integration_reference("k08_24x32")["weight_sum"].max() == 3.0
    # split calls add up to one call, bit for bit, in the restatement too
    case = cases["weights"]
    part = C.run_integration(case, 0, 2)
    both = C.run_integration(case, 2, 3, part[:3])
    ref = C.integration_reference("weights")
    assert all(both[q].tobytes() == ref[k].tobytes() for q, k in enumerate(("tsdf_sum", "weight_sum", "rgb_sum")))
    # the depth step leaves a wall: more faces than the plane alone
    assert len(C.integration_reference("depth_step")["faces"]) > len(C.integration_reference("k08_24x32")["faces"])
    assert len(C.integration_reference("holes")["faces"]) < len(C.integration_reference("k08_24x32")["faces"])
    for dims in ((21, 17, 13), (9, 7, 5), C.SPHERE_DIMS, C.PLANE_DIMS):    # no grid is a multiple of a group of 256 nodes
        assert (dims[0] * dims[1] * dims[2]) % C.GROUP != 0
    assert (21 * 35) % 256 != 0


# --------------------------------------------------------------------------------------------------- PLY
def test_ply_round_trip_empty_mesh_and_foreign_header(tmp_path):
    from vggsfm_amd import fusion, meshing
    ref = C.volume_reference("sphere")
    mesh = meshing.Mesh(ref["vertices"], ref["normals"], ref["rgb"], ref["faces"])
    path = str(tmp_path / "sphere.ply")
    meshing.write_mesh_ply(path, mesh)
    back = meshing.read_mesh_ply(path)
    assert back.vertices.tobytes() == mesh.vertices.tobytes() and back.normals.tobytes() == mesh.normals.tobytes()
    assert back.faces.dtype == np.int32 and back.faces.tobytes() == mesh.faces.tobytes()
    assert np.abs(back.rgb.astype(np.float64) - np.clip(mesh.rgb, 0, 1)).max() <= 0.5 / 255 + 1e-7
    again = str(tmp_path / "again.ply")
    meshing.write_mesh_ply(again, back)                                       # what was read writes the same file
    assert open(again, "rb").read() == open(path, "rb").read()
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    assert head[2] == "element vertex 764" and head[-3:-1] == ["element face 1524", "property list uchar int vertex_indices"]
    # the vertex block is the cloud format: fusion's reader takes the file's vertices when the face element is cut away
    empty = meshing.Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    path0 = str(tmp_path / "empty.ply")
    meshing.write_mesh_ply(path0, empty)
    back0 = meshing.read_mesh_ply(path0)
    assert back0.vertices.shape == (0, 3) and back0.faces.shape == (0, 3) and back0.faces.dtype == np.int32
    cloud = fusion.FusedCloud(ref["vertices"], ref["normals"], ref["rgb"], np.zeros(764, np.int32), None, None)
    foreign = str(tmp_path / "cloud.ply")
    fusion.write_ply(foreign, cloud)
    for bad in (foreign, __file__):
        with pytest.raises(ValueError):
            meshing.read_mesh_ply(bad)
    ascii_ply = tmp_path / "ascii.ply"
    ascii_ply.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="binary little-endian"):
        meshing.read_mesh_ply(str(ascii_ply))
    cut = tmp_path / "cut.ply"
    cut.write_bytes(open(path, "rb").read()[:-5])
    with pytest.raises(ValueError, match="bytes of data"):
        meshing.read_mesh_ply(str(cut))
