"""The BA launches live in several translation units (csrc/ba_cam.hip, ba_point.hip, ba_tiles.hip; the driver is ba.hip) and
share ONE profiler, vgg::g_prof: the launch counts that vgg_ba_profile_read reports per kernel id after one solve.  A unit
with a copy of its own would count its launches where no entry point reads them -- zero for every id outside the driver."""
import ctypes

import pytest

from tests.test_gpu_ba_step_sweep import small_case
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA

pytestmark = pytest.mark.gpu

# kProfLinearize, kProfPointPass, kProfCamRhs, kProfSchurTile, kProfCholesky, kProfPointStep, kProfSchurTileDiag (ba_types.hpp)
IDS = ("linearize", "point_pass", "cam_rhs", "schur_tile", "cholesky", "point_step", "schur_tile_diag")


def launch_counts(L):
    counts = []
    for kid in range(len(IDS)):
        total_ms, n = ctypes.c_double(), ctypes.c_int()
        assert L.vgg_ba_profile_read(kid, ctypes.byref(total_ms), ctypes.byref(n), 1) == 0
        counts.append(n.value)
    return dict(zip(IDS, counts))


def test_every_unit_counts_its_launches_in_the_one_profiler():
    """6 cameras x 48 points, shared SIMPLE_RADIAL, focal and distortion refined, three LM iterations with the tolerances off:
    vgg_ba_solve enqueues four rounds of phases (the fourth only checks, its launches return at once but are launched and
    counted).  One camera group and few observations: one merged tile launch per round under the id of the off-diagonal
    launch, none under the diagonal one's.  Recorded from the library before the split, on an MI355X:
      default (reduced right-hand side from the tile launch): linearize 4, point_pass 4, cam_rhs 0, schur_tile 4, cholesky 4,
                                                              point_step 4, schur_tile_diag 0
      vgg_ba_set_tile_rhs(0) (camera pass):                   the same, but cam_rhs 4"""
    L = _lib.lib()
    _, build, opt = small_case("radial_shared_kd2", "TRIVIAL")
    got = {}
    try:
        assert L.vgg_ba_profile(1, 64) == 0
        for mode in (2, 0):
            assert L.vgg_ba_set_tile_rhs(mode) == 0
            summ, _ = BA.solve(build(False), opt)
            assert summ["num_iterations"] == 3
            got[mode] = launch_counts(L)
            print(f"\nvgg_ba_set_tile_rhs({mode}): {got[mode]}")
    finally:
        L.vgg_ba_set_tile_rhs(2)
        L.vgg_ba_profile(0, 0)
    assert got[2] == dict(linearize=4, point_pass=4, cam_rhs=0, schur_tile=4, cholesky=4, point_step=4, schur_tile_diag=0)
    assert got[0] == dict(linearize=4, point_pass=4, cam_rhs=4, schur_tile=4, cholesky=4, point_step=4, schur_tile_diag=0)
    assert got[2]["cam_rhs"] == 0 and got[0]["cam_rhs"] > 0
