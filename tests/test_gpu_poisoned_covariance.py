"""The covariance entries (vggc_spd_inverse, vggc_ba_covariance) on poisoned, guard-banded memory, in the form of
tests/test_gpu_poisoned_pnp.py: the matrix, every workspace and every output come from ``torch.empty`` and are filled with
0x00, 0xFF and 0x7F and framed by guard bands; what is read back must be run-to-run deterministic, bit-identical across the
patterns, free of the pattern, and no guard byte may change.  Sizes that are no multiple of 16: n = 77 for the inverse (two
64-blocks, the second of 13 rows), case c for the bundle adjustment (n = 104, 17 cameras) -- once with every optional output
NULL, once with all of them -- and case e (7 x 7 blocks, per-camera intrinsics, n = 231) with all of them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ba_system_cases as SC
from tests import covariance_cases as CC
from tests.test_gpu_poisoned_memory import _check_poisoned
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA

pytestmark = pytest.mark.gpu


def _spd(n):
    def case(mp):
        L = _lib.lib()
        A_host, ref, dev, bound, _ = CC.spd_reference(n)
        A = torch.empty((n, n), dtype=torch.float64, device="cuda")          # (poisoned: the strict upper triangle stays so)
        low = torch.ones(n, n, device="cuda").tril().bool()
        A[low] = torch.from_numpy(A_host).cuda()[low]
        ws = torch.empty(L.vggc_spd_inverse_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(L.vggc_spd_inverse(A, n, ws, fail, _lib.stream_ptr()), "vggc_spd_inverse")
        X = A.cpu().numpy()
        assert int(fail.cpu()[0]) == 0
        d = np.diag(ref).astype(np.float64)
        assert float((np.abs((X - ref).astype(np.float64)) / np.sqrt(np.outer(d, d))).max()) <= bound
        assert X.tobytes() == X.T.copy().tobytes()
    return case


def _ba(name, all_outputs):
    def case(mp):
        L = _lib.lib()
        opt = SC.options_of(SC.CASES[name])
        prob = SC.compile_case(name, "cuda")
        prob.refine_focal, prob.refine_extra = opt.refine_focal_length, opt.refine_extra_params
        prob.loss, prob.loss_scale = BA.LOSS_ID[opt.loss_function_type], opt.loss_function_scale
        cp, co = prob.c_struct(), BA._c_options(opt, overlap=False)
        C, NI, P = prob.cam_t.shape[0], prob.intr.shape[0], prob.pts.shape[0]
        kd = int(prob.refine_focal) + int(prob.refine_extra and prob.camera_model == 1)
        n = 6 * C + kd * NI
        flags = 3 if all_outputs else 1
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
        outs = [new(n, n), new(C, 6, 6), new(NI, kd, kd), new(C, 6, kd), new(P, 3, 3)] if all_outputs else [None] * 5
        nbytes = L.vggc_ba_covariance_workspace_bytes(ctypes.byref(cp), ctypes.byref(co), flags)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(L.vggc_ba_covariance(ctypes.byref(cp), ctypes.byref(co), ws, nbytes, flags, *outs, fail, _lib.stream_ptr()),
                   "vggc_ba_covariance")
        assert int(fail.cpu()[0]) == 0
        if all_outputs:
            red, pose, intr, pose_intr, pts = (t.cpu().numpy() for t in outs)
            R = CC.reference(name, SC.host_arrays(prob, SC.CASES[name]))
            got = CC.SimpleNamespace(pose=pose, intrinsics=intr, pose_intrinsics=pose_intr, points=pts)
            for k, (err, zeros) in CC.errors(got, R.ref).items():
                assert zeros and err <= R.bounds[k], (k, err, R.bounds[k])
            assert red.tobytes() == red.T.copy().tobytes()
    return case


CASES = {
    "spd_inverse_77": _spd(77),
    "ba_c_no_optional_output": _ba("c", False),
    "ba_c_all_outputs": _ba("c", True),
    "ba_e_all_outputs": _ba("e", True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_covariance_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
