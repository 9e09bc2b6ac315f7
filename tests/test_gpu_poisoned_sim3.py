"""Every vggs_ entry (vggs_sim3_fit on both of its paths, vggs_sim3_score, vggs_sim3_ransac with rows that fail,
vggs_pose_pair_errors) on poisoned, guard-banded memory, in the form of tests/test_gpu_poisoned_essential.py: outputs and
workspaces come from ``empty``-family buffers filled with 0x00, 0xFF and 0x7F and framed by guard bands; what is read back
must be run-to-run deterministic, bit-identical across the patterns, hold no element that still shows the pattern
(every output element is written, the rows with success = 0 included), and no guard byte may change."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import sim3_cases as SC
from tests import test_gpu_sim3 as TS
from tests.test_gpu_poisoned_memory import _check_poisoned
from vggsfm_amd import sim3
from vggsfm_amd.utils import metric

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _score_inputs():
    sc = SC.score_case(SC.SCORE_TILE + 1)
    return sc, TS._hypotheses(sc)


def _fit(name):
    s, R, t, ok = TS._fit(TS.FIT[name])
    assert ok.all() == TS.FIT[name]["valid"] and np.isfinite(s).all() and np.isfinite(R).all() and np.isfinite(t).all()


def _score():
    sc, (s, R, t, ok) = _score_inputs()
    counts, sums = sim3.score_sim3(TS._dev(sc["src"]), TS._dev(sc["tgt"]), TS._dev(s), TS._dev(R), TS._dev(t),
                                   TS._dev(ok, torch.uint8), TS._dev(sc["max_error"]))
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    assert ((counts >= 0) == ok).all() and np.isfinite(sums).all() and (counts <= 300).all()


def _ransac(failing):
    sc = SC.ransac_case()
    if failing:
        sc = copy.deepcopy(sc)
        sc["samples"][0, :, 1] = sc["samples"][0, :, 0]
        sc["mask"][1] = False
        sc["mask"][1, [3, 77]] = True
    s, R, t, num, inl, success, counts, sums, best, rounds = TS._ransac(sc, 3)
    assert success.tolist() == ([False, False, True] if failing else [True, True, True])
    assert np.isfinite(s).all() and np.isfinite(R).all() and np.isfinite(t).all() and (num == inl.sum(1)).all()
    assert ((counts >= -1) & (counts <= 400)).all() and np.isfinite(sums).all() and ((rounds >= 0) & (rounds <= 3)).all()


def _pairs():
    pred, gt = SC.pose_set(65, 125)
    rot, trans = (x.cpu().numpy() for x in metric.pose_pair_errors(TS._dev(pred), TS._dev(gt)))
    assert ((rot >= 0) & (rot <= 180)).all() and ((trans >= 0) & (trans <= 90)).all()


CASES = {
    "fit_one_workgroup": lambda mp: _fit("n65"),
    "fit_batched_masks": lambda mp: _fit("b3_masks"),
    "fit_multi_workgroup": lambda mp: _fit("n5000_multi_workgroup"),
    "fit_invalid": lambda mp: _fit("collinear"),
    "score": lambda mp: _score(),
    "ransac": lambda mp: _ransac(False),
    "ransac_failing_rows": lambda mp: _ransac(True),
    "pair_errors": lambda mp: _pairs(),
}


@pytest.mark.parametrize("name", list(CASES))
def test_sim3_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
