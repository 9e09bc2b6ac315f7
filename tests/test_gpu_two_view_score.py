"""GPU: ``vgg_fmat_score`` and ``vgge_emat_score`` are one computation (two_view_score_kernel, csrc/two_view.hpp): with
no match mask and the same threshold for every pair the two entries must write the same counts and the same bits of the
residual sums, -1 / 0.0 for a dead hypothesis, and nothing outside their (B, K) outputs.  The match mask of the
fundamental entry is checked against a float64 recount with oracle/fundamental.py's ``sampson_sq``.

N = 70: a lane sweeps one or two points (more than one stride of 64, not a multiple of it).  K = 9: one workgroup with a
ragged last wavefront; K = 17: two workgroups, the second with one hypothesis.  In pair 1 the four hypotheses of the
second wavefront are all dead (the kernel's early-out)."""
import numpy as np
import pytest
import torch

from oracle import fundamental as OF
from vggsfm_amd import _lib

pytestmark = pytest.mark.gpu

B, N, THR = 2, 70, 0.25
GUARD = 64                       # sentinel elements on either side of an output
DROPPED = (0, 64, 69)


def _inputs(K):
    rng = np.random.default_rng(100 + K)
    p1, p2 = rng.uniform(-1, 1, (B, N, 2)), rng.uniform(-1, 1, (B, N, 2))
    M = rng.standard_normal((B, K, 3, 3))
    flag = np.ones((B, K), np.uint8)
    flag[:, 2] = 0
    flag[:, K - 1] = 0
    flag[1, 4:8] = 0
    return p1, p2, M, flag


def _score(entry, K, p1, p2, M, flag, mask=None):
    """counts (B,K), sums (B,K) and whether the guard bands around both outputs kept their sentinel"""
    L = _lib.lib()
    d1, d2, dM, dflag = (torch.from_numpy(x).cuda() for x in (p1, p2, M, flag))
    dmask = None if mask is None else torch.from_numpy(mask).cuda()
    cbuf = torch.full((B * K + 2 * GUARD,), -77, dtype=torch.int32, device="cuda")
    sbuf = torch.full((B * K + 2 * GUARD,), -77.5, dtype=torch.float64, device="cuda")
    cnt, rs = cbuf[GUARD:GUARD + B * K], sbuf[GUARD:GUARD + B * K]
    if entry == "fmat":
        _lib.check(L.vgg_fmat_score(d1, d2, dmask, dM, dflag, B, N, K, THR, cnt, rs, _lib.stream_ptr()), "vgg_fmat_score")
    else:
        thr = torch.full((B,), THR, dtype=torch.float64, device="cuda")
        _lib.check(L.vgge_emat_score(d1, d2, dM, dflag, thr, B, N, K, cnt, rs, _lib.stream_ptr()), "vgge_emat_score")
    torch.cuda.synchronize()
    c, s = cbuf.cpu().numpy(), sbuf.cpu().numpy()
    guards = all((x[:GUARD] == v).all() and (x[GUARD + B * K:] == v).all() for x, v in ((c, -77), (s, -77.5)))
    return c[GUARD:GUARD + B * K].reshape(B, K), s[GUARD:GUARD + B * K].reshape(B, K), guards


@pytest.mark.parametrize("K", [9, 17])
def test_the_two_scoring_entries_are_one_computation(K):
    p1, p2, M, flag = _inputs(K)
    cf, sf, gf = _score("fmat", K, p1, p2, M, flag)
    ce, se, ge = _score("emat", K, p1, p2, M, flag)
    assert gf and ge, "written outside (B, K)"
    live = flag.astype(bool)
    np.testing.assert_array_equal(cf, ce)
    np.testing.assert_array_equal(sf.view(np.int64), se.view(np.int64))
    assert (cf[~live] == -1).all() and (cf[live] >= 0).all()
    assert (sf[~live].view(np.int64) == 0).all()                       # +0.0 exactly
    assert 0 < cf[live].sum() < live.sum() * N                          # the threshold splits the matches
    # an all-ones mask is no mask
    c1, s1, g1 = _score("fmat", K, p1, p2, M, flag, np.ones((B, N), np.uint8))
    assert g1
    np.testing.assert_array_equal(c1, cf)
    np.testing.assert_array_equal(s1.view(np.int64), sf.view(np.int64))
    # a mask that drops points: float64 recount on the kept points
    mask = np.ones((B, N), np.uint8)
    mask[:, list(DROPPED)] = 0
    cm, sm, gm = _score("fmat", K, p1, p2, M, flag, mask)
    assert gm
    keep = mask[0].astype(bool)
    for b in range(B):
        r = OF.sampson_sq(M[b], p1[b], p2[b])[:, keep]
        inl = r <= THR
        np.testing.assert_array_equal(cm[b][live[b]], inl.sum(1)[live[b]])
        np.testing.assert_allclose(sm[b][live[b]], np.where(inl, r, 0.0).sum(1)[live[b]], rtol=1e-11, atol=0)
    assert (cm[~live] == -1).all() and (sm[~live].view(np.int64) == 0).all()
    assert (cm[live] <= cf[live]).all() and (cm[live] < cf[live]).any()      # the dropped points were counted before
