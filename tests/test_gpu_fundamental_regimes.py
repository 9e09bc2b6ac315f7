"""GPU: vgg_fmat_seven_point / vgg_fmat_score / vgg_fmat_eight_point and ``estimate_fundamental`` on the regimes of
tests/fundamental_cases.py: bit for bit against the mirror oracle/fundamental.py at the launch edges, against the
independent long-double references of the golden files by their own bounds, finite or flagged on degenerate scenes, and
the whole flow against the true inlier set.  Figures measured on an MI355X: DESIGN.md section 22."""
import numpy as np
import pytest
import torch

from oracle import fundamental as Fd
from tests import fundamental_cases as C
from vggsfm_amd import _lib
from vggsfm_amd.two_view_geo import estimate_fundamental

pytestmark = pytest.mark.gpu
HUGE = 1e300                    # a squared threshold every usable match passes: the 8-point mask is the valid mask


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def seven(x1, x2, smp):
    B, N, H = x1.shape[0], x1.shape[1], len(smp)
    d1, d2, ds = D(x1), D(x2), D(smp.astype(np.int32))
    F = torch.full((B, H, 3, 9), np.nan, dtype=torch.float64, device="cuda")
    v = torch.full((B, H, 3), 7, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vgg_fmat_seven_point(d1, d2, ds, B, N, H, F, v, _lib.stream_ptr()), "seven")
    return F.cpu().numpy().reshape(B, H, 3, 3, 3), v.cpu().numpy()


def score(x1, x2, vm, F, valid, thr):
    B, N, K = x1.shape[0], x1.shape[1], F.shape[1]
    d1, d2, dm, dF, dv = D(x1), D(x2), D(None if vm is None else vm.astype(np.uint8)), D(F.reshape(B, K, 9)), D(valid.astype(np.uint8))
    cnt = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    rs = torch.full((B, K), np.nan, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().vgg_fmat_score(d1, d2, dm, dF, dv, B, N, K, thr, cnt, rs, _lib.stream_ptr()), "score")
    return cnt.cpu().numpy(), rs.cpu().numpy()


def eight(x1, x2, vm, Fsrc, cnt, sel, thr):
    B, N, K, L = x1.shape[0], x1.shape[1], Fsrc.shape[1], sel.shape[1]
    d1, d2, dm = D(x1), D(x2), D(None if vm is None else vm.astype(np.uint8))
    dF, dc, ds = D(Fsrc.reshape(B, K, 9)), D(cnt.astype(np.int32)), D(sel.astype(np.int32))
    F = torch.full((B, L, 9), np.nan, dtype=torch.float64, device="cuda")
    ok = torch.full((B, L), 7, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vgg_fmat_eight_point(d1, d2, dm, dF, dc, ds, B, N, K, L, thr, F, ok, _lib.stream_ptr()), "eight")
    return F.cpu().numpy().reshape(B, L, 3, 3), ok.cpu().numpy()


def eight_on_masks(x1, x2, masks):
    """The 8-point fit of (N,2) points on each of the (M,N) masks: one pair per mask, any live source hypothesis."""
    M = len(masks)
    src = np.broadcast_to(np.eye(3).reshape(1, 1, 9), (M, 1, 9)).copy()
    F, ok = eight(np.broadcast_to(x1, (M,) + x1.shape).copy(), np.broadcast_to(x2, (M,) + x2.shape).copy(), masks, src,
                  np.ones((M, 1), np.int32), np.zeros((M, 1), np.int32), HUGE)
    return F[:, 0], ok[:, 0]


@pytest.fixture(scope="module")
def golden():
    return {name: C.load(name) for name in C.REGIMES}


def mirror_seven(x1, x2, smp):
    """The mirror on samples that may hold indices out of range: those rows are flagged and zero."""
    N = len(x1)
    bad = ((smp < 0) | (smp >= N)).any(1)
    s = np.where((smp < 0) | (smp >= N), 0, smp)
    F, v = Fd.seven_point(x1[s], x2[s])
    F[bad], v[bad] = 0.0, False
    return F, v


# ------------------------------------------------------------------------------------------------ (a) kernel == mirror
@pytest.mark.parametrize("H", [1, 5, 21, 22, 63, 64, 65])
def test_seven_point_and_score_equal_the_mirror_at_every_block_edge(golden, H):
    names = list(C.REGIMES)
    trio = [names[(3 * H + i * 5) % len(names)] for i in range(3)]
    x1, x2 = np.stack([golden[n]["x1"] for n in trio]), np.stack([golden[n]["x2"] for n in trio])
    N = x1.shape[1]
    x1[:, :7, 1], x2[:, :7, 1] = 2.0 * x1[:, :7, 0] + 5.0, 2.0 * x2[:, :7, 0] - 3.0          # seven collinear matches
    smp = golden[trio[0]]["samples"][:H].copy()
    special = np.array([[0, 1, 2, 3, 4, 5, 6], [9, 9, 9, 9, 9, 9, 9], [10, 11, 12, 10, 13, 14, 15], [20, 21, -1, 22, 23, 24, 25],
                        [30, 31, 32, 33, 34, 35, N]], np.int32)
    k = min(len(special), max(H - 1, 1) if H > 1 else 1)
    smp[H - k:] = special[:k] if H > 1 else special[3:4]
    rng = np.random.default_rng(H)
    vm = rng.random((3, N)) < np.array([0.9, 0.5, 1.0])[:, None]
    F, v = seven(x1, x2, smp)
    assert set(np.unique(v)) <= {0, 1}
    cnt, rs = score(x1, x2, vm, F.reshape(3, 3 * H, 3, 3), v.reshape(3, 3 * H), 1.0)
    for b in range(3):
        Fo, vo = mirror_seven(x1[b], x2[b], smp)
        np.testing.assert_array_equal(v[b].astype(bool), vo)
        np.testing.assert_array_equal(F[b], Fo)
        co, ro, _ = Fd.score(Fo.reshape(-1, 3, 3), vo.reshape(-1), x1[b], x2[b], vm[b], 1.0)
        np.testing.assert_array_equal(cnt[b], co)
        np.testing.assert_array_equal(rs[b], ro)


@pytest.mark.parametrize("N", C.EIGHT_N)
def test_score_and_eight_point_equal_the_mirror_at_every_stride_edge(golden, N):
    names = list(C.EQUALITY)
    trio = [names[(N + i * 5) % len(names)] for i in range(3)]
    x1 = np.stack([golden[n]["e_x1_1"][:N] for n in trio])
    x2 = np.stack([golden[n]["e_x2_1"][:N] for n in trio])
    H = 22
    rng = np.random.default_rng(N)
    smp = np.stack([rng.choice(N, 7, replace=False) for _ in range(H)]).astype(np.int32)
    vm = rng.random((3, N)) < np.array([1.0, 0.8, 0.6])[:, None]
    F, v = seven(x1, x2, smp)
    K = 3 * H
    Fa, va = F.reshape(3, K, 3, 3), v.reshape(3, K)
    cnt, rs = score(x1, x2, vm, Fa, va, 4.0)
    dead = [int(np.nonzero(va[b] == 0)[0][0]) if (va[b] == 0).any() else -1 for b in range(3)]
    sel = np.stack([np.concatenate([Fd._order(cnt[b])[:6], [-1, K, dead[b], 0]]) for b in range(3)]).astype(np.int32)
    F8, ok8 = eight(x1, x2, vm, Fa, cnt, sel, 4.0)
    # masks with 0, 7 and exactly 8 usable matches: every usable match is an inlier of a live hypothesis
    few = np.zeros((3, N), bool)
    few[1, rng.choice(N, 7, replace=False)] = True
    few[2, rng.choice(N, 8, replace=False)] = True
    live = np.stack([Fd._order(cnt[b])[:1] for b in range(3)]).astype(np.int32)
    Ff, okf = eight(x1, x2, few, Fa, cnt, live, HUGE)
    assert okf[:, 0].tolist()[:2] == [0, 0] and not Ff[:2].any()
    for b in range(3):
        co, ro, inl = Fd.score(Fa[b], va[b], x1[b], x2[b], vm[b], 4.0)
        np.testing.assert_array_equal(cnt[b], co)
        np.testing.assert_array_equal(rs[b], ro)
        inside = (sel[b] >= 0) & (sel[b] < K)
        s = np.where(inside, sel[b], 0)
        masks = inl[s] & (inside & (co[s] >= 0))[:, None]
        Fo, vo = Fd.eight_point(x1[b], x2[b], masks)
        np.testing.assert_array_equal(ok8[b].astype(bool), vo)
        np.testing.assert_array_equal(F8[b], Fo)
        assert not ok8[b, 6] and not ok8[b, 7] and (dead[b] < 0 or not ok8[b, 8])
        Fo, vo = Fd.eight_point(x1[b], x2[b], few[b][None] & (co[live[b]] >= 0)[:, None])
        np.testing.assert_array_equal(okf[b].astype(bool), vo)
        np.testing.assert_array_equal(Ff[b], Fo)
    assert okf[2, 0] == 1


# ------------------------------------------------------------------------------------------------ (b) kernel vs reference
@pytest.mark.parametrize("name", C.EQUALITY + ("planar80",))
def test_seven_point_against_the_independent_reference(golden, name):
    g = golden[name]
    F, v = seven(g["x1"][None], g["x2"][None], g["samples"])
    worst, bad = C.check_seven(g, F[0], v[0])
    print(f"{name}: largest deviation / max(1e-13, sens) = {worst:.3e} on {int(g['admit'].sum())} admitted samples")
    assert not bad, f"{len(bad)} samples, first:\n" + "\n".join(bad[:3])
    if name in ("sideways", "vertical"):
        for h in np.nonzero(g["admit"])[0]:
            assert C.distance(F[0, h][v[0, h].astype(bool)], g["F_true"]).min() <= max(C.FLOOR7, g["sens"][h])


@pytest.mark.parametrize("name", C.EQUALITY)
def test_eight_point_against_the_independent_reference(golden, name):
    g, bad, worst = golden[name], [], 0.0
    for label, x1, x2, m, Fref, gap, sens in C.eight_cases(g, name):
        F, ok = eight_on_masks(x1, x2, m[None])
        dev = float(C.distance(F[0], Fref)) if ok[0] else np.inf
        print(f"{name} {label}: deviation {dev:.2e}, x gap^2 / eps {dev * gap ** 2 / C.EPS:.2e}, gap {gap:.2e}, sens {sens:.2e}")
        worst = max(worst, dev / C.bound8(gap, sens))
        if not dev <= C.bound8(gap, sens):
            bad.append((label, dev, C.bound8(gap, sens)))
    print(f"{name}: largest deviation / bound {worst:.3e}")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (c) degenerate scenes
@pytest.mark.parametrize("name", C.DEGENERATE)
def test_degenerate_scenes_are_finite_or_flagged(golden, name):
    g = golden[name]
    F, v = seven(g["x1"][None], g["x2"][None], g["samples"])
    F, v = F[0], v[0].astype(bool)
    assert np.isfinite(F).all() and not F[~v].any()
    nrm = np.linalg.norm(F[v], axis=(-2, -1))
    assert np.abs(nrm - 1).max(initial=0) < 1e-12
    worst = 0.0
    for h in range(len(F)):
        h1, h2 = C._homog(g["x1"][g["samples"][h]]), C._homog(g["x2"][g["samples"][h]])
        for Fs in F[h][v[h]]:
            r = np.abs(np.einsum("ni,ij,nj->n", h2, Fs.astype(C.LD), h1)) / (np.linalg.norm(h1, axis=1) * np.linalg.norm(h2, axis=1))
            worst = max(worst, float(r.max()))
    print(f"{name}: {int(v.sum())} of {v.size} slots valid, largest constraint residual {worst:.2e}")
    assert worst <= 1e-6
    N = len(g["x1"])
    masks = np.stack([np.ones(N, bool), np.arange(N) % 3 > 0])
    F8, ok8 = eight_on_masks(g["x1"], g["x2"], masks)
    ok8 = ok8.astype(bool)
    assert np.isfinite(F8).all() and not F8[~ok8].any()
    assert np.abs(np.linalg.norm(F8[ok8], axis=(-2, -1)) - 1).max(initial=0) < 1e-12


# ------------------------------------------------------------------------------------------------ (d) the whole flow
@pytest.mark.parametrize("N", C.FLOW_N)
@pytest.mark.parametrize("batch", C.FLOW_BATCHES)
def test_whole_flow_finds_the_true_inlier_set(batch, N):
    flow = C.load("flow")
    pairs = C.FLOW_BATCHES[batch]
    scs = [C.flow_scene(n, s, N) for n, s in pairs]
    B = len(scs)
    smp = C.flow_samples(batch, N, np.stack([sc["inl"] for sc in scs]))
    x1, x2 = np.stack([sc["x1"] for sc in scs]), np.stack([sc["x2"] for sc in scs])
    err = scs[0]["max_error"]
    F7, v7 = seven(x1, x2, smp)
    worst = 0.0
    for vm in C.flow_masks(batch, N, B):
        for lo in C.FLOW_LO:
            run = lambda a, b_, m: estimate_fundamental(D(a), D(b_), max_error=err, lo_num=lo, valid_mask=D(m), samples=smp,
                                                        return_residuals=True)
            out = [t.cpu().numpy() for t in run(x1, x2, vm)]
            again = [t.cpu().numpy() for t in run(x1, x2, vm)]
            for a, b_ in zip(out, again):
                np.testing.assert_array_equal(a, b_)                                        # two runs, equal bits
            for b, sc in enumerate(scs):
                alone = [t.cpu().numpy() for t in run(x1[b:b + 1], x2[b:b + 1], None if vm is None else vm[b:b + 1])]
                for a, b_ in zip(out, alone):
                    np.testing.assert_array_equal(a[b], b_[0])                              # alone == its slice of the batch
                r = C.check_flow(flow, batch, N, b, sc, None if vm is None else vm[b], lo, out[0][b], out[1][b], out[2][b])
                if r["dev"] is not None:
                    worst = max(worst, r["dev"] / r["bound"])
                if lo == 0:                                                                 # the winner is a 7-point candidate
                    cands = F7[b][v7[b].astype(bool)]
                    scaled = np.where(np.abs(cands[:, 2:, 2:]) > 1e-8, cands / np.where(np.abs(cands[:, 2:, 2:]) > 1e-8, cands[:, 2:, 2:], 1.0), cands)
                    assert (scaled == out[0][b]).all((-2, -1)).any()
    print(f"{batch} N {N}: largest winner deviation / bound {worst:.3e}")
    with pytest.raises(ValueError):
        estimate_fundamental(D(x1), D(x2), max_error=err, lo_num=-1, samples=smp)
