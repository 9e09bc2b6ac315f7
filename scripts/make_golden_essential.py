"""Writes tests/golden/essential_<case>.npz for the 5-point essential-matrix tests.  The files are written with fixed zip
time stamps: the same script gives the same bytes.

  python scripts/make_golden_essential.py [case ...]

The reference's own ``estimate_essential`` (vggsfm/two_view_geo/essential.py:111-200) is imported through
oracle.ref_harness and run on the CPU.  Its ``run_5point`` needs kornia's polynomial solvers, which the harness can only
fabricate, so it is replaced by the independent CPU solver of tests/essential_cases.py (real roots only, the identity in
unused slots, the identity everywhere for fewer than five unmasked rows); ``generate_samples`` is replaced by a recorded
table.  Everything else -- normalisation, the float32 Sampson scoring, the choice of what to refine, the gathering of the
inlier sets, ``calculate_residual_indicator`` and the argmax -- is the reference's code.

Inputs are float32, and such that the reference's float32 normalisation is exact: focal lengths are powers of two, pixel
coordinates and principal points are multiples of 2^-10.  The float64 device code then starts from the same numbers.

Admission -- what a test may compare -- is decided here, from the reference side alone, stored, and asserted:
  flow cases   lo_num = 10 H: every candidate is refined, so the reference's unstable sort decides nothing.  A pair is
               admitted when, scored in float64, the reference's winner beats every candidate further than 1e-6 from it
               (Frobenius, up to sign): by inlier count, or at equal count by a mean-residual margin above 1e-3 relative.
               Every pair of every case must be admitted (the seeds below are chosen so).
               admit_match: the winner's float64 residual is further than 1e-3 relative from the threshold.
  solver case  admit_sample: the CPU solver's solution set of the sample is stable -- the same number of real solutions and
               every E moving by less than 1e-7 when the five points are jittered by 1e-13 relative.
No file may leave out more than 2 % of its matches or samples.

Cases:
  solver       B = 3 pairs, N = 64 matches (normalised, float64), H = 64 samples -> the CPU solver's candidates
  flow_equal   B = 2, N = 64, H = 16, lo_num = 160, 30 % outliers, 0.5 px noise, all focal lengths 1024
  flow_mixed   the same with focal lengths that differ per pair and per frame (per-pair thresholds)
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import essential_cases as EC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GRID = 2.0 ** -10

FLOW = {
    "flow_equal": dict(seed=315, focal=[[1024, 1024, 1024, 1024], [1024, 1024, 1024, 1024]]),
    "flow_mixed": dict(seed=314, focal=[[1024, 512, 2048, 1024], [512, 512, 1024, 2048]]),
}
SOLVER_SEED = 301
N, H, LO_NUM, MAX_ERROR = 64, 16, 160, 4.0


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[k]))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < 1_000_000, f"{path}: {os.path.getsize(path)} bytes"


def distinct_samples(rng, n, count, size=5):
    out = []
    while len(out) < count:
        s = rng.integers(0, n, size)
        if len(set(s.tolist())) == size:
            out.append(s)
    return np.array(out, np.int32)


def padded(Es):
    """(k,3,3) -> (10,3,3) with the identity in the unused slots, and k"""
    out = np.tile(np.eye(3), (10, 1, 1))
    out[:len(Es)] = Es[:10]
    return out, min(len(Es), 10)


def cpu_run_5point(points1, points2, masks=None, weights=None):
    """The stand-in for the reference's run_5point: tests/essential_cases.py on every set of the batch."""
    p1, p2 = points1.double().numpy(), points2.double().numpy()
    m = None if masks is None else masks.double().numpy()
    out = np.empty((len(p1), 10, 3, 3))
    for b in range(len(p1)):
        if m is not None and m[b].sum() < 5:
            out[b] = np.eye(3)
        else:
            out[b] = padded(EC.five_point(p1[b], p2[b], None if m is None else m[b]))[0]
    return torch.from_numpy(out)


def reference_modules():
    ref_harness.install()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import vggsfm.two_view_geo.essential as RE
        import vggsfm.two_view_geo.utils as RU

    def to_h(p):
        return torch.cat([p, torch.ones_like(p[..., :1])], -1)
    for mod in (RE, RU):
        mod.ones_like, mod.stack, mod.zeros, mod.where, mod.concatenate = (torch.ones_like, torch.stack, torch.zeros,
                                                                           torch.where, torch.cat)
        mod.Tensor = torch.Tensor
    RU.convert_points_to_homogeneous = to_h
    RE.run_5point = cpu_run_5point
    return RE


def make_solver():
    rng = np.random.default_rng(SOLVER_SEED)
    f, pp = np.ones(4), np.zeros(4)
    B, Hs = 3, 64
    p1, p2 = np.empty((B, N, 2)), np.empty((B, N, 2))
    for b in range(B):
        p1[b], p2[b], *_ = EC.two_view_scene(rng, N, f, pp, noise=1e-3)
    samples = distinct_samples(rng, N, Hs)
    cand, num, admit = np.empty((B, Hs, 10, 3, 3)), np.empty((B, Hs), np.int32), np.empty((B, Hs), bool)
    for b in range(B):
        for h in range(Hs):
            a1, a2 = p1[b, samples[h]], p2[b, samples[h]]
            Es = EC.five_point(a1, a2)
            Ej = EC.five_point(a1 * (1 + EC.JITTER * rng.uniform(-1, 1, a1.shape)),
                               a2 * (1 + EC.JITTER * rng.uniform(-1, 1, a2.shape)))
            cand[b, h], num[b, h] = padded(Es)
            admit[b, h] = 0 < len(Es) <= 10 and EC.set_deviation(Es, Ej) < EC.STABLE
    assert 1.0 - admit.mean() <= EC.CAP, f"solver: {(~admit).sum()} of {admit.size} samples are not admitted"
    save_npz(os.path.join(OUT, "essential_solver.npz"),
             dict(points1=p1, points2=p2, samples=samples, cpu_emat=cand, cpu_num=num, admit_sample=admit, cap=EC.CAP))
    print(f"solver: {(~admit).sum()} of {admit.size} samples left out; real solutions per sample {np.bincount(num.ravel())}")


def make_flow(RE, name, seed, focal):
    rng = np.random.default_rng(seed)
    focal = np.array(focal, np.float64)
    B = len(focal)
    pp = np.round(rng.uniform(300, 700, (B, 4)) / GRID) * GRID
    px1, px2 = np.empty((B, N, 2)), np.empty((B, N, 2))
    for b in range(B):
        px1[b], px2[b], *_ = EC.two_view_scene(rng, N, focal[b], pp[b], noise=0.5, outliers=0.3)
    px1, px2 = np.round(px1 / GRID) * GRID, np.round(px2 / GRID) * GRID
    samples = distinct_samples(rng, N, H)
    t32 = lambda a: torch.from_numpy(a.astype(np.float32))
    assert all((a.astype(np.float32) == a).all() for a in (px1, px2, pp, focal))
    calls = []

    def recording(points1, points2, masks=None, weights=None):
        calls.append(cpu_run_5point(points1, points2, masks, weights))
        return calls[-1]
    RE.run_5point = recording
    RE.generate_samples = lambda n, target, size: samples
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        emat, num, mask = RE.estimate_essential(t32(px1), t32(px2), t32(focal), t32(pp), max_ransac_iters=H,
                                                max_error=MAX_ERROR, lo_num=LO_NUM)
    assert len(calls) == 2 and emat.dtype == torch.float64
    cand_ransac = calls[0].numpy().reshape(B, 10 * H, 3, 3)
    cand_lo = calls[1].numpy().reshape(B, 10 * LO_NUM, 3, 3)
    emat, num, mask = emat.numpy(), num.numpy(), mask.numpy()
    # float64 re-scoring of everything the reference chose from
    allc = np.concatenate([cand_ransac, cand_lo], 1)
    thr = (MAX_ERROR / focal.mean(1)) ** 2
    res_w = np.empty((B, N))
    for b in range(B):
        n1, n2 = EC.normalise(px1[b], px2[b], focal[b], pp[b])
        r = EC.sampson_sq(allc[b], n1, n2)
        inl = r <= thr[b]
        cnt = inl.sum(1)
        mean = np.where(cnt > 0, (r * inl).sum(1) / np.maximum(cnt, 1), 1e6)
        w = int(np.argmin(EC.distance(allc[b], emat[b])))
        assert EC.distance(allc[b, w], emat[b]) == 0.0
        other = EC.distance(allc[b], emat[b]) > EC.DISTINCT
        beaten = (cnt < cnt[w]) | ((cnt == cnt[w]) & (mean - mean[w] > EC.MARGIN * mean[w]))
        assert (beaten | ~other).all(), f"{name} pair {b}: the winner does not beat {(~beaten & other).sum()} candidates"
        res_w[b] = r[w]
        print(f"{name} pair {b}: winner index {w} ({'LO' if w >= 10 * H else 'RANSAC'}), {cnt[w]} inliers in float64, "
              f"{num[b]} in the reference; runner-up count {np.sort(cnt[other])[-1]}")
    admit = np.abs(res_w - thr[:, None]) > EC.MARGIN * thr[:, None]
    assert 1.0 - admit.mean() <= EC.CAP
    save_npz(os.path.join(OUT, f"essential_{name}.npz"),
             dict(points1=px1.astype(np.float32), points2=px2.astype(np.float32), focal_length=focal.astype(np.float32),
                  principal_point=pp.astype(np.float32), samples=samples, max_error=MAX_ERROR, lo_num=LO_NUM,
                  cand_ransac=cand_ransac, cand_lo=cand_lo, ref_emat=emat, ref_inlier_num=num, ref_inlier_mask=mask,
                  ref_residuals=res_w, admit_match=admit, admit_pair=np.ones(B, bool), cap=EC.CAP))
    print(f"{name}: {(~admit).sum()} of {admit.size} matches left out")


def main():
    args = sys.argv[1:]
    want = lambda n: not args or n in args
    if want("solver"):
        make_solver()
    if any(want(n) for n in FLOW):
        RE = reference_modules()
        for name, cfg in FLOW.items():
            if want(name):
                make_flow(RE, name, **cfg)


if __name__ == "__main__":
    main()
