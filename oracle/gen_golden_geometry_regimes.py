"""Generate tests/golden/geom_regimes_*.npz: the cases of tests/geometry_cases.py through the REFERENCE's own
project_3D_points, cam_from_img / iterative_undistortion and filter_all_points3D (float64, CPU) and through the long-double
restatement of tests/geometry_cases.py, one file per family of cases, every field named <case>__<field>.

Run where the reference tree is available (see oracle/ref_harness.py):
    python -m oracle.gen_golden_geometry_regimes
The vectors are committed; the test-suite rebuilds the inputs from the case table (the fixture holds their sha256) and reads
the recorded results.  The files are written with fixed zip timestamps, so a second run gives the same bytes.

From the restatement alone, because the reference cannot run them: `s4096` (the reference builds the (S^2, P) angle tensor).
The grid-stride cases are recorded on their distinct points / tracks; the tests tile them to the launch size.  The
reference's iteration count is the number of its apply_distortion calls divided by the nine of one iteration; the
max_iterations cases call its iterative_undistortion directly on its own normalisation.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import geometry_cases as C  # noqa: E402
from oracle import ref_harness  # noqa: E402


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).astype(np.float64))


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def reference_filter(helpers, job):
    kw = {k: v for k, v in job["kw"].items() if k != "behind_value"}           # (1e6 is written into the reference)
    m, d = helpers.filter_all_points3D(T(job["pts"]), T(job["tracks"]), T(job["ext"]), T(job["K"]), T(job["extra"]),
                                       return_detail=True, **kw)
    return dict(ref_mask=m.numpy().astype(bool), ref_detail=d.numpy().astype(bool))


def reference_project(helpers, job):
    px, pc = helpers.project_3D_points(T(job["pts"]), T(job["ext"]), T(job["K"]), T(job["extra"]), return_points_cam=True)
    only = helpers.project_3D_points(T(job["pts"]), T(job["ext"]), only_points_cam=True)
    assert torch.equal(only, pc)
    return dict(ref_px=px.numpy(), ref_pc=pc.numpy())


def reference_undistort(helpers, dist, job):
    calls = [0]
    orig = dist.apply_distortion

    def counting(*a, **kw):
        calls[0] += 1
        return orig(*a, **kw)

    dist.apply_distortion = counting
    try:
        if job["extra"] is None or job["max_iterations"] == 100:
            out = helpers.cam_from_img(T(job["tracks"]), T(job["K"]), T(job["extra"]))
        else:
            tn = helpers.cam_from_img(T(job["tracks"]), T(job["K"]), None)
            out = dist.iterative_undistortion(T(job["extra"]), tn, max_iterations=job["max_iterations"])
    finally:
        dist.apply_distortion = orig
    assert calls[0] % 9 == 0, "the reference fell back to single_undistortion"
    return dict(ref_values=out.numpy(), ref_iters=calls[0] // 9)


def case_record(mods, name):
    _, helpers, dist = mods
    job = C.build(name)
    r = C.evaluate(job)
    out = dict(digest=C.input_digest(job), figures=r["figures"])
    if job["kind"] == "filter":
        out.update(ld_mask=r["mask"], ld_detail=r["detail"], adm_mask=r["adm_mask"], adm_detail=r["adm_detail"], ld_best=r["best"])
        if name not in C.REFERENCE_CANNOT_RUN:
            out.update(reference_filter(helpers, job))
        line = (f"mask {int(r['mask'].sum())}/{len(r['mask'])}, admitted {r['adm_mask'].mean():.4f} / {r['adm_detail'].mean():.4f}, "
                f"dev err {r['figures'][0]:.2e} cz {r['figures'][1]:.2e} angle {r['figures'][2]:.2e}")
    elif job["kind"] == "project":
        out.update(ld_px=r["px"], ld_pc=r["pc"], cls=r["cls"], adm=r["adm"], **reference_project(helpers, job))
        line = f"classes {np.bincount(r['cls'].ravel(), minlength=4)}, admitted {r['adm'].mean():.4f}, dev64 px {r['figures'][0]:.2e} cam {r['figures'][1]:.2e}"
    else:
        out.update(ld_values=r["values"], ld_iters=r["iters"], adm_count=r["adm_count"], adm_elem=r["adm_elem"], swaps=r["swaps"],
                   **reference_undistort(helpers, dist, job))
        line = (f"iterations {r['iters']} (reference {out['ref_iters']}), swaps in step 1 {int(r['swaps'][0])}, admitted {r['adm_elem'].mean():.4f}, "
                f"dev64 {r['figures'][0]:.2e} stop {r['figures'][1]:.2e} swap {r['figures'][2]:.2e}")
    print(f"{name}: {line}", flush=True)
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    mods = ref_harness.load()
    torch.set_num_threads(1)
    for family, names in C.FAMILIES.items():
        arrays = {}
        for name in names:
            arrays.update(case_record(mods, name))
        path = os.path.join(C.GOLDEN, f"geom_regimes_{family}.npz")
        save_npz(path, arrays)
        print(f"wrote {os.path.relpath(path, ROOT)}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
