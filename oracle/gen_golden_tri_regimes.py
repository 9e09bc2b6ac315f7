"""Generate tests/golden/tri_regimes_*.npz: the cases of tests/triangulation_cases.py through the REFERENCE's own
triangulate_tracks / triangulate_by_pair (float64, CPU, stable sort, the torch.manual_seed draws the tests replay) and
through the long-double restatement of tests/triangulation_cases.py.

Run where the reference tree is available (see oracle/ref_harness.py):
    python -m oracle.gen_golden_tri_regimes [case ...]
The vectors are committed; the test-suite only reads the .npz files (and regenerates slices of the long-double half).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import triangulation_cases as C  # noqa: E402
from oracle import ref_harness  # noqa: E402
from oracle.gen_golden import T, _StableSort, tc  # noqa: E402


def case_fixture(tri, name):
    case = C.build(name)
    pairs = C.draw_pairs(case)
    torch.manual_seed(case["seed"])
    with _StableSort():
        p3, num, msk = tri.triangulate_tracks(T(case["ext"]), tc(T(case["tn"])), max_ransac_iters=case["iters"],
                                              track_vis=tc(T(case["vis"])),
                                              track_score=None if case["score"] is None else tc(T(case["score"])),
                                              max_tri_points_num=case["max_pts"])
    out = dict(seed=case["seed"], iters=case["iters"], max_pts=case["max_pts"], size=case["size"],
               ref_points=p3.numpy(), ref_num=num.numpy(), ref_mask=msk.numpy())
    if case.get("hashed"):
        out["digest"] = C.input_digest(case)
    else:
        out.update(ext=case["ext"], tn=case["tn"], vis=case["vis"])
        if case["score"] is not None:
            out["score"] = case["score"]
    out.update({f"ld_{k}": v for k, v in C.reference(case, pairs).items()})
    np.savez_compressed(os.path.join(C.GOLDEN, f"tri_regimes_{name}.npz"), **out)
    adm = out["ld_admitted"]
    print(f"wrote tri_regimes_{name}: not admitted {1 - adm.mean():.4f}, delta {out['ld_delta']:.2e}, dev64 {out['ld_dev64']:.2e}, "
          f"reference vs long double on admitted: {int((out['ref_mask'][adm] != out['ld_mask'][adm]).sum())} mask bits", flush=True)


def pair_fixture(tri, group):
    ext, tn, size = C.pair_inputs(group)
    p3, che, ang = tri.triangulate_by_pair(T(ext)[None], T(tn)[None])
    ld = C.pair_reference(ext, tn)
    out = dict(size=size, ref_points=p3.numpy(), ref_che=che.numpy(), ref_ang=ang.numpy(), ld_points=ld["points"].astype(np.float64),
               ld_lam=ld["lam"].astype(np.float64), ld_che=ld["che"], ld_ang=ld["ang"].astype(np.float64))
    if group == "pair_sweep":
        out.update(ext=ext, tn=tn)
    np.savez_compressed(os.path.join(C.GOLDEN, f"tri_regimes_{C.pair_name(group)}.npz"), **out)
    print(f"wrote tri_regimes_{C.pair_name(group)}: {out['ld_che'].size} inputs", flush=True)


def main():
    tri, _, _ = ref_harness.load()
    torch.set_num_threads(8)
    only = sys.argv[1:]
    for name in C.NAMES:
        if not only or name in only:
            case_fixture(tri, name)
    for group in C.PAIR_GROUPS:
        if not only or C.pair_name(group) in only:
            pair_fixture(tri, group)


if __name__ == "__main__":
    main()
