"""Generate tests/golden/fundamental_*.npz: the regimes of tests/fundamental_cases.py through its long-double 7-point
solver and 8-point fit -- inputs, samples, reference solutions, root counts, sens, gap and admit flags, and for the whole
flow the reference's fit on the true inliers.  Nothing but numpy is needed:

    python -m oracle.gen_golden_fundamental [case ...]          (case: a regime name, or `flow`)

The vectors are committed; the test-suite only reads the .npz files (and regenerates a slice of each)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fundamental_cases as C  # noqa: E402


def main():
    only = sys.argv[1:]
    for name in C.REGIMES:
        if only and name not in only:
            continue
        out = C.build_regime(name)
        np.savez_compressed(C.path(name), **out)
        msg = f"wrote fundamental_{name}: left out {1 - out['admit'].mean():.4f} of {len(out['admit'])} samples, " \
              f"median sens {np.median(out['sens']):.2e}, root counts {np.bincount(out['ref_count'], minlength=4).tolist()}"
        if "e_admit" in out:
            msg += f"; 8-point left out {1 - out['e_admit'].mean():.4f} of {out['e_admit'].size}, smallest gap {out['e_gap'].min():.2e}"
        print(msg, flush=True)
    if not only or "flow" in only:
        out = C.build_flow()
        np.savez_compressed(C.path("flow"), **out)
        metas = np.array([v for k, v in out.items() if k.endswith("_meta")])
        print(f"wrote fundamental_flow: {len(metas)} fits, largest share inside the band {metas[:, 2].max():.4f}, "
              f"not admitted {int((metas[:, 3] == 0).sum())}", flush=True)


if __name__ == "__main__":
    main()
