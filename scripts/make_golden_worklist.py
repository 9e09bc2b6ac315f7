"""Digests of the Schur work list (vggsfm_amd.ba.build_schur_tiles) on a dozen small problems -> tests/golden/schur_worklist.json.

The tables are what a device port of the work-list builder has to reproduce: chunk_desc, entries, tile_desc, obs_slot and
batch_desc, plus the number of segments.  Everything runs on CPU tensors (integer tables and float64 costs: nothing in them
depends on the device).  The committed digests were recorded from the builder as it stood BEFORE it was cut into stages
(DESIGN.md section 26); tests/test_schur_worklist_golden.py rebuilds the cases and compares.

    python scripts/make_golden_worklist.py            # rewrite the JSON from the code of this tree
    python scripts/make_golden_worklist.py --check    # compare, write nothing
"""
import argparse
import hashlib
import json
import os
import sys
from contextlib import contextmanager

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vggsfm_amd import ba as BA                                      # noqa: E402
from vggsfm_amd.scene import make_scene, perturb_for_ba              # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "schur_worklist.json")
TABLES = ("chunk_desc", "entries", "tile_desc", "obs_slot", "batch_desc")
HOOK_VARS = ("VGGSFM_AMD_DEBUG_HOOKS", "VGGSFM_TILE_ORDER")


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


@contextmanager
def settings(env=None, **consts):
    """Module constants of vggsfm_amd.ba and hook variables for the duration of one case; both are put back."""
    old_c = {k: getattr(BA, k) for k in consts}
    old_e = {k: os.environ.pop(k, None) for k in HOOK_VARS}
    try:
        for k, v in consts.items():
            setattr(BA, k, v)
        os.environ.update(env or {})
        yield
    finally:
        for k, v in old_c.items():
            setattr(BA, k, v)
        for k in HOOK_VARS:
            os.environ.pop(k, None)
            if old_e[k] is not None:
                os.environ[k] = old_e[k]


def _scene_tables(S, N, cam, shared, seed, masks=None):
    sc = make_scene(S, N, cam, shared_camera=shared, seed=seed)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=seed)
    m = sc.mask if masks is None else masks
    prob, _, _ = BA.compile_problem(T(pts0), T(ext0), T(K0), T(sc.tracks), T(m), T(extra0), shared, cam)
    return prob.chunk_desc, prob.entries, prob.tile_desc, prob.obs_slot, prob.num_segments, prob.batch_desc


def _bernoulli_masks(S, N, density, seed):
    """The masks of tests/test_host_logic.py::test_compile_problem_on_irregular_visibility."""
    rng = np.random.default_rng(seed)
    masks = rng.random((S, N)) < density
    if S > 4:
        masks[rng.integers(2, S)] = False                   # a camera that sees nothing
        masks[:, 0] = False
        masks[0, 0] = masks[S - 1, 0] = True                # a point seen by the first and the last camera only
    return masks


def _direct_tables():
    """build_schur_tiles on the random mask of tests/test_host_logic.py::test_schur_chunks_adaptive_cover."""
    torch.manual_seed(0)
    S, P = 40, 300
    m = torch.rand(S, P) < 0.4
    m[:2] = True
    pm = torch.nonzero(m.t())
    obs_cam = pm[:, 1].to(torch.int32)
    row_ptr = torch.zeros(P + 1, dtype=torch.int32)
    row_ptr[1:] = torch.cumsum(m.sum(0), 0).to(torch.int32)
    return BA.build_schur_tiles(row_ptr, obs_cam, max_chunks=40, num_batches=3, later_scale=0.875)


FULL = dict(SIMPLE_WORKLIST_MAX_OBS=0)                      # the full construction: density order, pattern grouping, cost model
C1 = (70, 400, "SIMPLE_RADIAL", True, 7)
# name -> (constants of vggsfm_amd.ba, hook variables, builder of the 6-tuple)
CASES = {
    "01_c70x400_shared_full": (FULL, None, lambda: _scene_tables(*C1)),
    "02_c70x400_shared_simple": (dict(SIMPLE_WORKLIST_MAX_OBS=10 ** 9), None, lambda: _scene_tables(*C1)),
    "03_c70x400_per_camera_8x8": (FULL, None, lambda: _scene_tables(70, 400, "SIMPLE_RADIAL", False, 70)),
    "04_c40x300_pinhole_shared": (FULL, None, lambda: _scene_tables(40, 300, "SIMPLE_PINHOLE", True, 40)),
    "05_c17x900_three_tiles": (FULL, None, lambda: _scene_tables(17, 900, "SIMPLE_RADIAL", True, 17)),
    "06_c2x30_one_group": (FULL, None, lambda: _scene_tables(2, 30, "SIMPLE_RADIAL", True, 2)),
    "07_bernoulli_33x200_empty_camera": (FULL, None, lambda: _scene_tables(33, 200, "SIMPLE_RADIAL", False, 4,
                                                                          _bernoulli_masks(33, 200, 0.08, 4))),
    "08_case1_two_launches": (dict(FULL, MERGED_TILE_MAX_OBS=0), None, lambda: _scene_tables(*C1)),
    "09_case1_no_top_up": (dict(FULL, TILE_TOP_UP=False), None, lambda: _scene_tables(*C1)),
    "10_case1_dense_first": (dict(FULL, TILE_ORDER="dense_first"), None, lambda: _scene_tables(*C1)),
    "11_case1_stride_through_the_hook": (FULL, {"VGGSFM_AMD_DEBUG_HOOKS": "1", "VGGSFM_TILE_ORDER": "stride"},
                                         lambda: _scene_tables(*C1)),
    "12_direct_40x300_three_batches": ({}, None, _direct_tables),
}


def digest(t):
    """SHA-256 of a table: dtype, shape and the little-endian bytes of the C-contiguous array."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}{list(a.shape)}".encode())
    h.update(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
    return h.hexdigest()


def build_case(name):
    consts, env, fn = CASES[name]
    with settings(env, **consts):
        chunk_desc, entries, tile_desc, obs_slot, nseg, batch_desc = fn()
    out = {k: digest(v) for k, v in zip(TABLES, (chunk_desc, entries, tile_desc, obs_slot, batch_desc))}
    out["num_segments"] = int(nseg)
    # (sizes are recorded to make a mismatch readable; the digests cover them)
    out["shapes"] = {k: list(v.shape) for k, v in zip(TABLES, (chunk_desc, entries, tile_desc, obs_slot, batch_desc))}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    got = {name: build_case(name) for name in CASES}
    if a.check:
        with open(a.out) as f:
            want = json.load(f)["cases"]
        bad = [n for n in CASES if got[n] != want.get(n)]
        print("mismatch: " + ", ".join(bad) if bad else f"{len(CASES)} cases match")
        return 1 if bad else 0
    with open(a.out, "w") as f:
        json.dump({"tables": list(TABLES), "cases": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(got)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
