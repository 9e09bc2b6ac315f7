"""The Schur work list, table for table: vggsfm_amd.ba.build_schur_tiles against digests recorded from the builder before it was
cut into stages (scripts/make_golden_worklist.py, tests/golden/schur_worklist.json).  test_host_logic.py checks the
invariants of a work list; this pins the tables themselves -- chunk_desc, entries, tile_desc, obs_slot, batch_desc and the
number of segments -- on the paths the builder can take: full and simple list, 6 x 6 and 8 x 8 blocks, one and two camera
groups, a camera without observations, one and two launches, with and without top-up, three launch orders, three batches."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_golden_worklist", os.path.join(ROOT, "scripts", "make_golden_worklist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_generator()
with open(GEN.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_holds_every_case_and_table():
    assert tuple(GOLDEN["tables"]) == GEN.TABLES
    assert sorted(GOLDEN["cases"]) == sorted(GEN.CASES) and len(GEN.CASES) == 12
    for rec in GOLDEN["cases"].values():
        assert set(rec) == set(GEN.TABLES) | {"num_segments", "shapes"}


@pytest.mark.parametrize("name", sorted(GEN.CASES))
def test_work_list_tables_match_the_recorded_digests(name):
    got, want = GEN.build_case(name), GOLDEN["cases"][name]
    assert got["num_segments"] == want["num_segments"]
    assert got["shapes"] == want["shapes"]
    for table in GEN.TABLES:
        assert got[table] == want[table], f"{name}: {table} differs from the recorded table"
