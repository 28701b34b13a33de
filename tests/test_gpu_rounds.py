"""How a round of nets goes out, held against a table (csrc/net_rounds.hip launch_round).

The generic launch sequence sends the nets of one pass — twin critics, TQC's five quantile critics, REDQ's ensemble — as ONE
k_mlp_slice_tp2 launch, ONE layer-by-layer sequence or multi launch, pairs, or a fork / join over the side streams.  Losing a
grouping changes no bit of any result: twin critics as two launches pass every numeric test.  What it changes is the number
of launches, which oprl_profile_read counts per kind.  tests/golden/round_counts.json (tools/round_counts.py, MI355X) holds
the counts of K = 4 updates at S = 17, A = 6, B = 64 for every case; kinds 0 (the net passes), 1 (dW + Adam) and 3 (everything
else) are compared.  Reference: none (the reference has one path, autograd)."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TABLE = json.loads((ROOT / "tests" / "golden" / "round_counts.json").read_text())
WANT = {r["id"]: r["counts"] for r in TABLE["rows"]}
COMPARED = (0, 1, 3)


def _round_counts():
    spec = importlib.util.spec_from_file_location("round_counts", ROOT / "tools" / "round_counts.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RC = _round_counts()


def test_the_table_holds_every_case():
    assert sorted(WANT) == sorted(c[0] for c in RC.CASES)
    assert TABLE["shape"] == dict(S=RC.S, A=RC.A, B=RC.B, K=RC.K)


@pytest.mark.parametrize("case", RC.CASES, ids=[c[0] for c in RC.CASES])
def test_launch_counts_match_the_table(case, monkeypatch):
    import torch as t
    if t.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table is for a 256-compute-unit MI355X")
    for k in RC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case[3].items():
        monkeypatch.setenv(k, v)
    got, _ = RC.run_case(case)          # (profiling is switched off again in its `finally`)
    want = WANT[case[0]]
    print(case[0], "launches per kind:", got, "table:", want)
    diff = {kind: (got[kind], want[kind]) for kind in COMPARED if got[kind] != want[kind]}
    assert not diff, f"{case[0]}: (got, table) per kind {diff}"
