"""The numpy restatements of the Gauss-Newton family pinned to what they returned before their common parts were merged
(tests/golden/gn_restatement_sums.json, tools/gen_gn_golden.py): the 33 integers of track_ref.linearize and register_ref.linearize, the score fields of
register_search_ref.score, and the final poses of track and register, exactly.  The GPU tests compare the kernels with these restatements; without
this file a rewrite of both could drift together."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_restatements_reproduce_the_recorded_sums():
    import gen_gn_golden as gg
    with open(gg.PATH) as f:
        gold = json.load(f)
    got = json.loads(json.dumps(gg.compute()))
    assert sorted(got) == sorted(gold)
    assert len([k for k in gold if k.startswith("track/") and "stride" in k]) == 7 and len([k for k in gold if k.startswith("register/") and "stride" in k]) == 8
    for k in sorted(gold):
        assert got[k] == gold[k], k
