#!/usr/bin/env python
"""Record tests/golden/update_closures.json: per update-batch family of tests/test_update_closures_pins.py, every value
the closures of NPO / VPG / REPS ``init_opt`` return (and their gradients), as ``float.hex()``, computed by the code of
``--parent-commit`` with float64 parameters on the CPU and one thread.  The cases and how they run are the test module's own
(``FAMILIES`` / ``run_family``): the recorder and the test cannot drift apart.

  python tools/make_golden_update_closures.py --parent-commit <40 hex digits> [--out tests/golden/update_closures.json]

Run it ONCE, with the code of the commit BEFORE a change to these closures, and name that commit.  A value that differs
afterwards is a defect of the change, never a reason to run this again."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "update_closures.json"))
    args = ap.parse_args()
    assert len(args.parent_commit) == 40 and int(args.parent_commit, 16) >= 0, "the full commit hash"
    from tests.test_update_closures_pins import FAMILIES, run_family
    res = dict(parent_commit=args.parent_commit, cases={})
    for family in FAMILIES:
        named, plain = run_family(family, False), run_family(family, True)
        assert named == plain, "%s: a plain tuple and what npo_inputs returns give different values" % family
        res["cases"][family] = {k: [float(x).hex() for x in v] for k, v in named.items()}
        print("%s: %s" % (family, " ".join(sorted(named))), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
