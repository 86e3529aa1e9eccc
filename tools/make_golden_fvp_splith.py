#!/usr/bin/env python
"""Record tests/golden/fvp_splith_pins.json: per case of tests/test_gpu_fvp_splith_pins.py the shape, the dtype and a
SHA-256 of the float64 Fisher-vector product, as the library built from ``--parent-commit`` computes it.  The cases and how
they run are the test module's own (``CASES`` / ``run_case``): the recorder and the test cannot drift apart.

  python tools/make_golden_fvp_splith.py --parent-commit <40 hex digits> [--out tests/golden/fvp_splith_pins.json]

Run it ONCE, on a HIP device, with the library of the commit BEFORE a change to csrc/policy_splith_kernels.hip, and name that
commit.  A digest that differs afterwards is a defect of the change, never a reason to run this again."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fvp_splith_pins.json"))
    args = ap.parse_args()
    assert len(args.parent_commit) == 40 and int(args.parent_commit, 16) >= 0, "the full commit hash"
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_fvp_splith.py records on a HIP device; none is visible")
    from tests.test_gpu_fvp_splith_pins import CASES, run_case
    res = dict(parent_commit=args.parent_commit, device=torch.cuda.get_device_name(0), cases={})
    for name in sorted(CASES):
        res["cases"][name] = run_case(name)
        print("%s: %s" % (name, res["cases"][name]["sha256"][:16]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
