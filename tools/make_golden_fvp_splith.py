#!/usr/bin/env python
"""Record the pins of the split-operand Fisher-vector products: per case of tests/test_gpu_fvp_splith_pins.py the shape, the
dtype and a SHA-256 of the float64 product, as the library built from ``--parent-commit`` computes it.  The cases and how
they run are the test module's own (``CASES`` / ``run_case``): the recorder and the test cannot drift apart.

  python tools/make_golden_fvp_splith.py --parent-commit <40 hex digits> [--which splith|split] [--out FILE]

``--which splith`` (the default): the two-way f16 kernels, tests/golden/fvp_splith_pins.json; ``--which split``: the bf16, the
16-sample-tile and the cooperative kernels, tests/golden/fvp_split_pins.json.

Run it ONCE, on a HIP device, with the library of the commit BEFORE a change to the kernels' sources, and name that
commit.  A digest that differs afterwards is a defect of the change, never a reason to run this again.

  python tools/make_golden_fvp_splith.py --parent-commit <40 hex digits> --variant-table

records tests/golden/fvp_variant_table.json instead, the answers of rl_policy_fvp_variant (a host query: no device needed)
over the table of tests/test_fvp_variant_table.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-commit", required=True)
    ap.add_argument("--which", choices=("splith", "split"), default="splith")
    ap.add_argument("--variant-table", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert len(args.parent_commit) == 40 and int(args.parent_commit, 16) >= 0, "the full commit hash"
    if args.variant_table:
        from tests.test_fvp_variant_table import GOLDEN, variant_table
        _write(args.out or GOLDEN, dict(parent_commit=args.parent_commit, table=variant_table()))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_fvp_splith.py records on a HIP device; none is visible")
    from tests.test_gpu_fvp_splith_pins import CASES, GOLDEN, run_case
    res = dict(parent_commit=args.parent_commit, device=torch.cuda.get_device_name(0), cases={})
    for name in sorted(n for n in CASES if CASES[n][0] == args.which):
        res["cases"][name] = run_case(name)
        print("%s: %s" % (name, res["cases"][name]["sha256"][:16]), flush=True)
    _write(args.out or GOLDEN[args.which], res)


if __name__ == "__main__":
    main()
