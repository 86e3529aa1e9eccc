#!/usr/bin/env python
"""Record tests/golden/planes_ops.json: per case of tests/test_gpu_planes_ops_pins.py and per output of the networks-on-planes
update passes (loss sums, gradient, Fisher-vector product, device CG, penalised value and gradient), a SHA-256 of the bytes as
the code of ``--parent-commit`` computes them.  The cases and how they run are the test module's own (``CASES`` /
``run_case``): the recorder and the test cannot drift apart.

Every case runs twice, in two fresh processes.  An output whose digests differ between the two is recorded as unstable,
with the first run's values: the test holds it to the bar of the existing parity test of that quantity, not to a digest.

  python tools/make_golden_planes_ops.py --parent-commit <40 hex digits> [--out tests/golden/planes_ops.json]

Run it ONCE, on a HIP device, with the code of the commit BEFORE a change to these passes, and name that commit.  A digest
that differs afterwards is a defect of the change, never a reason to run this again."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_run(path):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_planes_ops.py records on a HIP device; none is visible")
    from tests.test_gpu_planes_ops_pins import CASES, digest, run_case
    res = {}
    for name in sorted(CASES):
        res[name] = {k: dict(digest(a), values=[float(x).hex() for x in a]) for k, a in run_case(name).items()}
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), cases=res), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "planes_ops.json"))
    ap.add_argument("--one-run", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one_run:
        return one_run(args.one_run)
    assert args.parent_commit and len(args.parent_commit) == 40 and int(args.parent_commit, 16) >= 0, "the full commit hash"
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(2):
            path = os.path.join(tmp, "run%d.json" % i)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--one-run", path], timeout=300)
            with open(path) as f:
                runs.append(json.load(f))
    res = dict(parent_commit=args.parent_commit, device=runs[0]["device"], cases={})
    for name, outs in sorted(runs[0]["cases"].items()):
        res["cases"][name] = {}
        for k, first in sorted(outs.items()):
            stable = first["sha256"] == runs[1]["cases"][name][k]["sha256"]
            res["cases"][name][k] = {f: v for f, v in first.items() if f != "values" or not stable}
            if not stable:
                print("UNSTABLE %s %s" % (name, k), flush=True)
        print("%s: %s" % (name, " ".join(sorted(outs))), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
