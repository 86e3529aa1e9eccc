#!/usr/bin/env python
"""Two built trees of this repository timed against each other on one box, interleaved: the headline bench and whole TRPO
iterations of the two networks-on-planes policies (tools/exp/planes_update_time.py).  Written for a change to the host side
of the update, where what can get slower is the time between launches.

  python tools/exp/update_batch_refactor_ab.py --parent DIR [--new DIR] [--pairs 4] --out profiles/update_batch_refactor_time.json

Per pair: one run of each tree, each a fresh process; which tree goes first alternates from pair to pair (the host-bound
iterations of the second run of a pair came out 0.03-0.06 ms slower than the first whichever tree it was).  Per quantity:
every run, the two medians, the parent's own min-max spread over its runs -- that spread is the measurement's resolution --
and ``within``: the new median is not worse than the parent's by more than that spread.  Neither tree is built here: build
both first."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# quantity -> lower is better?
QUANTITIES = dict(bench_env_steps_per_s=False, bench_update_phase_ms=True, adaptive_std_iteration_ms=True,
                  adaptive_std_update_ms=True, categorical_iteration_ms=True, categorical_update_ms=True)


def one_side(root, steps, warmup):
    bench = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                           cwd=root, check=True, stdout=subprocess.PIPE, text=True, timeout=400).stdout
    line = json.loads([l for l in bench.splitlines() if l.startswith("{")][-1])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "planes.json")
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "exp", "planes_update_time.py"), "--root", root,
                        "--out", out], cwd=root, check=True, timeout=400)
        with open(out) as f:
            planes = json.load(f)
    return dict(bench_env_steps_per_s=line["value"], bench_update_phase_ms=line["phase_ms"]["update"],
                adaptive_std_iteration_ms=planes["adaptive_std"]["iteration_median_ms"],
                adaptive_std_update_ms=planes["adaptive_std"]["update_median_ms"],
                categorical_iteration_ms=planes["categorical"]["iteration_median_ms"],
                categorical_update_ms=planes["categorical"]["update_median_ms"]), planes["device"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=HERE)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    runs = dict(parent=[], new=[])
    for pair in range(args.pairs):
        sides = (("parent", os.path.abspath(args.parent)), ("new", os.path.abspath(args.new)))
        for side, root in (sides[::-1] if pair % 2 else sides):
            r, device = one_side(root, args.steps, args.warmup)
            runs[side].append(r)
            print("pair %d %-6s %s" % (pair, side, json.dumps(r, sort_keys=True)), flush=True)
    res = dict(device=device, pairs=args.pairs, order="parent first in even pairs, new first in odd ones",
               bench="bench.py --gpus 1 --steps %d --warmup %d" % (args.steps, args.warmup),
               planes="tools/exp/planes_update_time.py (median of 15 iterations after 3 per run)", quantities={})
    for q, lower_is_better in QUANTITIES.items():
        p, n = np.array([r[q] for r in runs["parent"]]), np.array([r[q] for r in runs["new"]])
        spread = float(p.max() - p.min())
        worse_by = float(np.median(n) - np.median(p)) * (1.0 if lower_is_better else -1.0)
        res["quantities"][q] = dict(parent_runs=p.tolist(), new_runs=n.tolist(), parent_median=float(np.median(p)),
                                    new_median=float(np.median(n)), parent_spread=spread, new_worse_by=worse_by,
                                    lower_is_better=lower_is_better, within=bool(worse_by <= spread))
        print("%-28s parent %.4f new %.4f spread %.4f within %s" % (q, np.median(p), np.median(n), spread, worse_by <= spread))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
