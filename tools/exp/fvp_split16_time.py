#!/usr/bin/env python
"""fvp_split_kernel (two wavefronts per SIMD, 32-sample tiles) against fvp_split16_kernel (RLLAB_FVP_SPLIT=3: four per
SIMD, 16-sample tiles), interleaved in one process, at the headline batch.  GPU box.

  python tools/exp/fvp_split16_time.py [n_shapes [ablation]]

The timing ablations of fvp_split16_kernel (the tile loop re-uses the first tile's inputs: WRONG results) are a build-time
switch of csrc/policy_split16_kernels.hip, like every RL_ABL_* one: build the library with -DRL_ABL_SPLIT16_FETCH=1 (no fetch of
the cached fragments), 2 (none of the observations / weight) or 3 (neither) and name that value as ``ablation``; the split16
rows are then tagged with it.  This script cannot tell which build it runs."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from tests import test_gpu_update_parity as U

def timed(fn, n=40):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n

for do, da, B in [(13, 2, 2048000), (4, 1, 409600), (13, 2, 8192000)][:int(sys.argv[1]) if len(sys.argv) > 1 else 3]:
    pol = U._policy(do, da, 32)
    ops = pol.fused_ops()
    inp = U._inputs(pol, B, ragged=False, old_equals_new=True)
    v = torch.randn(pol.flat_params.numel(), device="cuda", dtype=torch.float64)
    ops.loss_grad(inp, keep_activations=True)
    out = dict(net=[do, da, 32], B=B)
    abl = {"0": "", "1": "_no_acts_fetch", "2": "_no_x_fetch", "3": "_no_fetch"}[sys.argv[2] if len(sys.argv) > 2 else "0"]
    for rnd in range(3):
        for tag, val, wps in (("split32", "1", "0"), ("split16_wps4" + abl, "3", "4"), ("split16_wps3" + abl, "3", "3")):
            os.environ["RLLAB_FVP_SPLIT"] = val
            os.environ["RLLAB_FVP_SPLIT_WPS"] = wps
            out.setdefault(tag + "_ms", []).append(round(timed(lambda: ops.fvp(inp, v)), 4))
    print(json.dumps(out), flush=True)
