#!/usr/bin/env python
"""Record tests/golden/swimmer_perp_operands.json: the digests of every output plane of the cases of
tests/test_gpu_swimmer_perp_operands.py.  Run on the GPU with the kernels whose bits are to be kept (the library as it
was before the change under test):   python tools/make_golden_swimmer_perp_operands.py [file]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_gpu_swimmer_perp_operands as T  # noqa: E402

if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for c in T.CASES:
        _, kernel, out = T.run_case(*c)
        rec[T.case_id(*c)] = T.digests(out)
        print("%s: kernel %d" % (T.case_id(*c), kernel))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases -> %s" % (len(rec), path))
