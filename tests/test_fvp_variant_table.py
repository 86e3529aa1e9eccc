"""Which Fisher-vector-product kernel rl_policy_fvp launches, as data (host logic, no GPU): rl_policy_fvp_variant over the cross
product of shapes, rl_launch_opts.fvp_split / fvp_split_wps, the optional pointers and a whole / ragged tile count, against
tests/golden/fvp_variant_table.json -- recorded (tools/make_golden_fvp_splith.py --variant-table) with the library of the
commit the file names, BEFORE the query and the dispatch chain of csrc/policy_kernels.hip came to walk one ordered list."""
import ctypes
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fvp_variant_table.json")

# every shape of RL_NARROW_NETS (csrc/policy_kernels.hip), two cooperative shapes, one no split kernel is built for
SHAPES = [(do, da, (h, h, 0)) for h, pairs in ((32, [(4, 1), (6, 1), (11, 1), (13, 2), (20, 3), (20, 6), (21, 6)]),
                                               (64, [(4, 1), (6, 1), (11, 1), (13, 2), (20, 3), (20, 6), (21, 6)]),
                                               (32, [(13, 1), (20, 1), (21, 1)])) for do, da in pairs]
SHAPES += [(20, 6, (128, 128, 0)), (20, 6, (128, 64, 32)), (20, 6, (48, 48, 0))]


def variant_table():
    """{"do,da,h0,h1,h2|fvp_split|fvp_split_wps|obs_absmax|activations|n_samples": variant} of the loaded library."""
    from rllab_amd import _lib
    table = {}
    opts = _lib.LaunchOpts()
    for do, da, hid in SHAPES:
        for split in range(6):
            for wps in (0, 1, 4):
                for absmax in (1, 0):
                    for acts in (1, 0):
                        for B in (64, 48):
                            opts.fvp_split, opts.fvp_split_wps = split, wps
                            # (the query reads the pointers for being set only)
                            b = _lib.PolicyBatch(n_samples=B, obs_dim=do, act_dim=da, hidden0=hid[0], hidden1=hid[1],
                                                 hidden2=hid[2], activation=_lib.ACT_TANH, opts=ctypes.addressof(opts),
                                                 activations=256 if acts else None, obs_absmax=256 if absmax else None)
                            key = "%d,%d,%d,%d,%d|%d|%d|%d|%d|%d" % ((do, da) + hid + (split, wps, absmax, acts, B))
                            table[key] = int(_lib.lib.rl_policy_fvp_variant(ctypes.byref(b)))
    return table


def test_the_choice_of_the_fvp_kernel_is_the_recorded_one():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40
    got = variant_table()
    assert sorted(got) == sorted(g["table"]) and len(got) == len(SHAPES) * 6 * 3 * 2 * 2 * 2
    assert set(got.values()) == {0, 1, 2, 3, 4}                     # (every kernel family is in the table)
    diff = {k: (got[k], g["table"][k]) for k in got if got[k] != g["table"][k]}
    assert not diff, diff
