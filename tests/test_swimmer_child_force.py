"""`substep_quad` (dyn_swimmer_chain.h) forms the force on the subtree behind a body's child joint as the CHILD's value of
`g = F + qp<SHL1>(F)` (every lane adds its child's force to its own) instead of adding two lane moves of F.  Body 0 then
reads F_1 + F_2 and body 1 reads F_2 + (the zero lane's force): the operands and the order of `Fsx[1]`, `Fsx[2]` in
`substep_scalar`.  The four-lane host emulation must still equal the scalar program bit for bit -- also where the sums
meet signed zeros: at rest every body force is +-0.0 (both signs occur over the quadrants of the body angles, and
-0.0 + +0.0 depends on nothing but the operands), with one body moving the others' forces stay zeros, and hinges beyond
their limits switch the penalty torque on."""
import numpy as np
import pytest

from oracle import host_env as H


def _states():
    rng = np.random.default_rng(23)
    out = []
    for root in [-2.6, -0.3, 1.3, np.pi]:                                   # one body angle per quadrant
        for j1, j2 in [(0.0, 0.0), (1.9, -1.9), (-0.0, 2.2)]:               # limit: 100 deg = 1.745
            # at rest: every fluid force is a signed zero
            out.append(np.array([0.1, -0.2, root, j1, j2, 0, 0, 0, 0, 0], dtype=np.float64))
            # negative zeros as the rates themselves
            out.append(np.array([0.1, -0.2, root, j1, j2, -0.0, -0.0, -0.0, -0.0, -0.0], dtype=np.float64))
            # one joint moving, root at rest / the root sliding along one axis only
            out.append(np.array([0.0, 0.0, root, j1, j2, 0, 0, 0, 0, rng.normal(0, 3.0)], dtype=np.float64))
            out.append(np.array([0.0, 0.0, root, j1, j2, rng.normal(0, 1.0), -0.0, 0, 0, 0], dtype=np.float64))
            # everything moving, hinges beyond their limits
            out.append(np.concatenate([rng.normal(0, 1.0, 2), [root, j1, j2], rng.normal(0, 3.0, 5)]))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nsub,every", [(1, 1), (2, 1), (50, 13)])
def test_child_subtree_force_of_the_lane_program_is_bitwise_the_scalar_program(dtype, nsub, every):
    """one and two sub-steps from every state (the second starts from the zeros the first left); a whole env-step of 50
    from every 13th (one of each kind: the emulator replays a sub-step once per exchange point)"""
    ctrls = [np.array([0.0, 0.0, 0.0]), np.array([0.0, -0.0, 1.0]), np.array([0.0, -1.0, 0.37])]
    for k, state in list(enumerate(_states()))[::every]:
        a, b = H.swim_quad_compare(state, ctrls[k % 3], nsub, dtype)
        assert np.all(np.isfinite(a)), (k, state)
        assert a.tobytes() == b.tobytes(), (k, state, a, b)
