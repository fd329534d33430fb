"""Pin the oracle's second solve entry point (pft_or_solve_ex: DELTA_LOCAL, chunk multipliers, a
skip mask and the error norm's arg-max) to the reference's own runs with those inputs
(tests/golden/epsctl, from gen_golden.py's case_epsctl through the harness options --delta, --mult
and --mult-odd-planes), and to pft_or_solve where nothing new is passed."""
import numpy as np
import pytest

import _oracle as O


def epsctl_mult(info, run):
    """chunk multipliers of an epsctl run: None, three per-variable values, or the (q, k, j) table
    with 1 on the even planes and `mult_odd_planes` on the odd ones"""
    if run["mult_odd_planes"] is not None:
        cm = np.ones((3, info["n3"], info["n2"]))
        cm[:, 1::2, :] = run["mult_odd_planes"]
        return cm
    return run["mult"]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_solve_ex_equals_reference(name):
    meta, A = O.load_case("epsctl")
    P, info = O.params_from_meta(meta)
    run = meta["runs"][name]
    t, h, s, st, rc, x, recs = O.solve_ex(info, P, 0, A["ic"], run["t0"], run["h0"], [meta["T"]],
                                          delta_local=run["delta_local"], chunk_mult=epsctl_mult(info, run))[0]
    ref = run["traj"][0]
    assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(),
                                             ref[2], ref[3], ref[4])
    assert np.array_equal(x, A[f"{name}_state0"])
    # the record: every attempted step's arg-max is a cell of the grid that holds that norm
    assert len(recs) == 16 and all(e > 0.0 and 0 <= q < 3 and 0 <= k < info["n3"] and 0 <= j < info["n2"]
                                   and 0 <= i < info["n1"] for e, (q, k, j, i) in recs)


def test_epsctl_runs_differ_from_the_default():
    """the four runs are not the g20 trajectory: the options reached the reference's decision"""
    meta, _ = O.load_case("epsctl")
    g20, _ = O.load_case("g20")
    base = tuple(g20["traj_m0"][0][:4])
    rows = [tuple(r["traj"][0][:4]) for r in meta["runs"].values()]
    assert base not in rows and len(set(rows)) == 4


def test_solve_ex_without_new_arguments_is_solve():
    meta, A = O.load_case("g20")
    P, info = O.params_from_meta(meta)
    a = O.solve(info, P, 0, A["traj_m0_ic"], 0.0, 1.0, meta["traj_times"])
    b = O.solve_ex(info, P, 0, A["traj_m0_ic"], 0.0, 1.0, meta["traj_times"])
    for (t, h, s, st, rc, x), rb, ref, i in zip(a, b, meta["traj_m0"], range(len(a))):
        assert (t.hex(), h.hex(), s, st, rc) == (rb[0].hex(), rb[1].hex(), rb[2], rb[3], rb[4])
        assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(),
                                                 ref[2], ref[3], ref[4])
        assert np.array_equal(x, rb[5]) and np.array_equal(x, A[f"traj_m0_state{i}"])


def test_skip_mask_and_argmax():
    """a mask of zeros changes nothing; skipping the arg-max cell takes it out of the maximum itself
    (a mask that hid the cell from the arg-max scan only would leave the norm and h as they were)"""
    meta, A = O.load_case("g20")
    P, info = O.params_from_meta(meta)
    ic = A["traj_m0_ic"]
    base = O.solve_ex(info, P, 0, ic, 0.0, 1.0, [1e9], max_steps_total=3)[0]
    zero = np.zeros(ic.shape, dtype=np.uint8)
    same = O.solve_ex(info, P, 0, ic, 0.0, 1.0, [1e9], max_steps_total=3, skip=zero)[0]
    assert base[:5] == same[:5] and np.array_equal(base[5], same[5]) and base[6] == same[6]
    # on the g20 initial condition mirror-image cells tie for the maximum: skipping one moves the
    # arg-max to another and leaves the norm
    e0, (q, k, j, i) = base[6][0]
    zero[q, k, j, i] = 1
    cut = O.solve_ex(info, P, 0, ic, 0.0, 1.0, [1e9], max_steps_total=3, skip=zero)[0]
    assert cut[6][0][0] <= e0 and cut[6][0][1] != (q, k, j, i)
    # a state whose maximum one cell holds alone: u = top_temp1, p = 1 at that cell, else 0
    # (on 40 x 20 x 7 over g20's domain, where the issue worked the probe out)
    tgt = (3, 10, 20)
    info = dict(info, n1=40, n2=20, n3=7)
    x = np.zeros((3, 7, 20, 40))
    x[0] = P[O.PARAM_NAMES.index("top_temp1")]
    x[1][tgt] = 1.0
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[(slice(None),) + tgt] = 1
    one = O.solve_ex(info, P, 0, x, 0.0, 1.0, [1e9], max_steps_total=1)[0]
    cut = O.solve_ex(info, P, 0, x, 0.0, 1.0, [1e9], max_steps_total=1, skip=mask)[0]
    assert one[6][0][1][1:] == tgt
    assert cut[6][0][0] < one[6][0][0] and cut[6][0][1][1:] != tgt
    assert cut[1] != one[1]
