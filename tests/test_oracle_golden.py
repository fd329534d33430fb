"""Pin the CPU oracle (oracle/pft_oracle.c) to the reference's own outputs, bit for bit.

Golden vectors come from the reference compiled in place (tests/golden/gen_golden.py).
"""
import numpy as np
import pytest

import _dense as D
import _oracle as O


@pytest.fixture(scope="module")
def g20():
    return O.load_case("g20")


@pytest.fixture(scope="module")
def ragged():
    return O.load_case("ragged")


def test_float_val_matches_reference_params(g20):
    meta, _ = g20
    _, info = O.params_from_meta(meta)
    fv = O.lib().pft_or_float_val
    # Params:130 "tau_min 1e-6" is NOT the correctly rounded 1e-6 in the reference
    assert fv(b"1e-6") == info["tau_min"]
    assert fv(b"1e-6") != 1e-6
    assert fv(b"1e-3") == info["delta"]
    assert fv(b"0.03") == info["L1"]


def test_ic_default_bitwise(g20):
    meta, A = g20
    P, info = O.params_from_meta(meta)
    ic = O.ic_default(info, P, O.beads())
    assert np.array_equal(ic, A["ic"])


def test_ic_default_slabs_bitwise(g20):
    meta, A = g20
    P, info = O.params_from_meta(meta)
    parts = [O.ic_default(info, P, O.beads(), 3, r) for r in range(3)]
    assert np.array_equal(np.concatenate(parts, axis=1), A["ic"])


@pytest.mark.parametrize("mode", [0, 1, 2, 10, 11])
@pytest.mark.parametrize("tag", ["t0", "t1"])
def test_rhs_g20_bitwise(g20, mode, tag):
    meta, A = g20
    P, info = O.params_from_meta(meta)
    K, _ = O.rhs(info, P, mode, meta["rhs_times"][tag], A["ic"])
    assert np.array_equal(K, A[f"rhs_m{mode}_{tag}"])


@pytest.mark.parametrize("mode", [0, 1, 2, 10, 11])
@pytest.mark.parametrize("tag", ["t0", "t1"])
@pytest.mark.parametrize("nprocs", [1, 4])
def test_rhs_ragged_bitwise(ragged, mode, tag, nprocs):
    meta, A = ragged
    P, info = O.params_from_meta(meta)
    K, _ = O.rhs(info, P, mode, meta["rhs_times"][tag], A["state"], nprocs)
    assert np.array_equal(K, A[f"rhs_m{mode}_{tag}"])


@pytest.mark.parametrize("tag", ["t0", "t1"])
def test_boundary_kat(ragged, tag):
    """every rank's padded input after bcond_setup + sync_solution (equation.c:266-326)"""
    meta, A = ragged
    P, info = O.params_from_meta(meta)
    _, ws = O.rhs(info, P, 0, meta["rhs_times"][tag], A["state"], 4)
    for r in range(4):
        ref = A[f"w4_{tag}_rank{r}"].reshape(ws[r].shape)
        assert np.array_equal(ws[r], ref), r
    _, ws1 = O.rhs(info, P, 0, meta["rhs_times"][tag], A["state"], 1)
    assert np.array_equal(ws1[0], A[f"w1_{tag}_rank0"].reshape(ws1[0].shape))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_trajectory_bitwise(g20, mode):
    meta, A = g20
    P, info = O.params_from_meta(meta)
    res = O.solve(info, P, mode, A[f"traj_m{mode}_ic"], 0.0, 1.0, meta["traj_times"])
    for i, (t, h, s, st, rc, x) in enumerate(res):
        ref = meta[f"traj_m{mode}"][i]
        assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(),
                                                 ref[2], ref[3], ref[4])
        assert np.array_equal(x, A[f"traj_m{mode}_state{i}"])


@pytest.mark.parametrize("tag", ["small", "large"])
def test_single_step_bitwise(ragged, tag):
    meta, A = ragged
    P, info = O.params_from_meta(meta)
    m = meta[f"step_{tag}"]
    (t, h, s, st, rc, x), = O.solve(info, P, 0, A["state"], m["t0"], m["h0"], [m["T"]])
    r = m["result"]
    assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(r[0]).hex(), float.fromhex(r[1]).hex(), r[2], r[3], r[4])
    assert np.array_equal(x, A[f"step_{tag}"])


@pytest.mark.parametrize("mode", [10, 11])
def test_trajectory_no_flux_modes_bitwise(mode):
    """calc_mode 10 and 11 (no heat-flux term, du = 0): the oracle's trajectory to the g20 snapshot
    times equals the reference's own (tests/golden/g20nf, from gen_golden.py)"""
    meta, A = O.load_case("g20nf")
    P, info = O.params_from_meta({"params": meta[f"m{mode}_params"]})
    assert info["calc_mode"] == mode
    res = O.solve(info, P, mode, A[f"traj_m{mode}_ic"], 0.0, 1.0, meta["traj_times"])
    for i, (t, h, s, st, rc, x) in enumerate(res):
        ref = meta[f"traj_m{mode}"][i]
        assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(),
                                                 ref[2], ref[3], ref[4])
        assert np.array_equal(x, A[f"traj_m{mode}_state{i}"])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_trajectory_across_the_phase_switch_bitwise(mode):
    """tests/golden/gthaw: g20 with phase_switch_time = 100 s, so the top temperature jumps from
    top_temp1 to top_temp2 (equation.c:96-111,175-183) between the first two snapshot times.  The
    attempted steps that straddle the switch (each stage decides at its own time), the rejections
    after the 45 K jump and the thaw that follows equal the reference's, and the ice does melt"""
    meta, A = O.load_case("gthaw")
    P, info = O.params_from_meta(meta)
    assert P[O.PARAM_NAMES.index("phase_switch_time")] == meta["phase_switch_time"] == 100.0
    res = O.solve(info, P, mode, A[f"traj_m{mode}_ic"], 0.0, 1.0, meta["traj_times"])
    for i, (t, h, s, st, rc, x) in enumerate(res):
        ref = meta[f"traj_m{mode}"][i]
        assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(),
                                                 ref[2], ref[3], ref[4])
        assert np.array_equal(x, A[f"traj_m{mode}_state{i}"])
    # the switch is seen: the freeze (tests/golden/g20) has other states from t = 360 s on
    g20 = O.load_case("g20")[1]
    assert np.array_equal(A[f"traj_m{mode}_ic"], g20[f"traj_m{mode}_ic"])
    assert np.array_equal(A[f"traj_m{mode}_state0"], g20[f"traj_m{mode}_state0"])
    assert not np.array_equal(A[f"traj_m{mode}_state1"], g20[f"traj_m{mode}_state1"])
    if mode == 0:
        ice = [int((A[f"traj_m0_state{i}"][1] > 0.5).sum()) for i in range(3)]
        assert ice[0] > ice[2] > 0, ice


# ---- u_noise (tests/golden/gnoise: the reference with u_noise_amp = 0.5 K on one rank) ----------

def test_noise_field_is_glibc_rand_from_seed_1():
    """the reference's noise field (equation.c:450-456, rand() never seeded by the harness) is
    amp (rand()/RAND_MAX - 0.5) of glibc's sequence from seed 1, node by node in [k][j][i] order --
    what libpft draws after srand(1) (intertrack_model.c PrecalculateData)"""
    meta, A = O.load_case("gnoise")
    noise = O.glibc_noise(meta["u_noise_amp"], A["noise"].size)
    assert np.abs(A["noise"]).max() > 0.2
    assert np.array_equal(noise.reshape(A["noise"].shape), A["noise"])


@pytest.mark.parametrize("mode", [0, 10, 1, 11])
def test_noise_rhs_equals_reference(mode):
    """the four models that add u_noise to u in their reaction term (equation.c:676, 687), at a
    state with mixed phases"""
    meta, A = O.load_case("gnoise")
    P, info = O.params_from_meta({"params": meta[f"m{mode}_params"]})
    assert info["calc_mode"] == mode and P[O.PARAM_NAMES.index("u_noise_amp")] == meta["u_noise_amp"]
    x, t = A[meta["rhs_state"]], meta["rhs_time"]
    K, _ = O.rhs(info, P, mode, t, x, noise=A["noise"])
    assert np.array_equal(K, A[f"rhs_m{mode}"])
    K0, _ = O.rhs(info, P, mode, t, x)
    assert not np.array_equal(K0, A[f"rhs_m{mode}"])        # the noise is seen


@pytest.mark.parametrize("mode", [0, 1])
def test_noise_trajectory_equals_reference(mode):
    meta, A = O.load_case("gnoise")
    P, info = O.params_from_meta({"params": meta[f"m{mode}_params"]})
    res = O.solve(info, P, mode, A["ic"], 0.0, 1.0, meta["traj_times"], noise=A["noise"])
    for i, (t, h, s, st, rc, x) in enumerate(res):
        ref = meta[f"traj_m{mode}"][i]
        assert (t.hex(), h.hex(), s, st, rc) == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(),
                                                 ref[2], ref[3], ref[4])
        assert np.array_equal(x, A[f"traj_m{mode}_state{i}"])


# ---- dense edge-value states (tests/_dense.py; tests/golden/gedge and gedgep) --------------------
# The oracle is pinned on the clamp and threshold branches and on foreign constants before the
# device is compared with it (tests/test_dense_gpu.py), and the inputs of those comparisons are
# shown to be what they are meant to be: dense, and on every branch.

GEDGE = [("gedge", m) for m in D.MODES] + [("gedgep", m) for m in D.MODES]
GEDGE_TRAJ = [("gedge", m) for m in D.MODES] + [("gedgep", 0), ("gedgep", 1)]
DENSE_INPUTS = [("gedge", None), ("gedgep", None)] + [(d, pert) for d in D.GRIDS for pert in (False, True)]


def _dense_input(case, perturbed):
    if perturbed is None:
        meta, A, Pm, info = D.golden(case)
        return info, Pm, A["state"]
    return D.grid_case(case, perturbed)


def test_gedge_is_the_generator_state():
    """the golden's state is edge_state() of the reference's own parameter values, and the perturbed
    set differs from the default one in every physical constant"""
    for name in ("gedge", "gedgep"):
        meta, A, Pm, info = D.golden(name)
        assert (info["n1"], info["n2"], info["n3"]) == (44, 24, 6)
        assert np.array_equal(A["state"], D.edge_state(44, 24, 6, Pm, meta["state_seed"]))
    P0, Pp = D.golden("gedge")[2], D.golden("gedgep")[2]
    for k in D.PHYSICAL + list(D.FIXED):
        assert P0[D.PARAM_NAMES.index(k)] != Pp[D.PARAM_NAMES.index(k)], k
    for k, v in D.FIXED.items():
        assert Pp[D.PARAM_NAMES.index(k)] == O.lib().pft_or_float_val(repr(v).encode())


@pytest.mark.parametrize("case,mode", GEDGE)
@pytest.mark.parametrize("nprocs", [1, 3])
def test_rhs_gedge_bitwise(case, mode, nprocs):
    meta, A, Pm, info = D.golden(case)
    K, _ = O.rhs(info, Pm, mode, meta["rhs_time"], np.array(A["state"]), nprocs)
    assert np.array_equal(K, D.golden_rhs(A, mode))


@pytest.mark.parametrize("case,mode", GEDGE_TRAJ)
def test_six_steps_gedge_bitwise(case, mode):
    """the reference's first six attempted steps from h = 1 s: at least one rejected, two accepted"""
    meta, A, Pm, info = D.golden(case)
    t, h, steps, total, rc, x = O.solve(info, Pm, mode, np.array(A["state"]), 0.0, 1.0, [1e9],
                                        max_steps_total=meta["attempts"])[0]
    assert (t.hex(), h.hex(), steps, total, rc) == D.golden_record(meta, mode) + (2,)
    assert np.array_equal(x, D.golden_final(A, mode))
    assert total == D.ATTEMPTS and steps >= 2 and total - steps >= 1 and np.isfinite(x).all()


@pytest.mark.parametrize("case,perturbed", DENSE_INPUTS)
def test_dense_state_has_no_trivial_cell(case, perturbed):
    """K_u != 0 at every cell in modes 0, 1 and 2; K_p != 0 at >= 99% of the cells with
    1 - zeta gl > 0 in modes 0, 1, 10 and 11 (elsewhere the factor fmax(0, 1 - zeta gl) makes it 0)"""
    info, Pm, x = _dense_input(case, perturbed)
    wet = 1.0 - Pm[O.PARAM_NAMES.index("zeta")] * x[2] > 0
    for mode in D.MODES:
        K, _ = O.rhs(info, Pm, mode, 100.0, np.array(x))
        assert np.isfinite(K).all()
        if mode in (0, 1, 2):
            assert np.count_nonzero(K[0]) == K[0].size, mode
        if mode in (0, 1, 10, 11):
            assert np.count_nonzero(K[1][wet]) >= 0.99 * wet.sum(), mode
            assert not K[1][~wet].any()


@pytest.mark.parametrize("case,perturbed", DENSE_INPUTS)
def test_dense_state_populates_every_branch(case, perturbed):
    """more than 1% of the cells on each branch of the arithmetic: p < 0 and p > 1 (fmax(p(1-p), 0)
    clamps), the three pieces of sshape for p and for 1 - p, both sides of fmax(0, 1 - zeta gl),
    u = u_star; and the threshold values themselves are there"""
    info, Pm, x = _dense_input(case, perturbed)
    for k, v in D.branch_fractions(x, Pm).items():
        assert v > 0.01, (k, v)
    for v in D.p_specials(Pm):
        assert (x[1] == v).sum() > 0, v
    for v in D.gl_specials(Pm):
        assert (x[2] == v).sum() > 0, v


@pytest.mark.parametrize("dims", D.GRIDS)
@pytest.mark.parametrize("perturbed", [False, True])
def test_dense_grids_six_steps_are_finite(dims, perturbed):
    """the oracle's six attempted steps from h = 1 s on the larger grids: finite, steps of both kinds"""
    for mode in D.MODES:
        (t, h, steps, total), x = D.oracle_steps(dims, perturbed, mode)
        assert total == D.ATTEMPTS and 1 <= steps < total and np.isfinite(x).all(), (mode, steps)
