"""Dense edge-value states and perturbed parameter sets: plain numpy, fixed seeds.

Shared by the golden generator (tests/golden/gen_golden.py, case gedge) and the tests.  A state
from edge_state() differs from cell to cell, so no cell of it has a constant neighbourhood, and it
puts cells on every branch of the right-hand side's arithmetic: p below 0 and above 1 (where
fmax(p(1-p), 0) clamps), p on and one double either side of sshape's thresholds (equation.c:375-382),
gl on and one double either side of 1/zeta (where fmax(0, 1 - zeta gl) clamps), u on u_star.
"""
import numpy as np

PARAM_NAMES = [  # model.c:44-59, as tests/_oracle.py
    "u_star", "L", "xi", "a", "b", "alpha", "mu",
    "beads_scaling", "beads_offset_x", "beads_offset_y", "beads_offset_z",
    "xi_gl", "zeta", "p_eps0", "p_eps1", "gamma",
    "water_cp", "ice_cp", "glass_cp", "water_lambda", "ice_lambda", "glass_lambda",
    "water_rho", "ice_rho", "glass_rho", "top_temp1", "top_temp2", "phase_switch_time",
    "u_noise_amp", "ball_radius",
]
# the physical constants perturbed_params() scales; alpha is derived from two of them in the
# parameter file (alpha = water_rho * water_cp), so the golden generator leaves it to that formula
PHYSICAL = ["L", "xi", "a", "b", "alpha", "mu", "zeta", "gamma", "water_cp", "ice_cp", "glass_cp",
            "water_lambda", "ice_lambda", "glass_lambda", "water_rho", "ice_rho", "glass_rho"]
FIXED = {"p_eps0": 0.08, "p_eps1": 0.31, "u_star": 271.9}

SEED = 5            # the state seed of the golden case and of every test grid
PERTURB_SEED = 11   # the parameter seed of the golden case and of every test grid

U_EXACT, P_SPECIAL, GL_SPECIAL = 0.05, 0.15, 0.15     # fractions of cells given a special value


def _idx(name):
    return PARAM_NAMES.index(name)


def p_specials(Pm):
    e0, e1 = float(Pm[_idx("p_eps0")]), float(Pm[_idx("p_eps1")])
    return np.array([0.0, e0, np.nextafter(e0, np.inf), e1, np.nextafter(e1, -np.inf), 1.0 - e0, 1.0 - e1,
                     0.5, 1.0, np.nextafter(1.0, np.inf)])


def gl_specials(Pm):
    z = 1.0 / float(Pm[_idx("zeta")])
    return np.array([0.0, 1.0, z, np.nextafter(z, -np.inf), np.nextafter(z, np.inf)])


def edge_state(n1, n2, n3, Pm, seed=SEED):
    """[3][n3][n2][n1] float64: u = u_star + U(-20, 20) with 5% of the cells u_star exactly;
    p = U(-0.1, 1.1) with 15% of the cells from p_specials(); gl = U(0, 1), unsmoothed, with 15% of
    the cells from gl_specials().  No -0.0 anywhere."""
    rng = np.random.default_rng(seed)
    shape = (n3, n2, n1)
    u_star = float(Pm[_idx("u_star")])
    u = u_star + rng.uniform(-20.0, 20.0, size=shape)
    u[rng.random(shape) < U_EXACT] = u_star
    p = rng.uniform(-0.1, 1.1, size=shape)
    m = rng.random(shape) < P_SPECIAL
    sp = p_specials(Pm)
    p[m] = sp[rng.integers(0, sp.size, size=int(m.sum()))]
    gl = rng.uniform(0.0, 1.0, size=shape)
    m = rng.random(shape) < GL_SPECIAL
    sg = gl_specials(Pm)
    gl[m] = sg[rng.integers(0, sg.size, size=int(m.sum()))]
    x = np.ascontiguousarray(np.stack([u, p, gl]), dtype=np.float64)
    assert not np.signbit(x[2]).any()
    return x


def factors(seed=PERTURB_SEED):
    """{name: 1 + U(-0.3, 0.3)} for the PHYSICAL constants, independent, rounded to four decimals so
    that the parameter file's text holds them exactly as written"""
    rng = np.random.default_rng(seed)
    return {k: round(1.0 + float(rng.uniform(-0.3, 0.3)), 4) for k in PHYSICAL}


def perturbed_params(Pm, seed=PERTURB_SEED):
    """param[] with every physical constant times its own 1 + U(-0.3, 0.3) (alpha too: independent of
    water_rho * water_cp), p_eps0 = 0.08, p_eps1 = 0.31, u_star = 271.9; top_temp1/2,
    phase_switch_time, u_noise_amp and the bead geometry left alone"""
    out = np.array(Pm, dtype=np.float64, copy=True)
    for k, f in factors(seed).items():
        out[_idx(k)] *= f
    for k, v in FIXED.items():
        out[_idx(k)] = v
    return out


MODES = (0, 1, 2, 10, 11)
ATTEMPTS = 6
# the grids beside the golden one, with the default Params' domain (0.03 x 0.03 x 0.06 m, so
# h1 != h2 != h3).  Tiles (cells, pair_geometry and fused_geometry): 66 x 38: 2 x 2 pair tiles of
# 34 x 19, the automatic fused tile one wide (66 x 7), 3 x 3 fused16 tiles (32 x 16), 2 x 5 fused32
# tiles (64 x 8); 130 x 70: 7 x 2 pair tiles of 20 x 35, 2 x 10 automatic fused tiles; 120 x 60: the
# 40 x 20 pair tile 3 x 3 times and the automatic fused tile (42 x 12) 3 x 5 times, each with an
# interior tile.  The golden grid, 44 x 24: 3 pair tiles of 16 x 24, 2 x 2 fused16 tiles, 1 x 3
# fused32 tiles; its "default" flavour is the cache kernel, on the grids here the automatic fused one.
# The last three: the golden grid's plane, 5, 6 and 7 planes (tests/test_zplan_gpu.py).
GRIDS = [(66, 38, 7), (130, 70, 5), (120, 60, 6), (44, 24, 5), (44, 24, 6), (44, 24, 7)]

_cache = {}


def golden(name):
    """(meta, arrays, Pm, info) of tests/golden/gedge or gedgep, loaded once"""
    import _oracle as O
    if name not in _cache:
        meta, A = O.load_case(name)
        Pm, info = O.params_from_meta(meta)
        for a in A.values():
            a.setflags(write=False)
        _cache[name] = (meta, A, Pm, info)
    return _cache[name]


def golden_rhs(A, mode):
    """the golden's K [3][n3][n2][n1]: dgl, 0 everywhere, is not stored"""
    K = A[f"rhs_m{mode}"]
    return np.concatenate([K, np.zeros_like(K[:1])])


def golden_final(A, mode):
    """the golden's state after the six attempted steps: a component the run left as it was (gl
    always, u in modes 10 and 11) is not stored and comes from the initial state"""
    return np.stack([A.get(f"traj_m{mode}_q{q}", A["state"][q]) for q in range(3)])


def golden_record(meta, mode):
    """(t, h, steps, steps_total), t and h as hex"""
    t, h, steps, total = meta[f"traj_m{mode}"]
    return (float.fromhex(t).hex(), float.fromhex(h).hex(), steps, total)


def grid_case(dims, perturbed):
    """(info, Pm, state) of one of GRIDS: the g20 golden's parameters and domain at those dimensions,
    with perturbed_params() if perturbed, and the edge state drawn for those parameters"""
    import _oracle as O
    key = ("grid", tuple(dims), bool(perturbed))
    if key not in _cache:
        Pm, info = O.params_from_meta(O.load_case("g20")[0])
        n1, n2, n3 = dims
        info = dict(info, n1=n1, n2=n2, n3=n3)
        if perturbed:
            Pm = perturbed_params(Pm)
        x = edge_state(n1, n2, n3, Pm)
        x.setflags(write=False)
        _cache[key] = (info, Pm, x)
    return _cache[key]


def oracle_rhs(dims, perturbed, mode, t=100.0):
    """O.rhs of grid_case(), computed once"""
    import _oracle as O
    key = ("rhs", tuple(dims), bool(perturbed), mode, t)
    if key not in _cache:
        info, Pm, x = grid_case(dims, perturbed)
        K = O.rhs(info, Pm, mode, t, np.array(x))[0]
        K.setflags(write=False)
        _cache[key] = K
    return _cache[key]


def oracle_steps(dims, perturbed, mode, noise=None):
    """((t, h, steps, steps_total) with t, h as hex, final state) of the oracle's six attempted steps
    from h = 1 on grid_case(), computed once; noise: the u_noise field [k][j][i] or None"""
    import _oracle as O
    key = ("steps", tuple(dims), bool(perturbed), mode, None if noise is None else noise.tobytes())
    if key not in _cache:
        info, Pm, x = grid_case(dims, perturbed)
        t, h, steps, total, rc, out = O.solve(info, Pm, mode, np.array(x), 0.0, 1.0, [1e9],
                                              max_steps_total=ATTEMPTS, noise=noise)[0]
        assert rc == 2
        out.setflags(write=False)
        _cache[key] = ((t.hex(), h.hex(), steps, total), out)
    return _cache[key]


def branch_fractions(x, Pm):
    """the fractions of cells on each branch the right-hand side takes from p and gl alone"""
    p, gl = x[1], x[2]
    e0, e1, zeta = (float(Pm[_idx(k)]) for k in ("p_eps0", "p_eps1", "zeta"))
    q = 1.0 - p
    wi = 1.0 - zeta * gl
    return {
        "p<0": float((p < 0).mean()), "p>1": float((p > 1).mean()),
        "sshape(p)=0": float((p <= e0).mean()), "sshape(p)=1": float((p >= e1).mean()),
        "sshape(p) cubic": float(((p > e0) & (p < e1)).mean()),
        "sshape(1-p)=0": float((q <= e0).mean()), "sshape(1-p)=1": float((q >= e1).mean()),
        "sshape(1-p) cubic": float(((q > e0) & (q < e1)).mean()),
        "1-zeta*gl<=0": float((wi <= 0).mean()), "1-zeta*gl>0": float((wi > 0).mean()),
        "u=u_star": float((x[0] == float(Pm[_idx("u_star")])).mean()),
    }
